"""A fixed grid of GEMM queries that sits on every threshold of csrc/gemm_plan.h, and how to ask a built library and the stand-alone planner
(tests/gemm_plan_sweep.cpp) for the answer to one.  Used by tests/test_gemm_plan_cpu.py and tools/route_grid.py; nothing here touches a device.

A query is the tuple of GemmQuery's fields in order:
    (mode, dtype, M, N, K, ldx, ldw, ldy, ldaux, ldres, bias, y_pre, aux, res, rowscale, epi, rows_per_scale, x_epi)
mode 0-3 as fmmt_linear_fwd_route (forward, seg3 along N, seg3 along K, split-K), 4 / 5 = fmmt_linear_wgrad / _partials (ldy is dy's pitch).
An answer is (route or negative FMMT_E*, workspace bytes or -1): the bytes of fmmt_linear_splitk_workspace for mode 3, of fmmt_linear_wgrad_workspace
for modes 4 / 5."""
import ctypes as C
import itertools

F32, BF16 = 0, 1

# thresholds of the planners, each with its neighbours: 128 (few-token TN: more than), 256 (64-row tiles of wide outputs), 768 (one TN split), 2048 (few-token TN:
# up to), 4096 (64- / 128-row tiles, phase kernels from), 8192 (DMA-staged TN: more than, multiples of 64), 16384 (persistent kernel, full rounds), 65536 (deep
# kernels), 262144 (TN token step and split target); 501760 = Swin stage 0; small odd sizes in front
MS = [1, 8, 70, 127, 128, 129, 255, 256, 257, 640, 767, 768, 769, 2047, 2048, 2049, 4095, 4096, 4097, 7840, 8191, 8192, 8193, 8256, 16383, 16384, 16385, 31360,
      65535, 65536, 65537, 125440, 262143, 262144, 262145, 262208, 501760]
NKS = [8, 48, 64, 96, 128, 192, 256, 288, 384, 512, 576, 768, 1152, 1536, 2048, 2304, 3072, 4096, 6144, 37632]
RPS = [0, 1, 31, 32, 49]
# one (M, N, K) per kernel family and a few beside: where pitches, epilogues and operands are varied
SHAPES = [(70, 96, 96), (70, 768, 768), (640, 768, 3072), (1328, 3072, 768), (2048, 128, 48), (4096, 37632, 512), (200, 37632, 512), (4097, 96, 96), (4104, 128, 64),
          (7840, 1536, 1536), (7840, 1536, 6144), (8192, 2048, 192), (8192, 1024, 192), (8192, 288, 200), (16384, 1024, 128), (16384, 768, 128), (16384, 128, 128),
          (31360, 768, 768), (31360, 768, 3072), (31360, 3072, 768), (31360, 2304, 768), (56072, 384, 192), (65536, 128, 96), (65544, 128, 576), (65536, 96, 192),
          (65536, 288, 96), (65536, 128, 1152), (125440, 384, 384), (125440, 1152, 384), (125440, 1536, 384), (125440, 384, 1536), (501760, 192, 768),
          (501760, 96, 96), (501760, 768, 192), (501760, 576, 192), (8256, 256, 256), (9000, 1024, 1024), (16384, 192, 384), (500, 96, 96), (2048, 64, 512)]


def _q(mode, dt, M, N, K, ldx=None, ldw=None, ldy=None, ldaux=None, ldres=None, bias=0, y_pre=0, aux=0, res=0, rowscale=0, epi=0, rps=1, x_epi=0):
    ldy = N if ldy is None else ldy
    wcols = K // 3 if mode == 2 else K
    return (mode, dt, M, N, K, K if ldx is None else ldx, wcols if ldw is None else ldw, ldy, ldy if ldaux is None else ldaux, ldy if ldres is None else ldres,
            bias, y_pre, aux, res, rowscale, epi, rps, x_epi)


def _pitches(width):
    """equal to the width, width + 8, width + 4 (refused in bf16), below the width (refused)"""
    return [width, width + 8, width + 4, width - 8]


# forward epilogues of the model: plain + bias, GELU + pre-activation, residual + DropPath scale, GELU' from the pre-activation, product with the stored derivative
FWD_KINDS = [dict(bias=1), dict(bias=1, epi=1, y_pre=1), dict(bias=1, res=1, rowscale=1, rps=49), dict(epi=2, aux=1), dict(epi=4, aux=1), dict(rowscale=1, rps=49)]


def grid():
    out = []
    # every shape, contiguous: forward by epilogue kind, split-K, weight gradient (plain, scaled, recomputed activation) in both modes
    for M, N, K in itertools.product(MS, NKS, NKS):
        for kind in FWD_KINDS:
            out.append(_q(0, BF16, M, N, K, **kind))
        out.append(_q(0, F32, M, N, K, bias=1))
        for dt in (BF16, F32):
            out.append(_q(3, dt, M, N, K, bias=1))
        for mode in (4, 5):
            out.append(_q(mode, BF16, M, N, K))
            out.append(_q(mode, BF16, M, N, K, rowscale=1, rps=49))
            out.append(_q(mode, BF16, M, N, K, x_epi=1))
            out.append(_q(mode, F32, M, N, K))
    for M, N, K in SHAPES:
        # pitches, one operand at a time and all together
        for dt in (BF16, F32):
            for kind in FWD_KINDS:
                for name, width in (("ldx", K), ("ldw", K), ("ldy", N), ("ldaux", N), ("ldres", N)):
                    for ld in _pitches(width)[1:]:
                        out.append(_q(0, dt, M, N, K, **{name: ld}, **kind))
                out.append(_q(0, dt, M, N, K, ldx=K + 8, ldw=K + 16, ldy=N + 8, ldaux=N + 16, ldres=N + 24, **kind))
            for name, width in (("ldx", K), ("ldw", K), ("ldy", N)):
                for ld in _pitches(width)[1:]:
                    out.append(_q(3, dt, M, N, K, **{name: ld}))
            for mode in (4, 5):
                for name, width in (("ldx", K), ("ldy", N)):
                    for ld in _pitches(width)[1:]:
                        out.append(_q(mode, dt, M, N, K, **{name: ld}))
                        out.append(_q(mode, dt, M, N, K, rowscale=1, rps=49, **{name: ld}))
        # every epilogue value (and one on either side) x presence of every operand x rows_per_scale
        for epi in (-1, 0, 1, 2, 3, 4, 5):
            for bias, y_pre, aux, res, rowscale in itertools.product((0, 1), repeat=5):
                for rps in (RPS if rowscale else [1, 0]):
                    out.append(_q(0, BF16, M, N, K, bias=bias, y_pre=y_pre, aux=aux, res=res, rowscale=rowscale, epi=epi, rps=rps))
        for mode in (4, 5):
            for rps in RPS:
                for x_epi in (0, 1, 2):
                    out.append(_q(mode, BF16, M, N, K, rowscale=1, rps=rps, x_epi=x_epi))
    # rows x pitch on either side of 2^31 elements: x, y, the M x N operands (M = 2^20), the weight (N = 4096)
    M = 1 << 20
    for ld in (2040, 2048, 2056):
        for kind in FWD_KINDS:
            out.append(_q(0, BF16, M, 1024, 1024, ldx=ld, **kind))
            out.append(_q(0, BF16, M, 1024, 1024, ldy=ld, **kind))
            out.append(_q(0, BF16, M, 1024, 1024, ldaux=ld, ldres=ld, **kind))
            out.append(_q(0, BF16, M, 384, 384, ldx=ld, ldres=ld, **kind))
    for ldw in ((1 << 19) - 8, 1 << 19, (1 << 19) + 8):
        for M in (8192, 16384, 65536):
            out.append(_q(0, BF16, M, 4096, 128, ldw=ldw, bias=1))
    # three weights in one launch: along N and along K
    for mode in (1, 2):
        for M, N, K in itertools.product([1, 70, 128, 129, 2047, 2048, 2049, 4096, 4097], [64, 96, 192, 384, 576, 768, 1536, 2304, 3072, 6144, 37632], [64, 96, 128, 192, 384, 576, 768, 1536, 2048, 2304, 6144]):
            for dt in (BF16, F32):
                for bias in (0, 1):
                    out.append(_q(mode, dt, M, N, K, bias=bias))
            wcols = K // 3 if mode == 2 else K
            for name, width in (("ldx", K), ("ldw", wcols), ("ldy", N)):
                for ld in _pitches(width)[1:]:
                    out.append(_q(mode, BF16, M, N, K, **{name: ld}))
    return out


def load(path):
    lib = C.CDLL(path)
    lib.fmmt_linear_fwd_route.restype = C.c_int
    lib.fmmt_linear_fwd_route.argtypes = [C.c_int] * 17
    lib.fmmt_linear_wgrad_route.restype = C.c_int
    lib.fmmt_linear_wgrad_route.argtypes = [C.c_int] * 10
    lib.fmmt_linear_wgrad_workspace.restype = C.c_size_t
    lib.fmmt_linear_wgrad_workspace.argtypes = [C.c_int] * 4
    lib.fmmt_linear_splitk_workspace.restype = C.c_size_t
    lib.fmmt_linear_splitk_workspace.argtypes = [C.c_int] * 3
    return lib


def ask(lib, q):
    mode, dt, M, N, K, ldx, ldw, ldy, ldaux, ldres, bias, y_pre, aux, res, rowscale, epi, rps, x_epi = q
    if mode <= 3:
        route = lib.fmmt_linear_fwd_route(dt, M, N, K, ldx, ldw, ldy, bias, y_pre, epi, aux, ldaux, res, ldres, rowscale, rps, mode)
        return route, (lib.fmmt_linear_splitk_workspace(M, N, K) if mode == 3 else -1)
    return lib.fmmt_linear_wgrad_route(dt, M, N, K, ldy, ldx, rowscale, rps, x_epi, mode - 4), lib.fmmt_linear_wgrad_workspace(dt, M, N, K)
