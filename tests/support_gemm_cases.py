"""The case table of the strided GEMM tests: one row per kernel family (enum fmmt_route, include/fmmt_route.h) and epilogue, at the smallest shape the
dispatch sends there.  tests/test_gemm_routes_cpu.py holds every row's expected route to the route query (which IS the dispatch) and requires every
value of the enum to be reached by a row with leading dimensions different from the row widths; tests/test_gpu_gemm_strided.py runs the rows.

No torch here: a row is plain data.  Layouts (lds below; built by tests/support_strided.make): "pitch" = row pitch width + 8 on every operand and output, "packed" = every
matrix the middle third of a (rows, 3 * width) buffer, "pitch4" (fp32) = ldy / ldres / ldaux = width + 4 with x / w at width + 8, "bigx" = an x whose
pitch puts the last rows' byte offsets between 2^31 and 2^32 (Nt.ldx)."""
import os
import re
from dataclasses import dataclass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI_NONE, EPI_GELU, EPI_GELU_BWD, EPI_GELU_DG, EPI_MUL_AUX = 0, 1, 2, 3, 4


def route_enum():
    """name -> value of enum fmmt_route, read from the header (FMMT_ROUTE_COUNT left out)"""
    src = open(os.path.join(ROOT, "include", "fmmt_route.h")).read()
    body = src[src.index("enum fmmt_route {"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("};")], flags=re.S)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"FMMT_ROUTE_(\w+) = (\d+)", body) if m.group(1) != "COUNT"}


@dataclass(frozen=True)
class Nt:
    """y = epi(x w^T + bias); y = res + rowscale * y: fmmt_linear_fwd (mode 'fwd'), fmmt_linear_fwd_seg3 ('seg3n' / 'seg3k') or fmmt_linear_fwd_splitk ('splitk')"""
    route: str
    dt: str                     # "bf16" / "f32"
    M: int
    N: int
    K: int
    epi: int = EPI_NONE
    bias: bool = True
    pre: bool = False           # y_pre
    aux: bool = False
    res: bool = False
    rps: int = 0                # rows per scale of the DropPath row scale; 0 = none
    mode: str = "fwd"
    layouts: tuple = ("pitch", "packed")
    ldx: int = 0                # layout "bigx"

    @property
    def id(self):
        ops = "".join(s for s, on in (("+b", self.bias), ("+pre", self.pre), ("+aux", self.aux), ("+res", self.res), (f"+rs{self.rps}", self.rps)) if on)
        return f"{self.route}-{self.dt}-{self.M}x{self.N}x{self.K}-{self.mode}-e{self.epi}{ops}" + (f"-ldx{self.ldx}" if self.ldx else "")


@dataclass(frozen=True)
class Tn:
    """dw = (s dy)^T x (x_epi: gelu(x)), db = colsum(s dy): fmmt_linear_wgrad"""
    route: str
    dt: str
    M: int
    N: int
    K: int
    rps: int = 0                # 0 = unscaled
    two_valued: bool = True     # the scale DropPath hands over: 0 or 1 / keep
    x_gelu: bool = False
    layouts: tuple = ("pitch", "packed")

    @property
    def id(self):
        return f"{self.route}-{self.dt}-{self.M}x{self.N}x{self.K}" + (f"-rs{self.rps}{'' if self.two_valued else 'g'}" if self.rps else "") + ("-xgelu" if self.x_gelu else "")


B, F = "bf16", "f32"
F_LAYOUTS = ("pitch", "packed", "pitch4")

NT_CASES = [
    # --- bf16, tokens <= 4096
    Nt("NT_QUARTER", B, 70, 128, 128),
    Nt("NT_QUARTER", B, 70, 128, 128, res=True, rps=7),
    Nt("NT_QUARTER", B, 70, 128, 128, epi=EPI_GELU, pre=True),
    Nt("NT_QUARTER_R4", B, 70, 128, 2048),
    Nt("NT_SEG3", B, 70, 192, 128, mode="seg3n"),
    Nt("NT_SEG3", B, 70, 64, 192, mode="seg3k", bias=False),
    Nt("NT_SEG3_R4", B, 70, 192, 2048, mode="seg3n"),
    Nt("NT_SEG3_R4", B, 70, 64, 6144, mode="seg3k", bias=False),
    Nt("NT64_K96", B, 70, 96, 96),
    Nt("NT64_K96", B, 70, 160, 96),                                           # a ragged channel tile
    Nt("NT64_K96", B, 70, 96, 96, epi=EPI_GELU_DG, pre=True),
    Nt("NT64_K64", B, 70, 96, 48),
    Nt("NT64_DMA", B, 70, 96, 128),
    Nt("NT64_DMA", B, 70, 96, 128, epi=EPI_GELU_BWD, aux=True, bias=False, rps=7),
    Nt("NT64_DMA_R4", B, 70, 96, 2048),
    Nt("NT64_BK32", B, 70, 96, 160),
    Nt("NT64_BK32", B, 70, 96, 72),                                           # K tails that are not a multiple of the K step
    Nt("NT64_BK32", B, 70, 128, 104),
    Nt("NT64_BK32", B, 70, 128, 104, epi=EPI_MUL_AUX, aux=True, bias=False, res=True),
    # --- bf16, 128-row forms
    Nt("NT128_K96", B, 4104, 96, 96),
    Nt("NT128_K64", B, 4104, 96, 48),
    Nt("NT128_DMA", B, 4104, 96, 128),
    Nt("NT128_DMA", B, 4104, 96, 128, res=True, rps=49),
    Nt("NT128_BK32", B, 4104, 96, 160),
    Nt("NT128_BK32", B, 4104, 96, 72),
    Nt("NT128_BK32", B, 4104, 128, 104),
    # --- phase kernels
    Nt("PH", B, 8192, 2048, 192),
    Nt("PH3_PLAIN", B, 7840, 1536, 192),
    Nt("PH3_OP", B, 7840, 1536, 192, res=True, rps=49),
    Nt("PH3_OP", B, 7840, 1536, 192, bias=False, rps=49),
    Nt("PH3_MUL_AUX", B, 7840, 1536, 192, epi=EPI_MUL_AUX, aux=True, bias=False),
    Nt("PH3_GELU_PRE", B, 7848, 1536, 1536, epi=EPI_GELU, pre=True),
    Nt("PH3W_PLAIN", B, 56072, 384, 192),
    Nt("PH3W_OP", B, 56072, 384, 192, res=True),
    Nt("PH3W_MUL_AUX", B, 56072, 384, 192, epi=EPI_MUL_AUX, aux=True, bias=False),
    # --- persistent 256-row kernel
    Nt("P256_256", B, 16384, 1024, 128),
    Nt("P256_192", B, 16384, 768, 128),
    Nt("P256_128", B, 16384, 512, 128),
    Nt("P256_192_OP", B, 16384, 768, 128, res=True),
    Nt("P256_128_OP", B, 16384, 1024, 128, res=True, rps=64),
    Nt("P256_128_OP", B, 16384, 512, 128, bias=False, rps=64),
    Nt("P256_256_PIPE", B, 16400, 1536, 384),
    Nt("P256_192_PIPE", B, 16384, 768, 384),
    Nt("P256_128_PIPE", B, 16384, 512, 384),
    # --- 256-row deep kernels
    Nt("DEEP32_K96_N128", B, 65544, 128, 96),
    Nt("DEEP32_K96_N96", B, 65544, 96, 96),
    Nt("DEEP32_K192_N128", B, 65544, 128, 192),
    Nt("DEEP32_K192_N96", B, 65544, 96, 192),
    Nt("DEEP32_N128", B, 65544, 128, 160),
    Nt("DEEP32_N96", B, 65544, 96, 160),
    Nt("DEEP32_N128", B, 65544, 128, 160, epi=EPI_GELU_DG, pre=True),
    Nt("DEEP32_N96", B, 65544, 96, 160, epi=EPI_GELU_BWD, aux=True, bias=False, res=True, rps=196),
    Nt("DEEP", B, 65544, 128, 576),
    # --- split-K (the route of the contraction; its finish is one kernel)
    Nt("NT64_BK64", B, 8, 128, 4096, mode="splitk"),
    Nt("NT64_BK32", B, 8, 128, 4104, mode="splitk"),
    Nt("NT128_BK64", B, 4104, 128, 4096, mode="splitk"),
    Nt("NT64_F32", F, 8, 128, 4096, mode="splitk", layouts=F_LAYOUTS),
    # --- fp32 parity kernel
    Nt("NT64_F32", F, 70, 96, 96, layouts=F_LAYOUTS),
    Nt("NT64_F32", F, 70, 96, 20, layouts=F_LAYOUTS),
    Nt("NT64_F32", F, 70, 96, 96, epi=EPI_GELU, pre=True, res=True, rps=7, layouts=F_LAYOUTS),
    Nt("NT128_F32", F, 4104, 128, 64, layouts=F_LAYOUTS),
    # --- byte offsets of x between 2^31 and 2^32 in the two kernels that form them as unsigned 32-bit values
    # (rows are clamped to M - 1: it is (M - 1) * ldx * 2 that must pass 2^31, with M * ldx < 2^31 elements so that the route stays.  A third of the rows
    #  of each case start past 2^31 bytes, the last near 3.2e9; tests/test_gemm_routes_cpu.py holds the arithmetic)
    Nt("P256_256", B, 16384, 1024, 128, layouts=("bigx",), ldx=98312),
    Nt("PH3_PLAIN", B, 8192, 1024, 192, layouts=("bigx",), ldx=196616),
]

TN_CASES = [
    Tn("TN_FEW", B, 300, 128, 256),
    Tn("TN_REG32_FEW", B, 100, 96, 96),
    Tn("TN_REG32_FEW", B, 3000, 96, 48),
    Tn("TN_REG64", B, 5000, 96, 384),
    Tn("TN_REG64", B, 5000, 96, 384, rps=49, two_valued=False, x_gelu=True),
    Tn("TN_REG32", B, 262145, 8, 8),                                          # the smallest M past the 64-token form: a one-row ragged tail
    Tn("TN_F32", F, 500, 96, 96, layouts=F_LAYOUTS[:2]),
    Tn("TN_F32", F, 500, 96, 96, rps=100, two_valued=False, layouts=F_LAYOUTS[:2]),
    # the DMA-staged tiles at the fewest tokens tn_plan_dma admits (M > 8192, M % 64 == 0, chunk >= 512: at least 16 tiles at 8256 tokens)
    Tn("TN_DMA_256", B, 8256, 1024, 1024),
    Tn("TN_DMA_256_SCALED", B, 8256, 1024, 1024, rps=64),
    Tn("TN_DMA_192", B, 8256, 576, 2304),
    Tn("TN_DMA_192_SCALED", B, 8256, 576, 2304, rps=64),
    Tn("TN_DMA_384", B, 8256, 6144, 192),
    Tn("TN_DMA_384", B, 65600, 576, 192),                                     # N 192 short of two tiles: padded partials, rows dropped by the finish
    Tn("TN_REG64", B, 8256, 6144, 192, rps=64),                               # the <384,192> tile is unscaled-only: the scaled launch stays register-staged
]

# fmmt_colsum (the bias gradient beside the vendor library's GEMMs) takes a leading dimension too: (dtype, M, N), each with the output in dtype and in fp32.
# Ragged row counts on both sides of its 256-row loop, a last column block that is partly past N, a single 16-byte chunk.
COLSUM_CASES = [(B, 777, 1032), (B, 63, 8), (B, 2049, 64), (F, 1000, 516)]

# Routes that the contract makes unreachable with ld != width (none: every kernel family takes leading dimensions)
UNREACHABLE_WITH_LD = ()


def layout_of(name, width):
    """(ld, col) of a matrix of `width` elements in one of the layouts every matrix can take"""
    return {"contig": (width, 0), "pitch": (width + 8, 0), "packed": (3 * width, width)}[name]


def lds(case, layout):
    """(ld, col) per matrix name for one layout of a case: x, w, y (and pre), aux, res -- or dy, x for a Tn row"""
    def one(width, name):
        if layout == "pitch4":
            assert case.dt == F                                    # 4 elements are 16 bytes in fp32 only
            return (width + 4, 0) if name in ("y", "aux", "res") else (width + 8, 0)
        if layout == "bigx":
            return (case.ldx, 0) if name == "x" else (width, 0)
        return layout_of(layout, width)
    if isinstance(case, Tn):
        return {"dy": one(case.N, "dy"), "x": one(case.K, "x")}
    wk = case.K // 3 if case.mode == "seg3k" else case.K
    return {"x": one(case.K, "x"), "w": one(wk, "w"), "y": one(case.N, "y"), "aux": one(case.N, "aux"), "res": one(case.N, "res")}


def query_route(lib, case, layout):
    """the route query for one layout of a case: the value the dispatch of the real entry point would take"""
    dt = 1 if case.dt == B else 0
    ld = lds(case, layout)
    if isinstance(case, Tn):
        return lib.fmmt_linear_wgrad_route(dt, case.M, case.N, case.K, ld["dy"][0], ld["x"][0], 1 if case.rps else 0, max(case.rps, 1), EPI_GELU if case.x_gelu else 0, 0)
    mode = {"fwd": 0, "seg3n": 1, "seg3k": 2, "splitk": 3}[case.mode]
    return lib.fmmt_linear_fwd_route(dt, case.M, case.N, case.K, ld["x"][0], ld["w"][0], ld["y"][0], int(case.bias), int(case.pre), case.epi,
                                     int(case.aux), ld["aux"][0], int(case.res), ld["res"][0], 1 if case.rps else 0, max(case.rps, 1), mode)
