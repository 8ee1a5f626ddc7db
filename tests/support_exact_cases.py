"""Exact integer operands and an a-priori error bound for every GEMM route: the data tests/test_exact_cases_cpu.py (no GPU) and
tests/test_gpu_gemm_exact.py (the kernels) share.  Built on the rows of tests/support_gemm_cases.py -- no new shapes.  No torch at import: the
tables are plain data; the functions that build tensors take whatever device they are given and import torch when called.

Why integers.  A bf16 x bf16 product is exact in fp32 (8 + 8 significand bits).  If every operand is a small integer and every partial sum of
absolute values stays below 2^24, every fp32 partial sum is an integer below 2^24, hence exact, in ANY order: any tiling, K split, pipeline depth
or MFMA shape.  The value in front of the store is then one known integer (a half-integer below 2^23 where a row scale of 0.5 takes part), and
the stored element must be its single round-to-nearest-even image, bit for bit.  A truncating store, a second rounding, a partial kept below fp32
or an error confined to small outputs all change bits.

The recipe of a row (`nt_recipe`, `tn_recipe`, `colsum_recipe`): operand magnitudes from a ladder, largest first, the first rung whose WORST-CASE
epilogue value -- every operand at its largest magnitude, all signs aligned -- stays below the limit:
    NT   worst = ((|x| |w| K + |bias|) * |aux|) * max|rowscale| + |res|          limit 2^24, 2^23 with a row scale (its 0.5 makes half-integers)
    TN   worst = M |dy| |x| max|s|   (db: M |dy| max|s|)                         limit 2^24, 2^23 with a general scale (0.5)
    colsum worst = M |x|                                                         limit 2^24
x uses all 8 significand bits (|x| <= 255); bias fp32 integers |b| <= 100; res bf16 integers |r| <= 256; aux integers |a| <= 7; row scales from
{0, 0.5, 1, 2} with zeros (dropped samples); TN two-valued scales {0, 2}, general ones {-1, 0, 0.5, 1, 2}.  Every product of a scale with an
operand is itself exactly representable in bf16 (|s dy| <= 14 in halves), so the register-staged weight gradient's rounding of s * dy
(gemm.hip, linear_tn_kernel lstore: `R.a[i].set(e, R.a[i].get(e) * R.s[i])`) changes nothing on these operands.

Exactly determined outputs (`nt_exact_outputs`, `tn_exact_outputs`): y for EPI_NONE / EPI_MUL_AUX (with or without res / rowscale), seg3 and
split-K rows; y_pre (the pre-activation) alone for EPI_GELU; dw and db for TN rows without x_gelu; both output types of fmmt_colsum.  GELU
values, the GELU_DG derivative slot, GELU_BWD outputs and the x_gelu TN row are transcendental and stay with the tests they have.

The bound for REAL operands (`nt_bound`, `tn_bound`), for an element stored in type T with unit round-off u_T (bf16 2^-8, fp32 0):
    |got - ref64| <= u_T |ref64| + (1 + u_T) * (n u / (1 - n u)) * S + extra,      u = 2^-24,  n = L + e
L the contraction length (K for NT, M for TN, M for colsum); e the number of fp32 epilogue operations behind the contraction (bias add, aux
product, row-scale product, residual add: one rounding each; L itself already pays for L - 1 additions of exact products plus one spare);
S the same contraction on absolute values carried through the epilogue's linear operations (|rs| (S + |bias|) |aux| + |res|).  n u / (1 - n u)
is the worst case of an fp32 sum of n exact terms in any order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4: c = 1) --
derived, not measured.  `extra` is a rounding the contract documents, charged only to the routes that have it (EXTRA_ROUNDINGS)."""
import zlib
from dataclasses import dataclass

from tests import support_gemm_cases as GC

LIMIT = float(1 << 24)
U32 = 2.0 ** -24
U_T = {"bf16": 2.0 ** -8, "f32": 0.0}

X_W_LADDER = [(255, 7), (255, 3), (127, 3), (63, 3), (31, 1)]
DY_X_LADDER = [(7, 15), (7, 7), (3, 7), (3, 3), (1, 3), (1, 1)]
BIAS_MAX, RES_MAX, AUX_MAX, COLSUM_MAX = 100, 256, 7, 255
NT_SCALES = (0.0, 0.5, 1.0, 2.0)
TN_TWO_VALUED = (0.0, 2.0)
TN_GENERAL = (-1.0, 0.0, 0.5, 1.0, 2.0)

# Documented roundings below fp32, by route: (routes, condition, term, where it was read).  The term is a multiple of S.
REG_STAGED_TN = ("TN_REG32", "TN_REG32_FEW", "TN_REG64")
EXTRA_ROUNDINGS = [
    (REG_STAGED_TN, "a row scale is given", U_T["bf16"],
     "facialmmt_amd/csrc/gemm.hip, linear_tn_kernel, lstore(): R.a[i].set(e, R.a[i].get(e) * R.s[i]) -- s * dy is stored to LDS in the element type "
     "(tests/support_op_cases.py:189,201 state the same); db sums the rounded values (colsum[e] += R.a[i].get(e))"),
]


@dataclass(frozen=True)
class Recipe:
    x: int                      # NT: |x|; TN: |dy|
    w: int                      # NT: |w|; TN: |x|
    bias: int = 0
    aux: int = 0
    res: int = 0
    scales: tuple = ()
    worst: float = 0.0          # the worst-case value in front of the store
    limit: float = LIMIT


def nt_exact_outputs(case):
    """names of the outputs the integer recipe determines exactly"""
    if case.epi in (GC.EPI_NONE, GC.EPI_MUL_AUX):
        return ("y",)
    if case.epi == GC.EPI_GELU and case.pre:
        return ("y_pre",)
    return ()


def tn_exact_outputs(case):
    return () if case.x_gelu else ("dw", "db")


def nt_worst(case, x, w):
    v = float(x) * w * case.K + (BIAS_MAX if case.bias else 0)
    if case.epi == GC.EPI_MUL_AUX:
        v *= AUX_MAX
    if case.rps:
        v *= max(NT_SCALES)
    return v + (RES_MAX if case.res else 0)


def nt_recipe(case):
    limit = LIMIT / 2 if case.rps else LIMIT
    for x, w in X_W_LADDER:
        worst = nt_worst(case, x, w)
        if worst < limit:
            return Recipe(x, w, BIAS_MAX if case.bias else 0, AUX_MAX if case.aux else 0, RES_MAX if case.res else 0, NT_SCALES if case.rps else (), worst, limit)
    raise AssertionError(f"no rung of the ladder keeps {case.id} exact")


def tn_scales(case):
    return () if not case.rps else (TN_TWO_VALUED if case.two_valued else TN_GENERAL)


def tn_recipe(case):
    sc = tn_scales(case)
    smax = max((abs(s) for s in sc), default=1.0)
    limit = LIMIT / 2 if 0.5 in sc else LIMIT
    for dy, x in DY_X_LADDER:
        worst = float(case.M) * dy * x * smax
        if worst < limit:
            return Recipe(dy, x, scales=sc, worst=worst, limit=limit)
    raise AssertionError(f"no rung of the ladder keeps {case.id} exact")


def colsum_recipe(dt, M, N):
    return Recipe(COLSUM_MAX, 0, worst=float(M) * COLSUM_MAX)


def seed_of(name):
    return zlib.crc32(name.encode())


# ------------------------------------------------------------------------------------------------ operands (torch from here on)
def _torch():
    import torch
    return torch


def _dt(name):
    torch = _torch()
    return {"bf16": torch.bfloat16, "f32": torch.float32}[name]


def _ints(g, shape, amax, dtype, device):
    torch = _torch()
    return torch.randint(-amax, amax + 1, shape, generator=g, device=device).to(dtype)


def _pick(g, n, values, device):
    """n row scales from `values`, every value present where n allows, a zero at index 1 (a dropped sample)"""
    torch = _torch()
    tab = torch.tensor(values, dtype=torch.float32, device=device)
    s = tab[torch.randint(0, len(values), (n,), generator=g, device=device)]
    s[:min(n, len(values))] = tab[:min(n, len(values))]
    if n > 1:
        s[1] = 0.0
    return s


def _generator(name, device):
    torch = _torch()
    g = torch.Generator(device=device)
    g.manual_seed(seed_of(name))
    return g


def nt_int_values(case, device="cpu"):
    """integer operands of an Nt row: x, w (element type), bias (fp32), aux, res (element type), rs (fp32) -- None where the row has none"""
    r, g, dt = nt_recipe(case), _generator("int " + case.id, device), _dt(case.dt)
    M, N, K = case.M, case.N, case.K
    v = {"x": _ints(g, (M, K), r.x, dt, device), "w": _ints(g, (N, K), r.w, dt, device)}
    v["bias"] = _ints(g, (N,), r.bias, _torch().float32, device) if case.bias else None
    v["aux"] = _ints(g, (M, N), r.aux, dt, device) if case.aux else None
    v["res"] = _ints(g, (M, N), r.res, dt, device) if case.res else None
    v["rs"] = _pick(g, (M + case.rps - 1) // case.rps, r.scales, device) if case.rps else None
    return v


def nt_real_values(case, device="cpu"):
    """the operand distributions of tests/test_gpu_gemm_strided.py: unit normals, w scaled by K^-1/2, bias 0.1, row scales rand + 0.5 with zeros"""
    torch = _torch()
    g, dt = _generator(case.id, device), _dt(case.dt)
    M, N, K = case.M, case.N, case.K

    def randn(shape, dtype, scale=1.0):
        return (torch.randn(shape, device=device, generator=g) * scale).to(dtype)
    v = {"x": randn((M, K), dt), "w": randn((N, K), dt, K ** -0.5)}
    v["bias"] = randn((N,), torch.float32, 0.1) if case.bias else None
    v["aux"] = randn((M, N), dt) if case.aux else None
    v["res"] = randn((M, N), dt) if case.res else None
    v["rs"] = None
    if case.rps:
        rs = torch.rand((M + case.rps - 1) // case.rps, device=device, generator=g) + 0.5
        rs[1::5] = 0.0
        v["rs"] = rs
    return v


def _rows(case, rs):
    return rs.repeat_interleave(case.rps)[:case.M, None]


def nt_reference(case, v, absolute=False):
    """{name: fp64 tensor} of the exactly determined outputs: the product in fp64, the epilogue's linear operations in fp64, nothing rounded.
    absolute=True: the same on absolute values (S of the bound)."""
    torch = _torch()
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    acc = f(v["x"]) @ f(v["w"]).t()
    if v["bias"] is not None:
        acc = acc + f(v["bias"])
    out = {}
    if case.epi == GC.EPI_GELU:
        if case.pre:
            out["y_pre"] = acc
        return out
    if case.epi not in (GC.EPI_NONE, GC.EPI_MUL_AUX):
        return out
    y = acc * f(v["aux"]) if case.epi == GC.EPI_MUL_AUX else acc
    if v["rs"] is not None:
        y = y * _rows(case, f(v["rs"]))
    if v["res"] is not None:
        y = y + f(v["res"])
    out["y"] = y
    return out


def nt_epilogue_ops(case, name):
    """fp32 operations between the contraction and the store of output `name`"""
    e = int(case.bias)
    if name == "y":
        e += int(case.epi == GC.EPI_MUL_AUX) + int(bool(case.rps)) + int(case.res)
    return e


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def bound(ref, S, n, u_t, extra=0.0):
    """the a-priori bound, elementwise (fp64)"""
    return u_t * ref.abs() + (1.0 + u_t) * (gamma(n) + extra) * S


def worst_ratio(err, bnd):
    """max err / bound; where the bound is 0 (a dropped sample's row without a residual, an aux of exactly 0: ref and S both 0) the error must be 0 too"""
    torch = _torch()
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max().item())


def nt_bound(case, name, ref, S):
    return bound(ref, S, case.K + nt_epilogue_ops(case, name), U_T[case.dt])


def tn_int_values(case, device="cpu"):
    r, g, dt = tn_recipe(case), _generator("int " + case.id, device), _dt(case.dt)
    v = {"dy": _ints(g, (case.M, case.N), r.x, dt, device), "x": _ints(g, (case.M, case.K), r.w, dt, device), "rs": None}
    if case.rps:
        n = (case.M + case.rps - 1) // case.rps
        if case.two_valued:
            torch = _torch()
            rs = torch.full((n,), TN_TWO_VALUED[1], device=device)
            rs[::7] = 0.0
            rs[-1] = 0.0
            v["rs"] = rs
        else:
            v["rs"] = _pick(g, n, r.scales, device)
    return v


def tn_real_values(case, device="cpu"):
    torch = _torch()
    g, dt = _generator(case.id, device), _dt(case.dt)
    v = {"dy": torch.randn((case.M, case.N), device=device, generator=g).to(dt), "x": torch.randn((case.M, case.K), device=device, generator=g).to(dt), "rs": None}
    if case.rps:
        n = (case.M + case.rps - 1) // case.rps
        if case.two_valued:
            rs = torch.full((n,), 1.0 / 0.9, device=device)
            rs[::7] = 0.0
            rs[-1] = 0.0
        else:
            rs = torch.rand(n, device=device, generator=g) + 0.5
            rs[1] = 0.0
        v["rs"] = rs
    return v


def tn_reference(case, v, absolute=False):
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    sdy = f(v["dy"])
    if v["rs"] is not None:
        sdy = sdy * _rows(case, f(v["rs"]))
    return {"dw": sdy.t() @ f(v["x"]), "db": sdy.sum(0)}


def tn_extra(case):
    return sum(term for routes, _, term, _ in EXTRA_ROUNDINGS if case.route in routes and case.rps)


def tn_bound(case, name, ref, S):
    """dw / db are fp32: no store rounding.  A row scale is one more fp32 product (on the operand in fp32, on the accumulator in the DMA-staged kernel)"""
    return bound(ref, S, case.M + int(bool(case.rps)), 0.0, tn_extra(case))


# ------------------------------------------------------------------------------------------------ roundings and statistics
def rne(ref64, dtype):
    """ONE round-to-nearest-even of an fp64 tensor to `dtype`.  torch converts fp64 -> bf16 through fp32: where that fp32 value is a bf16 tie that the
    fp64 value is not, it is moved one fp32 step towards the fp64 value first"""
    torch = _torch()
    f = ref64.float()
    if dtype == torch.float32:
        return f
    d = ref64 - f.double()
    tie = (f.view(torch.int32) & 0xFFFF) == 0x8000
    nudge = torch.nextafter(f, torch.where(d > 0, torch.full_like(f, float("inf")), torch.full_like(f, float("-inf"))))
    return torch.where(tie & (d != 0), nudge, f).to(dtype)


def bits(t):
    torch = _torch()
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32}[t.dtype])


def bit_mismatch(got, want):
    """(elements whose bits differ, of those: -0 against +0).  Only the first minus the second is a failure"""
    torch = _torch()
    ne = bits(got) != bits(want)
    zeros = ne & (got == 0) & (want == 0)
    return int(ne.sum().item()), int(zeros.sum().item())


def ulp(ref64, dtype):
    """the spacing of `dtype` at |ref| (normal range)"""
    torch = _torch()
    p = {torch.bfloat16: 7, torch.float32: 23}[dtype]
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -120)))
    return torch.exp2(e - p)


def rounding_stats(got, ref64):
    """(share of elements that differ from RNE(ref64), mean of sign(ref) (got - ref) / ulp(ref)) of one stored output"""
    torch = _torch()
    want = rne(ref64, got.dtype)
    share = float((got != want).double().mean().item())
    bias = float((torch.sign(ref64) * (got.double() - ref64) / ulp(ref64, got.dtype)).mean().item())
    return share, bias


SHARE_K = 4.0                   # tests/support_value_cases.py: K
SIGMA_ROUNDING = 0.289          # 1 / sqrt(12): the standard deviation, in ulps, of an unbiased rounding error


def share_limit(stock, numel):
    return SHARE_K * stock + 16.0 / numel


def bias_limit(stock, numel):
    return SHARE_K * abs(stock) + 6.0 * SIGMA_ROUNDING / numel ** 0.5


# ------------------------------------------------------------------------------------------------ contractions outside gemm.hip
MLP_CASES = [(40, 96), (296, 96), (168, 192)]                       # fmmt_mlp_fwd (M, C): h_pre
PATCH_CASE = dict(M=3136, C=96, K=48)                               # fmmt_patch_embed_ln_fwd: x_pre, bf16 and fp32
MHA_SHAPES = [(70, 64, 2, 0), (33, 128, 1, 0), (70, 70, 2, 6)]      # (Lq, Lk, B, keys per batch element at -inf)


def mlp_worst(C):
    return 255.0 * 7 * C + BIAS_MAX


def patch_worst():
    return 255.0 * 7 * PATCH_CASE["K"] + BIAS_MAX
