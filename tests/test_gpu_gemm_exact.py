"""Every GEMM route held to exact integer results and to an a-priori bound (tests/support_exact_cases.py; tests/test_exact_cases_cpu.py holds the
recipe, the reference and the bound to account on the host, and shows that the wrong stand-ins fail).  The raw C entry points on contiguous
operands -- strides are tests/test_gpu_gemm_strided.py's job -- two passes per row of tests/support_gemm_cases.py.

Integer pass.  Operands are small integers whose worst-case sum stays below 2^24: fp32 accumulation is then exact in any order, and every exactly
determined output must be the bits of the fp64 product of the same operands converted ONCE to the output type (dw, db: equal as fp32).  -0 against
+0 is counted and printed, not failed.  The route query must name the route the row is listed under.

Real pass.  The operand distributions of the strided tests.  Every element of every exactly determined output is within the a-priori bound
u_T |ref| + (1 + u_T) gamma(L + e) S (+ the documented roundings of EXTRA_ROUNDINGS); the worst err / bound is printed per row.  For an output
stored in bf16 -- where a store rounding exists -- the share of elements that differ from RNE(ref64) is at most 4 * stock + 16 / numel, and the mean
of sign(ref) (got - ref) / ulp(ref) is within 4 |stock's| + 6 * 0.289 / sqrt(numel): stock is torch's fp32 product of the same operands with the
same fp32 epilogue, rounded once.  (0.289 ulp is the standard deviation of ONE unbiased rounding; a truncating store sits at -0.5.  An fp32 output
has no store rounding, u_T = 0: its error is the summation's, many fp32 ulps wide and not a rounding's, so the two statistics are printed for it
and the bound alone is asserted.)

Contractions outside gemm.hip, integer pass only: the first product of fmmt_mlp_fwd (h_pre), fmmt_patch_embed_ln_fwd (x_pre, bf16 and fp32),
fmmt_colsum, and fmmt_mha_fwd / _bwd with q = 0, integer v and no dropout, where every probability is exactly 2^-6 or 2^-7: `out` is the
once-rounded mean of the live values, dk == 0, and in bf16 dv is the once-rounded sum_q dout / L_live -- mha_mfma.hip rounds P to bf16 in front of
that product (dkv kernel: `pack8(&pp[0], &pp[4])` feeds the dv MFMAs), and 2^-6 (1 + 1e-7) rounds to 2^-6.

Measured on an MI355X (94 tests, 4 s): the 16x16x32 bf16 MFMA accumulation is exact on these operands on every route, as are the fp32 VALU routes.
The integer pass found one defect: the phase kernels' drip epilogue (gemm_ph3.h) rounded acc + bias to bf16 before `res + rowscale * value`
(PH3_OP 18 %, PH3W_OP 25 % of the elements off the single rounding), and the real pass its milder form in PH3_MUL_AUX / PH3W_MUL_AUX (a
2^-17-relative hi + lo pair: 3.6e-4 of the elements off RNE(ref64) against a limit of 2.7e-4); fixed there.  Worst err / bound: 0.99 on the
bf16 routes (the store's half ulp), 0.18 / 0.08 on NT64_F32 / NT128_F32, below 0.03 on the weight gradients; bf16 outputs differ from
RNE(ref64) at 0.1e-4 to 2.2e-4 of their elements, stock at 0 to 2.2e-4."""
import pytest
import torch

from facialmmt_amd import _lib
from tests import support_bounds_cases as BC
from tests import support_exact_cases as EC
from tests import support_gemm_cases as GC

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
DEV = "cuda"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _nan_workspace(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=DEV)


def _assert_bits(what, got, ref64):
    """got is the single rounding of ref64 to its own type, bit for bit; -0 against +0 is reported, not failed"""
    want = EC.rne(ref64, got.dtype)
    assert torch.equal(want.double(), ref64) or got.dtype == torch.bfloat16, f"{what}: the reference itself is not exact in fp32"
    bad, zeros = EC.bit_mismatch(got, want)
    if zeros:
        print(f"  {what}: {zeros} element(s) are -0 against +0 (not a failure)")
    if bad - zeros:
        d = (got.double() - want.double()).abs()
        idx = torch.nonzero((EC.bits(got) != EC.bits(want)) & ~((got == 0) & (want == 0)))[:4].tolist()
        pytest.fail(f"{what}: {bad - zeros} of {got.numel()} elements are not the single rounding of the exact value (max |got - want| {d.max().item():.4g}; first at "
                    f"{idx}: got {[got[tuple(i)].item() for i in idx]}, want {[want[tuple(i)].item() for i in idx]}, exact {[ref64[tuple(i)].item() for i in idx]})")


# ------------------------------------------------------------------------------------------------ NT
def _nt_run(lib, case, v):
    dt, code = DT[case.dt], _lib.dtype_code(DT[case.dt])
    M, N, K = case.M, case.N, case.K
    y = _nan((M, N), dt)
    pre = _nan((M, N), dt) if case.pre else None
    x, w = v["x"].contiguous(), v["w"].contiguous()
    keep = []
    if case.mode in ("seg3n", "seg3k"):
        if case.mode == "seg3n":
            ws = [w[i * N // 3:(i + 1) * N // 3].contiguous() for i in range(3)]
            bs = [v["bias"][i * N // 3:(i + 1) * N // 3].clone() if case.bias else None for i in range(3)]
        else:
            ws = [w[:, i * K // 3:(i + 1) * K // 3].contiguous() for i in range(3)]
            bs = [None] * 3
        keep += ws + bs
        rc = lib.fmmt_linear_fwd_seg3(code, M, N, K, x.data_ptr(), K, ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(), ws[0].shape[1],
                                      1 if case.mode == "seg3n" else 2, _ptr(bs[0]), _ptr(bs[1]), _ptr(bs[2]), y.data_ptr(), N, _st())
    elif case.mode == "splitk":
        nbytes = lib.fmmt_linear_splitk_workspace(M, N, K)
        assert nbytes > 0
        wsp = _nan_workspace(nbytes)
        keep.append(wsp)
        rc = lib.fmmt_linear_fwd_splitk(code, M, N, K, x.data_ptr(), K, w.data_ptr(), K, _ptr(v["bias"]), y.data_ptr(), N, wsp.data_ptr(), nbytes, _st())
    else:
        rc = lib.fmmt_linear_fwd(code, M, N, K, x.data_ptr(), K, w.data_ptr(), K, _ptr(v["bias"]), y.data_ptr(), N, _ptr(pre), case.epi, _ptr(v["aux"]), N,
                                 _ptr(v["res"]), N, _ptr(v["rs"]), max(case.rps, 1), _st())
    torch.cuda.synchronize()
    del keep
    assert rc == 0, rc
    return {"y": y, "y_pre": pre}


def _nt_stock(case, v):
    """torch's own fp32 product of the same operands, the epilogue in fp32 in the documented order, rounded once"""
    acc = v["x"].float() @ v["w"].float().t()
    if v["bias"] is not None:
        acc = acc + v["bias"]
    out = {}
    if case.epi == GC.EPI_GELU:
        out["y_pre"] = acc.to(DT[case.dt])
        return out
    if case.epi == GC.EPI_MUL_AUX:
        acc = acc * v["aux"].float()
    if v["rs"] is not None:
        acc = acc * v["rs"].repeat_interleave(case.rps)[:case.M, None]
    if v["res"] is not None:
        acc = acc + v["res"].float()
    out["y"] = acc.to(DT[case.dt])
    return out


def _judge_real(what, got, ref, bound, stock):
    """the a-priori bound on every element; for a bf16 output the two rounding statistics against stock"""
    ratio = EC.worst_ratio((got.double() - ref).abs(), bound)
    share, bias = EC.rounding_stats(got, ref)
    s_share, s_bias = EC.rounding_stats(stock, ref) if stock is not None else (float("nan"), float("nan"))
    n = got.numel()
    print(f"  {what}: worst err / bound {ratio:.4f}; differs from RNE(ref64) {share:.5f} (stock {s_share:.5f}, limit {EC.share_limit(s_share, n):.5f}); "
          f"mean signed error {bias:+.5f} ulp (stock {s_bias:+.5f}, limit {EC.bias_limit(s_bias, n):.5f})")
    assert torch.isfinite(got).all(), what
    assert ratio <= 1.0, (what, ratio)
    if got.dtype == torch.bfloat16:
        assert share <= EC.share_limit(s_share, n), (what, share, s_share)
        assert abs(bias) <= EC.bias_limit(s_bias, n), (what, bias, s_bias)


@pytest.mark.parametrize("case", [c for c in GC.NT_CASES if EC.nt_exact_outputs(c)], ids=lambda c: c.id)
def test_nt_exact(case):
    lib = _lib.load()
    assert GC.query_route(lib, case, "contig") == GC.route_enum()[case.route]
    # integer pass
    v = EC.nt_int_values(case, DEV)
    ref = EC.nt_reference(case, v)
    assert sorted(ref) == sorted(EC.nt_exact_outputs(case))
    got = _nt_run(lib, case, v)
    for name, r in ref.items():
        _assert_bits(f"{case.id} {name} [integers]", got[name], r)
    del v, ref, got
    # real pass
    v = EC.nt_real_values(case, DEV)
    ref, S, stock = EC.nt_reference(case, v), EC.nt_reference(case, v, absolute=True), _nt_stock(case, v)
    got = _nt_run(lib, case, v)
    for name, r in ref.items():
        _judge_real(f"{case.route} {case.id} {name}", got[name], r, EC.nt_bound(case, name, r, S[name]), stock[name])


# ------------------------------------------------------------------------------------------------ TN
def _tn_run(lib, case, v):
    code = _lib.dtype_code(DT[case.dt])
    M, N, K = case.M, case.N, case.K
    dw, db = _nan((N, K), torch.float32), _nan((N,), torch.float32)
    nbytes = lib.fmmt_linear_wgrad_workspace(code, M, N, K)
    wsp = _nan_workspace(nbytes)
    rc = lib.fmmt_linear_wgrad(code, M, N, K, v["dy"].data_ptr(), N, v["x"].data_ptr(), K, dw.data_ptr(), db.data_ptr(), _ptr(v["rs"]), max(case.rps, 1), 0,
                               wsp.data_ptr(), nbytes, _st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return {"dw": dw, "db": db}


@pytest.mark.parametrize("case", [c for c in GC.TN_CASES if EC.tn_exact_outputs(c)], ids=lambda c: c.id)
def test_tn_exact(case):
    lib = _lib.load()
    assert GC.query_route(lib, case, "contig") == GC.route_enum()[case.route]
    v = EC.tn_int_values(case, DEV)
    ref, got = EC.tn_reference(case, v), _tn_run(lib, case, v)
    for name in ("dw", "db"):
        _assert_bits(f"{case.id} {name} [integers]", got[name], ref[name])
    del v, ref, got
    v = EC.tn_real_values(case, DEV)
    ref, S, got = EC.tn_reference(case, v), EC.tn_reference(case, v, absolute=True), _tn_run(lib, case, v)
    for name in ("dw", "db"):
        _judge_real(f"{case.route} {case.id} {name}", got[name], ref[name], EC.tn_bound(case, name, ref[name], S[name]), None)


# ------------------------------------------------------------------------------------------------ contractions outside gemm.hip
@pytest.mark.parametrize("dt,M,N", GC.COLSUM_CASES, ids=lambda v: str(v))
def test_colsum_exact(dt, M, N):
    lib, dtype = _lib.load(), DT[dt]
    g = torch.Generator(device=DEV)
    g.manual_seed(EC.seed_of(f"colsum {dt} {M} {N}"))
    x = torch.randint(-EC.COLSUM_MAX, EC.COLSUM_MAX + 1, (M, N), generator=g, device=DEV).to(dtype)
    ref = x.double().sum(0)
    for od in sorted({dtype, torch.float32}, key=str):
        out = _nan((N,), od)
        rc = lib.fmmt_colsum(_lib.dtype_code(dtype), _lib.dtype_code(od), M, N, x.data_ptr(), N, out.data_ptr(), _st())
        torch.cuda.synchronize()
        assert rc == 0, rc
        _assert_bits(f"colsum {dt}->{od} {M}x{N}", out, ref)


@pytest.mark.parametrize("M,C", EC.MLP_CASES, ids=lambda v: str(v))
def test_mlp_fwd_first_product_exact(M, C):
    """h_pre = bf16(x . w1^T + b1) of the fused Mlp: an MFMA contraction of its own (mlp_fused.hip)"""
    lib = _lib.load()
    g = torch.Generator(device=DEV)
    g.manual_seed(EC.seed_of(f"mlp {M} {C}"))
    ri = lambda shape, a, dtype: torch.randint(-a, a + 1, shape, generator=g, device=DEV).to(dtype)
    x, w1, b1 = ri((M, C), 255, torch.bfloat16), ri((4 * C, C), 7, torch.bfloat16), ri((4 * C,), EC.BIAS_MAX, torch.float32)
    w2, b2 = torch.zeros((C, 4 * C), dtype=torch.bfloat16, device=DEV), torch.zeros((C,), device=DEV)
    y, hp = _nan((M, C), torch.bfloat16), _nan((M, 4 * C), torch.bfloat16)
    rc = lib.fmmt_mlp_fwd(_lib.BF16, M, C, x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), None, None, 1, y.data_ptr(), hp.data_ptr(), None, _st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    _assert_bits(f"mlp_fwd h_pre {M}x{C}", hp, x.double() @ w1.double().t() + b1.double())
    assert torch.isfinite(y).all()


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_patch_embed_ln_pre_norm_exact(dt):
    """include/fmmt.h: x_pre = bf16(cols . w^T + bias) (fp32: the fp32 value itself)"""
    lib, dtype = _lib.load(), DT[dt]
    M, C, K = EC.PATCH_CASE["M"], EC.PATCH_CASE["C"], EC.PATCH_CASE["K"]
    g = torch.Generator(device=DEV)
    g.manual_seed(EC.seed_of(f"patch {dt}"))
    ri = lambda shape, a, d: torch.randint(-a, a + 1, shape, generator=g, device=DEV).to(d)
    cols, w, bias = ri((M, K), 255, dtype), ri((C, K), 7, dtype), ri((C,), EC.BIAS_MAX, torch.float32)
    ga, be = torch.ones((C,), device=DEV), torch.zeros((C,), device=DEV)
    xp, y, mean, rstd = _nan((M, C), dtype), _nan((M, C), dtype), _nan((M,), torch.float32), _nan((M,), torch.float32)
    rc = lib.fmmt_patch_embed_ln_fwd(_lib.dtype_code(dtype), M, C, K, cols.data_ptr(), w.data_ptr(), bias.data_ptr(), ga.data_ptr(), be.data_ptr(), 1e-5,
                                     xp.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    _assert_bits(f"patch_embed_ln x_pre {dt}", xp, cols.double() @ w.double().t() + bias.double())
    assert torch.isfinite(y).all()


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("E,nh", BC.MHA_GEOM, ids=lambda v: str(v))
@pytest.mark.parametrize("Lq,Lk,B,dead", EC.MHA_SHAPES, ids=lambda v: str(v))
def test_mha_uniform_attention_exact(Lq, Lk, B, dead, E, nh, dt):
    """q = 0: every live key has probability 1 / L_live = 2^-6 or 2^-7 exactly"""
    lib, dtype = _lib.load(), DT[dt]
    code = _lib.dtype_code(dtype)
    g = torch.Generator(device=DEV)
    g.manual_seed(EC.seed_of(f"mha {Lq} {Lk} {B} {E} {dt}"))
    ri = lambda shape, a: torch.randint(-a, a + 1, shape, generator=g, device=DEV).to(dtype)
    q, k, vv, dout = torch.zeros((Lq, B, E), dtype=dtype, device=DEV), ri((Lk, B, E), 7), ri((Lk, B, E), 255), ri((Lq, B, E), 255)
    kb, live = None, torch.ones((B, Lk), dtype=torch.bool, device=DEV)
    if dead:
        for b in range(B):
            live[b, [(11 * j + 5 * b + 3) % Lk for j in range(dead)]] = False      # six distinct scattered keys (11 j mod 70 takes distinct values for j < 6)
        assert int((~live).sum()) == dead * B
        kb = torch.zeros((B, Lk), device=DEV).masked_fill(~live, float("-inf"))
    n_live = Lk - dead
    assert n_live in (64, 128)
    out, lse = _nan((Lq, B, E), dtype), _nan((B * nh * Lq,), torch.float32)
    scale = (E // nh) ** -0.5
    rc = lib.fmmt_mha_fwd(code, Lq, Lk, B, E, nh, q.data_ptr(), E, k.data_ptr(), vv.data_ptr(), E, scale, _ptr(kb), 0.0, 0, None, out.data_ptr(), E, lse.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    mean = (vv.double() * live.t()[:, :, None]).sum(0) / n_live                     # (B, E): the same for every query
    _assert_bits(f"mha_fwd out {dt} E={E}", out, mean[None].expand(Lq, B, E).contiguous())
    dq, dk, dv = _nan((Lq, B, E), dtype), _nan((Lk, B, E), dtype), _nan((Lk, B, E), dtype)
    rc = lib.fmmt_mha_bwd(code, Lq, Lk, B, E, nh, q.data_ptr(), E, k.data_ptr(), vv.data_ptr(), E, scale, _ptr(kb), 0.0, 0, None, out.data_ptr(), dout.data_ptr(), E,
                          lse.data_ptr(), dq.data_ptr(), E, dk.data_ptr(), dv.data_ptr(), E, _st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((dk == 0).all()), "dk = sum_q ds q with q = 0"
    assert torch.isfinite(dq).all()
    if dt == "bf16":
        want = (dout.double().sum(0) / n_live)[None].expand(Lk, B, E) * live.t()[:, :, None]
        _assert_bits(f"mha_bwd dv {dt} E={E}", dv, want.contiguous())
