"""Every GEMM kernel family with leading dimensions that are not the row widths (tests/support_gemm_cases.py: one row per route of enum fmmt_route).

Each operand and each output is a view into a larger allocation (tests/support_strided.py): 512 guard rows in front and behind, a row pitch of
width + 8 ("pitch"), the middle third of a packed (rows, 3 * width) buffer ("packed"), for fp32 outputs and M x N operands width + 4 ("pitch4");
NaN with one Inf per row around every input, a fixed bit pattern around every output, NaN in the output's own region, NaN bytes in the workspaces.
The raw C entry points are called directly (ops.*_raw state ld = width).  Asserted per layout, strongest first:
  * bit-identity with the contiguous call of the same operands wherever the route query names the same kernel -- an ld must not change arithmetic;
  * parity with a higher-precision restatement (fp64 below 16384 rows, the fp32 product of the same bf16 operands from there on), at the
    tolerances of the existing GEMM tests;
  * no stray write: padding and guard rows of y, y_pre, dw, db bitwise unchanged;
  * no padding in the result: the valid region finite everywhere.

The two "bigx" rows put the byte offsets of the last third of x's rows between 2^31 and 2^32 (row M - 1 near 3.2e9 bytes, M * ldx still below 2^31
elements: tests/test_gemm_routes_cpu.py holds the table to that) on the two kernels that form per-lane unsigned 32-bit byte offsets.  fmmt_colsum, the
one other GEMM-side entry point with a leading dimension, runs in the same layouts at the end of this file.  Read before the bigx rows were run:
  linear_nt_p256_kernel (gemm.hip, tile_offsets / issue_piece): poff = ((unsigned)(rb + rl) * (unsigned)ldx + (unsigned)(chunk << 3)) * 2u with
    rb + rl <= M - 1 and chunk << 3 <= 56; the address is base + (size_t)(poff + kbyte), kbyte = ik * 128 <= 2 K - 128.  In elements:
    (M - 1) ldx + 56 + (K - 64) + 8 lanes' worth <= (M - 1) ldx + K <= M ldx < 2^31 (p256_plan's guard, ldx >= K), so the product, the sum, the
    doubling (< 2^32) and poff + kbyte (< 2^32) are all unsigned and exact; the cast to size_t zero-extends.
  linear_nt_ph3_kernel (gemm_ph3.h) and linear_nt_ph_kernel (gemm_ph.h): xo = (unsigned)min(m, M - 1) * (unsigned)ldx * 2u + (chunk << 4), chunk << 4
    <= 112, address base + (size_t)(xo + kb), kb = st_k * 128: (M - 1) ldx * 2 + 112 + 16 + (2 K - 128) <= M ldx * 2 < 2^32 by ph_plan's guard; the
    same holds for w (N ldw), and the output side is a buffer resource of (unsigned)M * ldy * 2 bytes with unsigned offsets below it (M ldy < 2^31).
  No signed intermediate in either: the guards M * ld < 2^31 elements are the right ones."""
import math
import zlib

import pytest
import torch

from facialmmt_amd import _lib
from tests import support_gemm_cases as GC
from tests import support_strided as SS

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def _gen(case):
    g = torch.Generator(device="cuda")
    g.manual_seed(zlib.crc32(case.id.encode()))
    return g


def _randn(g, shape, dtype, scale=1.0):
    return (torch.randn(shape, device="cuda", generator=g) * scale).to(dtype)


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * (0.5 ** 0.5)))


def _dgelu(v):
    return 0.5 * (1.0 + torch.erf(v * (0.5 ** 0.5))) + v * torch.exp(-0.5 * v * v) * (1.0 / math.sqrt(2.0 * math.pi))


def _make(case, layout, name, rows, width, dtype, **kw):
    ld, col = GC.lds(case, layout)[name]
    return SS.make(rows, width, dtype, "cuda", ld=ld, col=col, **kw)


def _nan_workspace(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device="cuda")         # fp32 NaN in every word


def _ptr(s):
    return None if s is None else (s.ptr if isinstance(s, SS.Strided) else s.data_ptr())


def _bits(t):
    return t.contiguous().view(SS._INT[t.dtype])


# ------------------------------------------------------------------------------------------------ NT
def _nt_values(case):
    g, dt = _gen(case), DT[case.dt]
    M, N, K = case.M, case.N, case.K
    v = {"x": _randn(g, (M, K), dt), "w": _randn(g, (N, K), dt, K ** -0.5)}
    v["bias"] = _randn(g, (N,), torch.float32, 0.1) if case.bias else None
    v["aux"] = _randn(g, (M, N), dt) if case.aux else None
    v["res"] = _randn(g, (M, N), dt) if case.res else None
    if case.rps:
        rs = torch.rand((M + case.rps - 1) // case.rps, device="cuda", generator=g) + 0.5
        rs[1::5] = 0.0                                             # dropped samples
        v["rs"] = rs
    else:
        v["rs"] = None
    return v


def _nt_reference(case, v):
    """(y, y_pre or None) in fp64 (M <= 8192) or as the fp32 product of the same operands (M >= 16384)"""
    hp = torch.float64 if case.M <= 8192 else torch.float32
    acc = v["x"].to(hp) @ v["w"].to(hp).t()
    if v["bias"] is not None:
        acc += v["bias"].to(hp)
    pre = None
    if case.epi == GC.EPI_GELU:
        pre, y = (acc if case.pre else None), _gelu(acc)
    elif case.epi == GC.EPI_GELU_BWD:
        y = acc * _dgelu(v["aux"].to(hp))
    elif case.epi == GC.EPI_GELU_DG:
        pre, y = (_dgelu(acc) if case.pre else None), _gelu(acc)
    elif case.epi == GC.EPI_MUL_AUX:
        y = acc * v["aux"].to(hp)
    else:
        y = acc
    if v["rs"] is not None:
        y = y * v["rs"].to(hp).repeat_interleave(case.rps)[:case.M, None]
    if v["res"] is not None:
        y = y + v["res"].to(hp)
    return y, pre


def _nt_run(lib, case, layout, v):
    dt, code = DT[case.dt], _lib.dtype_code(DT[case.dt])
    M, N, K = case.M, case.N, case.K
    st = torch.cuda.current_stream().cuda_stream
    x = _make(case, layout, "x", M, K, dt, values=v["x"])
    y = _make(case, layout, "y", M, N, dt, output=True)
    pre = _make(case, layout, "y", M, N, dt, output=True) if case.pre else None
    aux = _make(case, layout, "aux", M, N, dt, values=v["aux"]) if case.aux else None
    res = _make(case, layout, "res", M, N, dt, values=v["res"]) if case.res else None
    ldaux, ldres = (aux.ld if aux else GC.lds(case, layout)["aux"][0]), (res.ld if res else GC.lds(case, layout)["res"][0])
    keep = [x, aux, res]
    if case.mode in ("seg3n", "seg3k"):
        if case.mode == "seg3n":
            parts = [v["w"][i * N // 3:(i + 1) * N // 3] for i in range(3)]
            biases = [v["bias"][i * N // 3:(i + 1) * N // 3].clone() if case.bias else None for i in range(3)]
        else:
            parts = [v["w"][:, i * K // 3:(i + 1) * K // 3] for i in range(3)]
            biases = [None] * 3
        ws = [_make(case, layout, "w", p.shape[0], p.shape[1], dt, values=p) for p in parts]
        keep += ws + biases
        rc = lib.fmmt_linear_fwd_seg3(code, M, N, K, x.ptr, x.ld, ws[0].ptr, ws[1].ptr, ws[2].ptr, ws[0].ld, 1 if case.mode == "seg3n" else 2,
                                      _ptr(biases[0]), _ptr(biases[1]), _ptr(biases[2]), y.ptr, y.ld, st)
    else:
        w = _make(case, layout, "w", N, K, dt, values=v["w"])
        keep.append(w)
        if case.mode == "splitk":
            nbytes = lib.fmmt_linear_splitk_workspace(M, N, K)
            assert nbytes > 0
            wsp = _nan_workspace(nbytes)
            keep.append(wsp)
            rc = lib.fmmt_linear_fwd_splitk(code, M, N, K, x.ptr, x.ld, w.ptr, w.ld, _ptr(v["bias"]), y.ptr, y.ld, wsp.data_ptr(), nbytes, st)
        else:
            rc = lib.fmmt_linear_fwd(code, M, N, K, x.ptr, x.ld, w.ptr, w.ld, _ptr(v["bias"]), y.ptr, y.ld, _ptr(pre), case.epi, _ptr(aux), ldaux,
                                     _ptr(res), ldres, _ptr(v["rs"]), max(case.rps, 1), st)
    torch.cuda.synchronize()
    del keep
    return rc, y, pre


def _nt_check(case, layout, got, ref, with_res):
    """parity of one output with its reference: the figures (printed) and whether they pass"""
    g, r = got.view.to(ref.dtype), ref
    err = (g - r).abs()
    if case.dt == "bf16":
        tol = 0.01 * r.abs() + (1.2e-2 if with_res else 6e-3)      # tests/test_gpu_gemm_ph.py; one more bf16 rounding with a residual
        bad = int((~(err <= tol)).sum().item())
        print(f"  {case.id} [{layout}] max |err| {err.max().item():.3e}, elements over 0.01 |ref| + {1.2e-2 if with_res else 6e-3}: {bad}")
        return bad == 0
    scale = r.abs().max().item()
    print(f"  {case.id} [{layout}] max |err| {err.max().item():.3e} of scale {scale:.3e} (bound 2e-5 of scale)")
    return bool(err.max().item() <= 2e-5 * scale)


@pytest.mark.parametrize("case", GC.NT_CASES, ids=lambda c: c.id)
def test_nt_strided(case):
    lib = _lib.load()
    v = _nt_values(case)
    ref_y, ref_pre = _nt_reference(case, v)
    route0 = GC.query_route(lib, case, "contig")
    assert route0 == GC.route_enum()[case.route]
    rc, y0, pre0 = _nt_run(lib, case, "contig", v)
    assert rc == 0, rc
    assert y0.problems() == [] and (pre0 is None or pre0.problems() == []), ("contig", y0.problems(), pre0 and pre0.problems())
    assert _nt_check(case, "contig", y0, ref_y, case.res)
    assert pre0 is None or _nt_check(case, "contig pre", pre0, ref_pre, False)
    for layout in case.layouts:
        rc, y, pre = _nt_run(lib, case, layout, v)
        assert rc == 0, (layout, rc)
        if GC.query_route(lib, case, layout) == route0:
            assert torch.equal(_bits(y.view), _bits(y0.view)), f"{layout}: the leading dimensions changed the result of the same kernel"
            assert pre is None or torch.equal(_bits(pre.view), _bits(pre0.view)), f"{layout}: y_pre differs from the contiguous call"
        assert _nt_check(case, layout, y, ref_y, case.res), layout
        assert pre is None or _nt_check(case, layout + " pre", pre, ref_pre, False), layout
        assert y.problems() == [], (layout, y.problems())
        assert pre is None or pre.problems() == [], (layout, "y_pre", pre.problems())
        del y, pre


# ------------------------------------------------------------------------------------------------ TN
def _tn_values(case):
    g, dt = _gen(case), DT[case.dt]
    v = {"dy": _randn(g, (case.M, case.N), dt), "x": _randn(g, (case.M, case.K), dt), "rs": None}
    if case.rps:
        n = (case.M + case.rps - 1) // case.rps
        if case.two_valued:                                        # what DropPath hands over: 0 for a dropped image, 1 / keep for the others
            rs = torch.full((n,), 1.0 / 0.9, device="cuda")
            rs[::7] = 0.0
            rs[-1] = 0.0
        else:
            rs = torch.rand(n, device="cuda", generator=g) + 0.5
            rs[1] = 0.0
        v["rs"] = rs
    return v


def _tn_reference(case, v):
    hp = torch.float64 if case.M < 16384 else torch.float32
    sdy = v["dy"].to(hp)
    if v["rs"] is not None:
        sdy = sdy * v["rs"].to(hp).repeat_interleave(case.rps)[:case.M, None]
    xx = v["x"].to(hp)
    if case.x_gelu:
        xx = _gelu(xx)
    return sdy.t() @ xx, sdy.sum(0)


def _tn_tolerance(case):
    """relative to the tensor's scale, from tests/support_op_cases.py (t_wgrad, t_wgrad_large)"""
    if case.dt == "f32":
        return 2e-5
    if case.M < 16384:
        return 2e-2                                                # bf16 against fp64
    return 5e-3 if case.rps and not case.route.endswith("_SCALED") else 1e-3      # against the fp32 product; a general row scale rounds s * dy


def _tn_run(lib, case, layout, v):
    dt, code = DT[case.dt], _lib.dtype_code(DT[case.dt])
    M, N, K = case.M, case.N, case.K
    st = torch.cuda.current_stream().cuda_stream
    dy = _make(case, layout, "dy", M, N, dt, values=v["dy"])
    x = _make(case, layout, "x", M, K, dt, values=v["x"])
    dw = SS.make(N, K, torch.float32, "cuda", output=True)          # the ABI gives dw / db no leading dimension: contiguous, between guards
    db = SS.make(1, N, torch.float32, "cuda", output=True)
    nbytes = lib.fmmt_linear_wgrad_workspace(code, M, N, K)
    wsp = _nan_workspace(nbytes)
    rc = lib.fmmt_linear_wgrad(code, M, N, K, dy.ptr, dy.ld, x.ptr, x.ld, dw.ptr, db.ptr, _ptr(v["rs"]), max(case.rps, 1), GC.EPI_GELU if case.x_gelu else 0,
                               wsp.data_ptr(), nbytes, st)
    torch.cuda.synchronize()
    del dy, x, wsp
    return rc, dw, db


def _tn_check(case, layout, name, got, ref):
    err = (got.to(ref.dtype) - ref).abs().max().item()
    scale, tol = ref.abs().max().item(), _tn_tolerance(case)
    print(f"  {case.id} [{layout}] {name}: max |err| {err:.3e} of scale {scale:.3e} (bound {tol:g} of scale)")
    return err <= tol * scale


@pytest.mark.parametrize("case", GC.TN_CASES, ids=lambda c: c.id)
def test_tn_strided(case):
    lib = _lib.load()
    v = _tn_values(case)
    ref_dw, ref_db = _tn_reference(case, v)
    route0 = GC.query_route(lib, case, "contig")
    assert route0 == GC.route_enum()[case.route]
    rc, dw0, db0 = _tn_run(lib, case, "contig", v)
    assert rc == 0, rc
    assert dw0.problems() == [] and db0.problems() == [], ("contig", dw0.problems(), db0.problems())
    assert _tn_check(case, "contig", "dw", dw0.view, ref_dw) and _tn_check(case, "contig", "db", db0.view[0], ref_db)
    for layout in case.layouts:
        rc, dw, db = _tn_run(lib, case, layout, v)
        assert rc == 0, (layout, rc)
        if GC.query_route(lib, case, layout) == route0:
            assert torch.equal(_bits(dw.view), _bits(dw0.view)), f"{layout}: the leading dimensions changed dw"
            assert torch.equal(_bits(db.view), _bits(db0.view)), f"{layout}: the leading dimensions changed db"
        assert _tn_check(case, layout, "dw", dw.view, ref_dw) and _tn_check(case, layout, "db", db.view[0], ref_db), layout
        assert dw.problems() == [] and db.problems() == [], (layout, dw.problems(), db.problems())
        del dw, db


# ------------------------------------------------------------------------------------------------ fmmt_colsum
@pytest.mark.parametrize("dt,M,N", GC.COLSUM_CASES, ids=lambda v: str(v))
def test_colsum_strided(dt, M, N):
    """out[n] = sum_m x[m * ldx + n] with ldx != N (ops.colsum_raw states ldx = N): bit-identical to the contiguous call, within the tolerances of
    tests/test_gpu_glue.py::test_colsum_and_vendor_linear_bias_gradient of the fp64 sum, nothing written around `out`, no padding in the sum"""
    lib, dtype = _lib.load(), DT[dt]
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(M * 4099 + N)
    xv = _randn(g, (M, N), dtype)
    ref = xv.double().sum(0)
    for od in sorted({dtype, torch.float32}, key=str):
        tol = 2e-2 if od == torch.bfloat16 else 1e-4
        outs = {}
        for layout in ("contig", "pitch", "packed"):
            ld, col = GC.layout_of(layout, N)
            x = SS.make(M, N, dtype, "cuda", ld=ld, col=col, values=xv)
            out = SS.make(1, N, od, "cuda", output=True)
            rc = lib.fmmt_colsum(_lib.dtype_code(dtype), _lib.dtype_code(od), M, N, x.ptr, x.ld, out.ptr, st)
            torch.cuda.synchronize()
            assert rc == 0, (layout, rc)
            err = (out.view[0].double() - ref).abs()
            print(f"  colsum {dt}->{od} {M}x{N} [{layout}] max |err| {err.max().item():.3e} of scale {ref.abs().max().item():.3e}")
            assert bool((err <= tol * ref.abs() + tol * ref.abs().max()).all()), (layout, od)
            assert out.problems() == [], (layout, od, out.problems())
            outs[layout] = _bits(out.view)
        assert torch.equal(outs["pitch"], outs["contig"]) and torch.equal(outs["packed"], outs["contig"]), od
