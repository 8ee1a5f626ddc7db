"""The memory contract of the non-GEMM kernels: multi-head attention, window attention, the fused Swin block half, the fused Mlp, fmmt_linear_ln_bwd,
the LayerNorm kernels, the text-side dropout / LayerNorm tails and the patch embedding (tests/support_bounds_cases.py: one row per call).

Every operand and every output of a row is a view into a larger allocation (tests/support_strided.py, tests/support_bounds.py): 512 guard rows -- 512
elements around a vector -- in front and behind, NaN with Inf around the inputs, a fixed bit pattern around the outputs, NaN in the outputs' own regions,
0xFF (NaN) in every workspace byte and a byte pattern around the workspace.  The attention core, the one entry point here with leading dimensions, gets
five pairwise distinct pitches and k / v (dk / dv) as column slices of one buffer.  The raw C entry point is called twice per row by ONE function: on
ordinary contiguous tensors with a zeroed workspace (the plain call: what ops.*_raw marshal, ld = width) and on the views.  Asserted, strongest first:
  1. bit-identity of every output with the plain call: nothing outside an operand's region, and nothing in the workspace, changes arithmetic;
  2. parity with an fp64 restatement -- on the keep-mask the kernel drew where dropout is on (read back with a probe launch, as
     tests/test_gpu_text_encoder.py does) -- at the tolerances the existing tests of each op hold it to (named at each check);
  3. no stray write: guard rows, pitch padding, the bytes around the workspace bitwise unchanged;
  4. nothing unwritten, no padding in a result: every output region finite (fmmt_mha_*_ragged's lse excepted: entries of padded queries are documented
     as not written);
  5. every input allocation bitwise unchanged;
  6. a workspace one byte short of *_workspace(...) returns FMMT_EWORKSPACE and writes nothing.
A sum over tokens that took in one row behind M (dgamma / dbeta, the column sum, dtable) shows in 1 and 4: 0 x NaN is NaN where 0 x zero-filled allocator
memory was 0."""
import math
import zlib

import pytest
import torch

from facialmmt_amd import _lib, ops
from oracle import swin as OS
from tests import support_bounds as SB
from tests import support_bounds_cases as BC

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
DEV = "cuda"
EWORKSPACE = -3


# ------------------------------------------------------------------------------------------------ helpers
def _gen(c):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(c.id.encode()))
    return g


def _randn(g, shape, dtype=torch.float32, scale=1.0, shift=0.0):
    return (torch.randn(shape, device=DEV, generator=g) * scale + shift).to(dtype)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _code(c):
    return _lib.dtype_code(DT[c.dt])


def _seed(c):
    return zlib.crc32(c.id.encode()) & 0x7FFFFFFF


def _drop_inv(p):
    """the kernels' realised 1 / keep rate: 2^16 / (2^16 - round(p 2^16)) (fmmt_common.h attn_drop_setup / elem_drop_setup)"""
    t = min(int(float(torch.tensor(p, dtype=torch.float32) * 65536.0) + 0.5), 65535)
    return 65536.0 / (65536.0 - t)


def _index():
    return OS.relative_position_index(7).to(DEV).int().contiguous().reshape(-1)


class Findings(list):
    """parity findings of one row; every figure is printed before it is judged"""

    def __init__(self, c):
        super().__init__()
        self.c = c

    def scale(self, name, got, ref, tol, floor=1e-6):
        """max |err| <= tol * max(max |ref|, floor): the rule of tests/support_op_cases.py `report` and tests/test_gpu_wblock.py `_rel`"""
        got, ref = got.double(), ref.double().reshape(got.shape)
        err, sc = (got - ref).abs().max().item(), ref.abs().max().item()
        print(f"  {self.c.id} {name}: max |err| {err:.3e} of scale {sc:.3e} (bound {tol:g} of max(scale, {floor:g}))")
        if not err <= tol * max(sc, floor):
            self.append(f"{name}: max |err| {err:.3e} > {tol:g} * max({sc:.3e}, {floor:g})")

    def l2(self, name, got, ref, rel_tol, abs_frac):
        """relative L2 <= rel_tol and max |err| <= abs_frac * scale: tests/test_gpu_text_encoder.py `_check_close`"""
        got, ref = got.double(), ref.double().reshape(got.shape)
        rel = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
        err, sc = (got - ref).abs().max().item(), ref.abs().max().item() + 1e-6
        print(f"  {self.c.id} {name}: relative L2 {rel:.3e} (bound {rel_tol:g}), max |err| {err:.3e} of scale {sc:.3e} (bound {abs_frac:g})")
        if not (rel <= rel_tol and err <= abs_frac * sc):
            self.append(f"{name}: relative L2 {rel:.3e} / max |err| {err:.3e} of {sc:.3e}")


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * (0.5 ** 0.5)))


def _dgelu(v):
    return 0.5 * (1.0 + torch.erf(v * (0.5 ** 0.5))) + v * torch.exp(-0.5 * v * v) * (1.0 / math.sqrt(2.0 * math.pi))


def _stats(x):
    xf = x.float()
    return xf.mean(1), (xf.var(1, unbiased=False) + 1e-5).rsqrt()


def _ln64(x64, g64, b64):
    return torch.nn.functional.layer_norm(x64, (x64.shape[-1],), g64, b64, 1e-5)


def _rowscale(c, g):
    return SB.rowscale_values(BC.rowscale_len(c), g, DEV) if c.opts.get("rowscale") else None


def _rs64(rs, rps, M):
    return rs.double().repeat_interleave(rps)[:M, None] if rs is not None else 1.0


# ================================================================================================ LayerNorm
def _merge_cat(x, n, hw):
    """PatchMerging's 2x2 concat of a (n * hw * hw, Cq) token grid -> (n * (hw / 2)^2, 4 Cq), channel blocks in fmmt_layernorm_fwd's order (fmmt.h)"""
    Cq = x.shape[-1]
    gq = x.reshape(n, hw // 2, 2, hw // 2, 2, Cq)
    return torch.cat([gq[:, :, 0, :, 0], gq[:, :, 1, :, 0], gq[:, :, 0, :, 1], gq[:, :, 1, :, 1]], -1).reshape(-1, 4 * Cq)


def _ln_values(c):
    g, dt, s = _gen(c), DT[c.dt], c.shape
    M, C, hw = s["M"], s["C"], s["merge_hw"]
    xs = (s["n"] * hw * hw, C // 4) if hw else (M, C)
    v = dict(x=_randn(g, xs, dt, 1.5, 0.3), gamma=_randn(g, (C,), scale=0.2, shift=1.0), beta=_randn(g, (C,), scale=0.1), dy=_randn(g, (M, C), dt))
    v["add"] = _randn(g, xs, dt) if c.opts.get("add") else None
    rows = _merge_cat(v["x"], s["n"], hw) if hw else v["x"]
    v["mean"], v["rstd"] = _stats(rows)
    return v


def _ln_fwd_run(lib, c, v, A):
    s = c.shape
    x, _ = A.mat_in("x", v["x"])
    ga, be = A.vec_in("gamma", v["gamma"]), A.vec_in("beta", v["beta"])
    y, _ = A.mat_out("y", s["M"], s["C"], DT[c.dt])
    mean, rstd = A.vec_out("mean", s["M"]), A.vec_out("rstd", s["M"])
    return A.launch(lib.fmmt_layernorm_fwd, _code(c), s["M"], s["C"], x, ga, be, 1e-5, y, mean, rstd, s["merge_hw"], _st())


def _ln_fwd_parity(c, v, A, F):
    s = c.shape
    rows = _merge_cat(v["x"], s["n"], s["merge_hw"]) if s["merge_hw"] else v["x"]
    r64 = rows.double()
    tol = 1e-5 if c.dt == "f32" else 1.5e-2                         # support_op_cases.t_layernorm
    F.scale("y", A.result("y"), _ln64(r64, v["gamma"].double(), v["beta"].double()), tol)
    F.scale("mean", A.result("mean"), r64.mean(1), 1e-5, 1.0)       # test_gpu_wblock._block_half_case: 1e-5 max(1, |mean|), 1e-4 relative
    F.scale("rstd", A.result("rstd"), (r64.var(1, unbiased=False) + 1e-5).rsqrt(), 1e-4)


def _ln_bwd_run(lib, c, v, A):
    s = c.shape
    M, C = s["M"], s["C"]
    dy, _ = A.mat_in("dy", v["dy"])
    x, _ = A.mat_in("x", v["x"])
    mean, rstd, ga = A.vec_in("mean", v["mean"]), A.vec_in("rstd", v["rstd"]), A.vec_in("gamma", v["gamma"])
    add, _ = A.mat_in("add", v["add"])
    dx, _ = A.mat_out("dx", v["x"].shape[0], v["x"].shape[1], DT[c.dt])
    dg, db = A.vec_out("dgamma", C), A.vec_out("dbeta", C)
    ws, nb = A.workspace(lib.fmmt_layernorm_bwd_workspace(C))
    return A.launch(lib.fmmt_layernorm_bwd, _code(c), M, C, dy, x, mean, rstd, ga, add, dx, dg, db, s["merge_hw"], ws, nb, _st())


def _ln_bwd_parity(c, v, A, F):
    s = c.shape
    x64 = v["x"].double().requires_grad_(True)
    g64 = v["gamma"].double().requires_grad_(True)
    b64 = torch.zeros_like(g64).requires_grad_(True)
    rows = _merge_cat(x64, s["n"], s["merge_hw"]) if s["merge_hw"] else x64
    gx, gg, gb = torch.autograd.grad(_ln64(rows, g64, b64), [x64, g64, b64], v["dy"].double())
    if v["add"] is not None:
        gx = gx + v["add"].double()
    tol = 2 * (1e-5 if c.dt == "f32" else 1.5e-2)                   # support_op_cases.t_layernorm: backward at twice the forward's
    F.scale("dx", A.result("dx"), gx, tol)
    F.scale("dgamma", A.result("dgamma"), gg, tol)
    F.scale("dbeta", A.result("dbeta"), gb, tol)


# ================================================================================================ fused Mlp
def _mlp_values(c):
    g, dt, s = _gen(c), DT[c.dt], c.shape
    M, C = s["M"], s["C"]
    v = dict(x=_randn(g, (M, C), dt, 1.5, 0.3), w1=_randn(g, (4 * C, C), dt, C ** -0.5), b1=_randn(g, (4 * C,), scale=0.1),
             w2=_randn(g, (C, 4 * C), dt, (4 * C) ** -0.5), b2=_randn(g, (C,), scale=0.1), gamma=_randn(g, (C,), scale=0.2, shift=1.0),
             beta=_randn(g, (C,), scale=0.1), dy=_randn(g, (M, C), dt), h_pre=_randn(g, (M, 4 * C), dt))
    v["res"] = _randn(g, (M, C), dt) if c.opts.get("res") else None
    v["rs"] = _rowscale(c, g)
    v["w1t"], v["w2t"] = v["w1"].t().contiguous(), v["w2"].t().contiguous()
    v["mean"], v["rstd"] = _stats(v["x"])
    return v


def _mlp_code(c):
    return _code(c) | (_lib.SAVE_DG if c.opts["dg"] else 0)


def _mlp_weights(A, v, names):
    return [A.mat_in(n, v[n])[0] if v[n].dim() == 2 else A.vec_in(n, v[n]) for n in names]


def _mlp_fwd_run(lib, c, v, A):
    s, o, dt = c.shape, c.opts, DT[c.dt]
    M, C = s["M"], s["C"]
    x, _ = A.mat_in("x", v["x"])
    w1, b1, w2, b2 = _mlp_weights(A, v, ("w1", "b1", "w2", "b2"))
    rs = A.vec_in("rowscale", v["rs"])
    y, _ = A.mat_out("y", M, C, dt)
    hp, _ = A.mat_out("h_pre", M, 4 * C, dt, present=o["h_pre"])
    ha, _ = A.mat_out("h_act", M, 4 * C, dt, present=o["h_act"])
    if c.entry == "fmmt_mlp_fwd":
        res, _ = A.mat_in("res", v["res"])
        return A.launch(lib.fmmt_mlp_fwd, _mlp_code(c), M, C, x, w1, b1, w2, b2, res, rs, s["rows_per_scale"], y, hp, ha, _st())
    ga, be = A.vec_in("gamma", v["gamma"]), A.vec_in("beta", v["beta"])
    xn, _ = A.mat_out("xn", M, C, dt, present=o["xn"])
    mean, rstd = A.vec_out("mean", M, present=o["stats"]), A.vec_out("rstd", M, present=o["stats"])
    return A.launch(lib.fmmt_mlp_ln_fwd, _mlp_code(c), M, C, x, ga, be, 1e-5, w1, b1, w2, b2, rs, s["rows_per_scale"], y, xn, mean, rstd, hp, ha, _st())


def _mlp_fwd_parity(c, v, A, F):
    s, o = c.shape, c.opts
    M = s["M"]
    x64 = v["x"].double()
    ln = c.entry == "fmmt_mlp_ln_fwd"
    xin = _ln64(x64, v["gamma"].double(), v["beta"].double()) if ln else x64
    pre = xin @ v["w1"].double().t() + v["b1"].double()
    body = _gelu(pre) @ v["w2"].double().t() + v["b2"].double()
    res = x64 if ln else (v["res"].double() if v["res"] is not None else 0.0)
    y = res + _rs64(v["rs"], s["rows_per_scale"], M) * body
    bf = c.dt == "bf16"
    # bf16: 2e-2 of scale (support_op_cases.t_mlp_fused, test_gpu_wblock._mlp_half_case); fp32: 1e-4 max(1, scale)
    # (test_gpu_wblock.test_fp32_instantiation_of_the_fused_mlp_against_fp64)
    tol, floor = (2e-2, 1e-6) if bf else (1e-4, 1.0)
    F.scale("y", A.result("y"), y, tol, floor)
    if o["h_pre"]:
        F.scale("h_pre", A.result("h_pre"), _dgelu(pre) if o["dg"] else pre, tol, floor)
    if o["h_act"]:
        F.scale("h_act", A.result("h_act"), _gelu(pre), tol, floor)
    if ln and o["xn"]:
        F.scale("xn", A.result("xn"), xin, 1.5e-2 if bf else 1e-5)  # support_op_cases.t_layernorm
    if ln and o["stats"]:
        F.scale("mean", A.result("mean"), x64.mean(1), 1e-5, 1.0)
        F.scale("rstd", A.result("rstd"), (x64.var(1, unbiased=False) + 1e-5).rsqrt(), 1e-4)


def _mlp_bwd_run(lib, c, v, A):
    s, dt = c.shape, DT[c.dt]
    M, C = s["M"], s["C"]
    dy, _ = A.mat_in("dy", v["dy"])
    hp, _ = A.mat_in("h_pre", v["h_pre"])
    w2t, w1t = _mlp_weights(A, v, ("w2t", "w1t"))
    rs = A.vec_in("rowscale", v["rs"])
    if c.entry == "fmmt_mlp_bwd_input":
        dh, _ = A.mat_out("dh", M, 4 * C, dt)
        dx, _ = A.mat_out("dx", M, C, dt)
        return A.launch(lib.fmmt_mlp_bwd_input, _mlp_code(c), M, C, dy, hp, w2t, w1t, rs, s["rows_per_scale"], dh, dx, _st())
    x, _ = A.mat_in("x", v["x"])
    mean, rstd, ga = A.vec_in("mean", v["mean"]), A.vec_in("rstd", v["rstd"]), A.vec_in("gamma", v["gamma"])
    dh, _ = A.mat_out("dh", M, 4 * C, dt)
    dx, _ = A.mat_out("dx", M, C, dt)
    dg, db = A.vec_out("dgamma", C), A.vec_out("dbeta", C)
    ws, nb = A.workspace(lib.fmmt_mlp_ln_bwd_input_workspace(C))
    return A.launch(lib.fmmt_mlp_ln_bwd_input, _mlp_code(c), M, C, dy, hp, w2t, w1t, rs, s["rows_per_scale"], x, mean, rstd, ga, dh, dx, dg, db, ws, nb, _st())


def _mlp_bwd_parity(c, v, A, F):
    s = c.shape
    M = s["M"]
    hp = v["h_pre"].double()
    dh = _rs64(v["rs"], s["rows_per_scale"], M) * (v["dy"].double() @ v["w2t"].double().t()) * (hp if c.opts["dg"] else _dgelu(hp))
    dxn = dh @ v["w1t"].double().t()
    bf = c.dt == "bf16"
    # bf16: dh at the GELU' epilogue's 2e-2 (support_op_cases.t_linear), gradients at 4e-2 (test_gpu_wblock._mlp_half_case); fp32: 1e-3
    # (test_gpu_wblock.test_fp32_instantiation_of_the_fused_mlp_against_fp64)
    F.scale("dh", A.result("dh"), dh, 2e-2 if bf else 1e-3)
    gtol = 4e-2 if bf else 1e-3
    if c.entry == "fmmt_mlp_bwd_input":
        F.scale("dx", A.result("dx"), dxn, gtol)
        return
    x64 = v["x"].double().requires_grad_(True)
    g64 = v["gamma"].double().requires_grad_(True)
    b64 = torch.zeros_like(g64).requires_grad_(True)
    gx, gg, gb = torch.autograd.grad(_ln64(x64, g64, b64), [x64, g64, b64], dxn)
    F.scale("dx", A.result("dx"), gx + v["dy"].double(), gtol)
    F.scale("dgamma", A.result("dgamma"), gg, gtol)
    F.scale("dbeta", A.result("dbeta"), gb, gtol)


# ================================================================================================ Linear + LayerNorm backward
def _lin_values(c):
    g, dt, s = _gen(c), DT[c.dt], c.shape
    M, C, K = s["M"], s["C"], s["K"]
    v = dict(x=_randn(g, (M, C), dt, 1.5, 0.3), dz=_randn(g, (M, K), dt), wt=_randn(g, (C, K), dt, C ** -0.5), gamma=_randn(g, (C,), scale=0.2, shift=1.0))
    v["dres"] = _randn(g, (M, C), dt) if c.opts["dres"] else None
    v["mean"], v["rstd"] = _stats(v["x"])
    return v


def _lin_run(lib, c, v, A):
    s = c.shape
    M, C, K = s["M"], s["C"], s["K"]
    dz, _ = A.mat_in("dz", v["dz"])
    wt, _ = A.mat_in("wt", v["wt"])
    x, _ = A.mat_in("x", v["x"])
    mean, rstd, ga = A.vec_in("mean", v["mean"]), A.vec_in("rstd", v["rstd"]), A.vec_in("gamma", v["gamma"])
    dres, _ = A.mat_in("dres", v["dres"])
    dx, _ = A.mat_out("dx", M, C, DT[c.dt])
    dg, db = A.vec_out("dgamma", C), A.vec_out("dbeta", C)
    ws, nb = A.workspace(lib.fmmt_linear_ln_bwd_workspace(C))
    return A.launch(lib.fmmt_linear_ln_bwd, _code(c), M, C, K, dz, wt, x, mean, rstd, ga, dres, dx, dg, db, ws, nb, _st())


def _lin_parity(c, v, A, F):
    x64 = v["x"].double().requires_grad_(True)
    g64 = v["gamma"].double().requires_grad_(True)
    b64 = torch.zeros_like(g64).requires_grad_(True)
    dxn = v["dz"].double() @ v["wt"].double().t()                   # wt = w^T [C, K]: d(LN out) = dz . w
    gx, gg, gb = torch.autograd.grad(_ln64(x64, g64, b64), [x64, g64, b64], dxn)
    if v["dres"] is not None:
        gx = gx + v["dres"].double()
    tol = 2e-2 if c.dt == "bf16" else 1e-4                          # test_gpu_wblock.test_linear_and_layernorm_backward_* (bf16 / fp32 instantiation)
    F.scale("dx", A.result("dx"), gx, tol)
    F.scale("dgamma", A.result("dgamma"), gg, tol)
    F.scale("dbeta", A.result("dbeta"), gb, tol)


# ================================================================================================ patch embedding
def _patch_values(c):
    g, dt, s = _gen(c), DT[c.dt], c.shape
    return dict(cols=_randn(g, (s["M"], s["K"]), dt), w=_randn(g, (s["C"], s["K"]), dt, s["K"] ** -0.5), bias=_randn(g, (s["C"],), scale=0.1),
                gamma=_randn(g, (s["C"],), scale=0.2, shift=1.0), beta=_randn(g, (s["C"],), scale=0.1))


def _patch_run(lib, c, v, A):
    s, dt = c.shape, DT[c.dt]
    cols, _ = A.mat_in("cols", v["cols"])
    w, _ = A.mat_in("w", v["w"])
    bias, ga, be = A.vec_in("bias", v["bias"]), A.vec_in("gamma", v["gamma"]), A.vec_in("beta", v["beta"])
    xp, _ = A.mat_out("x_pre", s["M"], s["C"], dt)
    y, _ = A.mat_out("y", s["M"], s["C"], dt)
    mean, rstd = A.vec_out("mean", s["M"]), A.vec_out("rstd", s["M"])
    return A.launch(lib.fmmt_patch_embed_ln_fwd, _code(c), s["M"], s["C"], s["K"], cols, w, bias, ga, be, 1e-5, xp, y, mean, rstd, _st())


def _patch_parity(c, v, A, F):
    pre = v["cols"].double() @ v["w"].double().t() + v["bias"].double()
    bf = c.dt == "bf16"
    # test_gpu_wblock.test_patch_embed_projection_and_layernorm_in_one_launch (bf16: 2e-2) / test_fp32_patch_embed_* (1e-5)
    F.scale("x_pre", A.result("x_pre"), pre, 2e-2 if bf else 1e-5)
    F.scale("y", A.result("y"), _ln64(pre, v["gamma"].double(), v["beta"].double()), 2e-2 if bf else 1e-5)
    seen = A.result("x_pre").double()                                # the statistics are those of x_pre as stored (fmmt.h): judged on the stored values
    F.scale("mean", A.result("mean"), seen.mean(1), 1e-5, 1.0)
    F.scale("rstd", A.result("rstd"), (seen.var(1, unbiased=False) + 1e-5).rsqrt(), 1e-4)


# ================================================================================================ text / fusion tails
def _tail_values(c):
    g, s = _gen(c), c.shape
    bf = torch.bfloat16
    if c.entry == "fmmt_plm_gelu_bwd_colsum":
        return dict(pre=_randn(g, (s["M"], s["H"]), bf, 3.0), dact=_randn(g, (s["M"], s["H"]), bf))
    M, C = s["M"], s["C"]
    pd = DT[s.get("param_dt", "bf16")]
    v = dict(h=_randn(g, (M, C), bf), res=_randn(g, (M, C), bf), x=_randn(g, (M, C), bf, 2.0, 0.5), dy=_randn(g, (M, C), bf),
             gamma=_randn(g, (C,), pd, 0.2, 1.0), beta=_randn(g, (C,), pd, 0.1), salt=3 << 40, seed=_seed(c), pd=pd)
    if "dropadd" in c.entry:
        v["keep"] = _tail_keep(c, v)
        t = (v["h"].float() * v["keep"] * _drop_inv(s["p"])).to(bf)
        v["xsum"] = (t.float() + v["res"].float()).to(bf)           # what the forward saves (fmmt.h); the backward rows take it as their input
    return v


def _tail_fwd_call(lib, c, args):
    if c.entry.startswith("fmmt_plm_"):
        return lib.fmmt_plm_dropadd_ln_fwd(*args)
    return lib.fmmt_dropadd_ln_fwd(_lib.dtype_code(DT[c.shape["param_dt"]]), *args)


def _tail_keep(c, v):
    """the keep-mask of (M, C, seed, salt): h = 1, res = 0 leaves keep / (1 - p) in xsum (tests/test_gpu_text_encoder.py's probe)"""
    s = c.shape
    M, C = s["M"], s["C"]
    ones, zeros = torch.ones(M, C, device=DEV, dtype=torch.bfloat16), torch.zeros(M, C, device=DEV, dtype=torch.bfloat16)
    probe, junk = torch.empty_like(ones), torch.empty_like(ones)
    rc = _lib.load().fmmt_plm_dropadd_ln_fwd(M, C, 1e-5, ones.data_ptr(), zeros.data_ptr(), v["gamma"].to(torch.bfloat16).data_ptr(),
                                             v["beta"].to(torch.bfloat16).data_ptr(), s["p"], v["seed"], None, v["salt"], probe.data_ptr(), junk.data_ptr(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    keep = (probe != 0).float()
    if s["p"] == 0.0:
        assert bool(keep.all())
    return keep


def _tail_fwd_run(lib, c, v, A):
    s = c.shape
    M, C = s["M"], s["C"]
    h, _ = A.mat_in("h", v["h"])
    res, _ = A.mat_in("res", v["res"])
    ga, be = A.vec_in("gamma", v["gamma"]), A.vec_in("beta", v["beta"])
    xs, _ = A.mat_out("xsum", M, C, torch.bfloat16)
    y, _ = A.mat_out("y", M, C, torch.bfloat16)
    args = (M, C, 1e-5, h, res, ga, be, s["p"], v["seed"], None, v["salt"], xs, y, _st())
    return A.launch(lambda: _tail_fwd_call(lib, c, args))


def _tail_fwd_parity(c, v, A, F):
    xs = v["h"].double() * v["keep"].double() * _drop_inv(c.shape["p"]) + v["res"].double()
    # tests/test_gpu_text_encoder.py::test_ffn_node_with_dropout_at_the_benchmark_shape: forward 1e-2 relative L2, 3e-2 of scale
    F.l2("xsum", A.result("xsum"), xs, 1e-2, 3e-2)
    F.l2("y", A.result("y"), _ln64(xs, v["gamma"].double(), v["beta"].double()), 1e-2, 3e-2)


def _tail_bwd_run(lib, c, v, A):
    s = c.shape
    M, C = s["M"], s["C"]
    pd = v["pd"]
    dy, _ = A.mat_in("dy", v["dy"])
    ga = A.vec_in("gamma", v["gamma"])
    if c.entry == "fmmt_layernorm_bwd_bf16":
        x, _ = A.mat_in("x", v["x"])
        dx, _ = A.mat_out("dx", M, C, torch.bfloat16)
        dg, db = A.vec_out("dgamma", C, torch.bfloat16), A.vec_out("dbeta", C, torch.bfloat16)
        ws, nb = A.workspace(lib.fmmt_layernorm_bwd_bf16_workspace(M, C))
        return A.launch(lib.fmmt_layernorm_bwd_bf16, M, C, 1e-5, dy, x, ga, dx, dg, db, ws, nb, _st())
    xs, _ = A.mat_in("xsum", v["xsum"])
    dx, _ = A.mat_out("dx", M, C, torch.bfloat16)
    dh, _ = A.mat_out("dh", M, C, torch.bfloat16)
    dg, db = A.vec_out("dgamma", C, pd), A.vec_out("dbeta", C, pd)
    dbias = A.vec_out("dbias", C, pd, present=c.opts["dbias"])
    if c.entry.startswith("fmmt_plm_"):
        ws, nb = A.workspace(lib.fmmt_plm_dropadd_ln_bwd_workspace(M, C))
        return A.launch(lib.fmmt_plm_dropadd_ln_bwd, M, C, 1e-5, dy, xs, ga, s["p"], v["seed"], None, v["salt"], dx, dh, dg, db, dbias, ws, nb, _st())
    ws, nb = A.workspace(lib.fmmt_dropadd_ln_bwd_workspace(M, C))
    return A.launch(lib.fmmt_dropadd_ln_bwd, _lib.dtype_code(pd), M, C, 1e-5, dy, xs, ga, s["p"], v["seed"], None, v["salt"], dx, dh, dg, db, dbias, ws, nb, _st())


def _tail_bwd_parity(c, v, A, F):
    x64 = (v["x"] if c.entry == "fmmt_layernorm_bwd_bf16" else v["xsum"]).double().requires_grad_(True)
    g64 = v["gamma"].double().requires_grad_(True)
    b64 = torch.zeros_like(g64).requires_grad_(True)
    gx, gg, gb = torch.autograd.grad(_ln64(x64, g64, b64), [x64, g64, b64], v["dy"].double())
    if c.entry == "fmmt_layernorm_bwd_bf16":
        for name, ref in (("dx", gx), ("dgamma", gg), ("dbeta", gb)):   # tests/test_gpu_glue.py::test_bf16_layernorm_backward_for_the_text_encoder
            F.scale(name, A.result(name), ref, 1.5e-2)
        return
    dh = gx * v["keep"].double() * _drop_inv(c.shape["p"])
    # tests/test_gpu_text_encoder.py::test_ffn_node_with_dropout_at_the_benchmark_shape: gradients 2e-2 relative L2, 4e-2 of scale
    for name, ref in (("dx", gx), ("dh", dh), ("dgamma", gg), ("dbeta", gb)):
        F.l2(name, A.result(name), ref, 2e-2, 4e-2)
    if c.opts["dbias"]:
        F.l2("dbias", A.result("dbias"), A.result("dh").double().sum(0), 2e-2, 4e-2)     # the column sum of dh as stored (fmmt.h)


def _colsum_run(lib, c, v, A):
    M, H = c.shape["M"], c.shape["H"]
    dact, _ = A.mat_in("dact", v["dact"])
    pre, _ = A.mat_in("pre", v["pre"])
    dpre, _ = A.mat_out("dpre", M, H, torch.bfloat16)
    dbias = A.vec_out("dbias", H, torch.bfloat16)
    ws, nb = A.workspace(lib.fmmt_plm_gelu_bwd_colsum_workspace(M, H))
    return A.launch(lib.fmmt_plm_gelu_bwd_colsum, M, H, dact, pre, dpre, dbias, ws, nb, _st())


def _colsum_parity(c, v, A, F):
    """tests/test_gpu_glue.py::test_gelu_backward_with_the_bias_gradient_in_one_pass: one bf16 step of the result + 2e-4 |dact| + 1e-6 per element;
    dbias against the column sum of the stored dpre at 8e-3 of scale + 1e-3"""
    g = v["dact"].double() * _dgelu(v["pre"].double())
    err = (A.result("dpre").double() - g).abs()
    tol = 8.5e-3 * g.abs() + 2e-4 * v["dact"].double().abs() + 1e-6
    worst = (err / tol).max().item()
    print(f"  {c.id} dpre: worst |err| / bound {worst:.3f}")
    if not worst <= 1.0:
        F.append(f"dpre: |err| reaches {worst:.3f} of its bound")
    ref = A.result("dpre").double().sum(0)
    e = (A.result("dbias").double() - ref).abs().max().item()
    print(f"  {c.id} dbias: max |err| {e:.3e} of scale {ref.abs().max().item():.3e} (bound 8e-3 of scale + 1e-3)")
    if not e <= 8e-3 * ref.abs().max().item() + 1e-3:
        F.append(f"dbias: max |err| {e:.3e}")


# ================================================================================================ window attention
def _wattn_ref(*a):
    from tests.support_op_cases import _wattn_ref as f
    return f(*a)


def _wattn_mask(s):
    return OS.shift_mask(s["H"], s["H"], 7, s["shift"]).to(DEV).float().contiguous() if s["shift"] else None


def _wattn_values(c):
    g, dt, s = _gen(c), DT[c.dt], c.shape
    T = s["n_img"] * s["H"] * s["H"]
    v = dict(qkv=_randn(g, (T, 3 * s["C"]), dt), table=_randn(g, (169 * s["heads"],), scale=0.5), dout=_randn(g, (T, s["C"]), dt), index=_index())
    v["mask"] = _wattn_mask(s) if c.opts["mask"] else None
    if c.entry == "fmmt_window_attn_bwd":                            # what the forward left behind, from the plain wrapper
        v["out"], v["lse"] = ops.window_attn_fwd_raw(v["qkv"], v["table"], v["index"], v["mask"], s["n_img"], s["H"], s["H"], s["heads"], s["shift"], 32 ** -0.5,
                                                     c.opts["mask_is_shift"])
    return v


def _wattn_common(c, v, A):
    qkv, _ = A.mat_in("qkv", v["qkv"])
    table, index = A.vec_in("table", v["table"]), A.vec_in("index", v["index"])
    mask = A.vec_in("mask", v["mask"].reshape(-1) if v["mask"] is not None else None)
    nWm = v["mask"].shape[0] if v["mask"] is not None else 0
    return qkv, table, index, mask, nWm


def _wattn_fwd_run(lib, c, v, A):
    s = c.shape
    T, nW = s["n_img"] * s["H"] ** 2, s["n_img"] * (s["H"] // 7) ** 2
    qkv, table, index, mask, nWm = _wattn_common(c, v, A)
    out, _ = A.mat_out("out", T, s["C"], DT[c.dt])
    lse = A.vec_out("lse", nW * s["heads"] * 49)
    return A.launch(lib.fmmt_window_attn_fwd, _code(c), s["n_img"], s["H"], s["H"], s["C"], s["heads"], s["shift"], qkv, table, index, mask, nWm,
                    int(c.opts["mask_is_shift"]), 32 ** -0.5, out, lse, _st())


def _wattn_fwd_parity(c, v, A, F):
    s = c.shape
    m = v["mask"].double() if v["mask"] is not None else None
    ref = _wattn_ref(v["qkv"].double(), v["table"].double().reshape(169, -1), m, s["n_img"], s["H"], s["C"], s["heads"], s["shift"])
    F.scale("out", A.result("out"), ref, 2e-5 if c.dt == "f32" else 2e-2)      # support_op_cases.t_wattn


def _wattn_bwd_run(lib, c, v, A):
    s = c.shape
    T = s["n_img"] * s["H"] ** 2
    qkv, table, index, mask, nWm = _wattn_common(c, v, A)
    out, _ = A.mat_in("out", v["out"])
    dout, _ = A.mat_in("dout", v["dout"])
    lse = A.vec_in("lse", v["lse"])
    dqkv, _ = A.mat_out("dqkv", T, 3 * s["C"], DT[c.dt])
    dtable = A.vec_out("dtable", 169 * s["heads"])
    ws, nb = A.workspace(lib.fmmt_window_attn_bwd_workspace(s["heads"]))
    return A.launch(lib.fmmt_window_attn_bwd, _code(c), s["n_img"], s["H"], s["H"], s["C"], s["heads"], s["shift"], qkv, out, dout, lse, table, index, mask, nWm,
                    int(c.opts["mask_is_shift"]), 32 ** -0.5, dqkv, dtable, ws, nb, _st())


def _wattn_bwd_parity(c, v, A, F):
    s = c.shape
    q64 = v["qkv"].double().requires_grad_(True)
    t64 = v["table"].double().reshape(169, -1).requires_grad_(True)
    m = v["mask"].double() if v["mask"] is not None else None
    ref = _wattn_ref(q64, t64, m, s["n_img"], s["H"], s["C"], s["heads"], s["shift"])
    gq, gt = torch.autograd.grad(ref, [q64, t64], v["dout"].double())
    tol = 2 * (2e-5 if c.dt == "f32" else 2e-2)                     # support_op_cases.t_wattn
    F.scale("dqkv", A.result("dqkv"), gq, tol)
    F.scale("dtable", A.result("dtable"), gt.reshape(-1), tol)


# ================================================================================================ fused block half
def _wblock_values(c):
    g, dt, s = _gen(c), DT[c.dt], c.shape
    C, nh = s["C"], s["heads"]
    T = s["n_img"] * s["H"] ** 2
    v = dict(x=_randn(g, (T, C), dt, 1.5, 0.3), gamma=_randn(g, (C,), scale=0.2, shift=1.0), beta=_randn(g, (C,), scale=0.1), wqkv=_randn(g, (3 * C, C), dt, C ** -0.5),
             bqkv=_randn(g, (3 * C,), scale=0.1), wproj=_randn(g, (C, C), dt, C ** -0.5), bproj=_randn(g, (C,), scale=0.1), table=_randn(g, (169 * nh,), scale=0.5),
             dy=_randn(g, (T, C), dt), index=_index(), rs=_rowscale(c, g), mask=_wattn_mask(s))
    if c.entry == "fmmt_window_block_attn_bwd":                      # LN(x), the attention output and the log-sum-exp, from the plain wrapper
        _, v["xn"], v["o"], _, _, v["lse"] = ops.window_block_raw(v["x"], s["n_img"], s["H"], s["H"], nh, s["shift"], v["gamma"], v["beta"], 1e-5, v["wqkv"], v["bqkv"],
                                                                  v["wproj"], v["bproj"], v["table"], v["index"], 32 ** -0.5, v["rs"], True, v["mask"])
    return v


def _wblock_fwd_run(lib, c, v, A):
    s, o, dt = c.shape, c.opts, DT[c.dt]
    T, nW = s["n_img"] * s["H"] ** 2, s["n_img"] * (s["H"] // 7) ** 2
    x, _ = A.mat_in("x", v["x"])
    ga, be = A.vec_in("gamma", v["gamma"]), A.vec_in("beta", v["beta"])
    wq, _ = A.mat_in("wqkv", v["wqkv"])
    bq = A.vec_in("bqkv", v["bqkv"])
    wp, _ = A.mat_in("wproj", v["wproj"])
    bp, table, index, rs = A.vec_in("bproj", v["bproj"]), A.vec_in("table", v["table"]), A.vec_in("index", v["index"]), A.vec_in("rowscale", v["rs"])
    y, _ = A.mat_out("y", T, s["C"], dt)
    xn, _ = A.mat_out("xn", T, s["C"], dt, present=o["xn"])
    ao, _ = A.mat_out("attn_out", T, s["C"], dt, present=o["attn_out"])
    mean, rstd = A.vec_out("mean", T, present=o["stats"]), A.vec_out("rstd", T, present=o["stats"])
    lse = A.vec_out("lse", nW * s["heads"] * 49)
    return A.launch(lib.fmmt_window_block_fwd, _code(c), s["n_img"], s["H"], s["H"], s["C"], s["heads"], s["shift"], x, ga, be, 1e-5, wq, bq, wp, bp, table, index,
                    32 ** -0.5, rs, y, xn, ao, mean, rstd, lse, _st())


def _wblock_fwd_parity(c, v, A, F):
    s, o = c.shape, c.opts
    C = s["C"]
    x64 = v["x"].double()
    xn = _ln64(x64, v["gamma"].double(), v["beta"].double())
    qkv = xn @ v["wqkv"].double().t() + v["bqkv"].double()
    m = v["mask"].double() if v["mask"] is not None else None
    att = _wattn_ref(qkv, v["table"].double().reshape(169, -1), m, s["n_img"], s["H"], C, s["heads"], s["shift"])
    y = x64 + _rs64(v["rs"], s["H"] ** 2, x64.shape[0]) * (att @ v["wproj"].double().t() + v["bproj"].double())
    F.scale("y", A.result("y"), y, 2e-2)                             # test_gpu_wblock._block_half_case
    if o["xn"]:
        F.scale("xn", A.result("xn"), xn, 1.5e-2)                    # support_op_cases.t_layernorm
    if o["attn_out"]:
        F.scale("attn_out", A.result("attn_out"), att, 2e-2)         # support_op_cases.t_wattn
    if o["stats"]:
        F.scale("mean", A.result("mean"), x64.mean(1), 1e-5, 1.0)    # test_gpu_wblock._block_half_case
        F.scale("rstd", A.result("rstd"), (x64.var(1, unbiased=False) + 1e-5).rsqrt(), 1e-4)


def _wblock_bwd_run(lib, c, v, A):
    s = c.shape
    T = s["n_img"] * s["H"] ** 2
    xn, _ = A.mat_in("xn", v["xn"])
    dy, _ = A.mat_in("dy", v["dy"])
    ao, _ = A.mat_in("attn_out", v["o"])
    lse = A.vec_in("lse", v["lse"])
    wq, _ = A.mat_in("wqkv", v["wqkv"])
    bq = A.vec_in("bqkv", v["bqkv"])
    wp, _ = A.mat_in("wproj", v["wproj"])
    table, index, rs = A.vec_in("table", v["table"]), A.vec_in("index", v["index"]), A.vec_in("rowscale", v["rs"])
    dqkv, _ = A.mat_out("dqkv", T, 3 * s["C"], DT[c.dt])
    dtable = A.vec_out("dtable", 169 * s["heads"])
    ws, nb = A.workspace(lib.fmmt_window_attn_bwd_workspace(s["heads"]))
    return A.launch(lib.fmmt_window_block_attn_bwd, _code(c), s["n_img"], s["H"], s["H"], s["C"], s["heads"], s["shift"], xn, dy, ao, lse, wq, bq, wp, table, index,
                    32 ** -0.5, rs, dqkv, dtable, ws, nb, _st())


def _wblock_bwd_parity(c, v, A, F):
    s = c.shape
    q64 = (v["xn"].double() @ v["wqkv"].double().t() + v["bqkv"].double()).requires_grad_(True)
    t64 = v["table"].double().reshape(169, -1).requires_grad_(True)
    m = v["mask"].double() if v["mask"] is not None else None
    att = _wattn_ref(q64, t64, m, s["n_img"], s["H"], s["C"], s["heads"], s["shift"])
    do = _rs64(v["rs"], s["H"] ** 2, att.shape[0]) * (v["dy"].double() @ v["wproj"].double())      # d(attention output) = rowscale * dy . wproj
    gq, gt = torch.autograd.grad(att, [q64, t64], do)
    F.scale("dqkv", A.result("dqkv"), gq, 4e-2)                      # test_gpu_wblock._block_half_case: gradients of the block half
    F.scale("dtable", A.result("dtable"), gt.reshape(-1), 4e-2)


# ================================================================================================ multi-head attention
def _mha_rows(t, bm):
    """(B, L, W) -> the (rows, W) matrix of the layout: time-major row t * B + b, batch-major row b * L + t"""
    B, L, W = t.shape
    return t.reshape(B * L, W).contiguous() if bm else t.transpose(0, 1).reshape(L * B, W).contiguous()


def _mha_unrows(m, B, L, bm):
    W = m.shape[-1]
    return m.reshape(B, L, W) if bm else m.reshape(L, B, W).transpose(0, 1)


def _mha_flags(c):
    return _code(c) | (_lib.BATCH_MAJOR if c.opts.get("batch_major") else 0)


def _mha_keep(lib, flags, dt, E, nh, Lq, Lk, B, p, seed, bm):
    """keep-mask (B, heads, Lq, Lk) of (seed, p): q = k = 0 makes every probability 1 / Lk, one-hot values on head_dim keys at a time leave
    keep / (Lk (1 - p)) in the output (tests/test_gpu_text_encoder.py::test_attention_core_with_dropout_at_the_benchmark_shape)"""
    keep = torch.ones(B, nh, Lq, Lk, dtype=torch.bool, device=DEV)
    if p == 0.0:
        return keep
    hd = E // nh
    es = torch.empty((), dtype=dt).element_size()
    q = torch.zeros(Lq * B, E, dtype=dt, device=DEV)
    for j0 in range(0, Lk, hd):
        w = min(hd, Lk - j0)
        kv = torch.zeros(B, Lk, 2 * E, dtype=dt, device=DEV)
        one_hot = torch.zeros(Lk, hd, dtype=dt, device=DEV)
        one_hot[j0:j0 + w, :w] = torch.eye(w, dtype=dt, device=DEV)
        kv[:, :, E:] = one_hot.repeat(1, nh)[None]
        kvr = _mha_rows(kv, bm)
        out = torch.empty(Lq * B, E, dtype=dt, device=DEV)
        lse = torch.empty(B * nh * Lq, device=DEV)
        rc = lib.fmmt_mha_fwd(flags, Lq, Lk, B, E, nh, q.data_ptr(), E, kvr.data_ptr(), kvr.data_ptr() + E * es, 2 * E, 1.0, None, p, seed, None, out.data_ptr(), E,
                              lse.data_ptr(), _st())
        assert rc == 0, rc
        torch.cuda.synchronize()
        o = _mha_unrows(out, B, Lq, bm).reshape(B, Lq, nh, hd).permute(0, 2, 1, 3)[..., :w].float()
        assert bool(((o == 0) | ((o - _drop_inv(p) / Lk).abs() <= 2e-2 / Lk)).all())      # 0 or inv / Lk, nothing else
        keep[..., j0:j0 + w] = o != 0
    return keep


def _mha_values(c):
    g, dt, s = _gen(c), DT[c.dt], c.shape
    if c.entry.endswith("_ragged"):
        return _ragged_values(c)
    B, Lq, Lk, E, nh = s["B"], s["Lq"], s["Lk"], s["E"], s["heads"]
    bm = c.opts["batch_major"]
    v = dict(q=_randn(g, (B, Lq, E), dt), k=_randn(g, (B, Lk, E), dt), vv=_randn(g, (B, Lk, E), dt), dout=_randn(g, (B, Lq, E), dt), seed=_seed(c), kb=None)
    if c.opts["key_bias"]:                                           # a smooth bias, and -10000 on the last keys of every batch but the first (support_op_cases.t_mha)
        kb = _randn(g, (B, Lk), scale=0.5)
        for b in range(1, B):
            kb[b, Lk - 1 - 3 * b:] += -10000.0
        v["kb"] = kb
    lib = _lib.load()
    v["keep"] = _mha_keep(lib, _mha_flags(c), dt, E, nh, Lq, Lk, B, s["p"], v["seed"], bm)
    if c.entry != "fmmt_mha_fwd":                                    # out and lse of the plain forward call on the same values
        P = SB.Arena(DEV, False)
        fwd = c._replace(entry="fmmt_mha_fwd")
        assert _mha_fwd_run(lib, fwd, v, P) == 0
        v["out"], v["lse"] = _mha_unrows(P.result("out"), B, Lq, bm).contiguous(), P.result("lse").clone()
    return v


def _mha_inputs(c, v, A):
    """q and k / v as views: q at ldq; k and v column slices [0, E) and [E, 2E) of one (rows, 2E) buffer at ldkv -- or two buffers of E columns"""
    s, bm = c.shape, c.opts.get("batch_major", False)
    E = s["E"]
    es = torch.empty((), dtype=DT[c.dt]).element_size()
    q, ldq = A.mat_in("q", _mha_rows(v["q"], bm), ld=s["ldq"])
    if c.opts["separate"]:
        k, ldkv = A.mat_in("k", _mha_rows(v["k"], bm), ld=s["ldkv"])
        vp, _ = A.mat_in("v", _mha_rows(v["vv"], bm), ld=s["ldkv"])
    else:
        k, ldkv = A.mat_in("kv", _mha_rows(torch.cat([v["k"], v["vv"]], -1), bm), ld=s["ldkv"])
        vp = k + E * es
    return q, ldq, k, vp, ldkv


def _mha_fwd_run(lib, c, v, A):
    s = c.shape
    B, Lq, Lk, E, nh = s["B"], s["Lq"], s["Lk"], s["E"], s["heads"]
    q, ldq, k, vp, ldkv = _mha_inputs(c, v, A)
    kb = A.vec_in("key_bias", v["kb"].reshape(-1) if v["kb"] is not None else None)
    out, ldo = A.mat_out("out", Lq * B, E, DT[c.dt], ld=s["ldo"])
    lse = A.vec_out("lse", B * nh * Lq)
    return A.launch(lib.fmmt_mha_fwd, _mha_flags(c), Lq, Lk, B, E, nh, q, ldq, k, vp, ldkv, (E // nh) ** -0.5, kb, s["p"], v["seed"], None, out, ldo, lse, _st())


def _mha_ref(c, v, q64, k64, v64):
    """(out (B, Lq, E), post-dropout probabilities (B, heads, Lq, Lk), lse (B, heads, Lq)) in fp64 on the kernel's keep-mask"""
    s = c.shape
    B, E, nh = s["B"], s["E"], s["heads"]
    hd = E // nh
    hs = lambda t: t.reshape(B, -1, nh, hd).permute(0, 2, 1, 3)
    sc = hs(q64) @ hs(k64).transpose(-1, -2) * hd ** -0.5
    if v["kb"] is not None:
        sc = sc + v["kb"].double()[:, None, None, :]
    pr = torch.softmax(sc, -1) * v["keep"].double() * _drop_inv(s["p"])
    return (pr @ hs(v64)).permute(0, 2, 1, 3).reshape(B, -1, E), pr, torch.logsumexp(sc, -1)


def _mha_tol(c):
    return 2e-5 if c.dt == "f32" else 2e-2                          # support_op_cases.t_mha (forward; gradients at twice that)


def _mha_fwd_parity(c, v, A, F):
    s, bm = c.shape, c.opts["batch_major"]
    ref, _, lse = _mha_ref(c, v, v["q"].double(), v["k"].double(), v["vv"].double())
    F.scale("out", _mha_unrows(A.result("out"), s["B"], s["Lq"], bm), ref, _mha_tol(c))
    F.scale("lse", A.result("lse"), lse.reshape(-1), _mha_tol(c))


def _mha_bwd_run(lib, c, v, A):
    s, bm, dt = c.shape, c.opts["batch_major"], DT[c.dt]
    B, Lq, Lk, E, nh = s["B"], s["Lq"], s["Lk"], s["E"], s["heads"]
    es = torch.empty((), dtype=dt).element_size()
    q, ldq, k, vp, ldkv = _mha_inputs(c, v, A)
    kb = A.vec_in("key_bias", v["kb"].reshape(-1) if v["kb"] is not None else None)
    out, ldo = A.mat_in("out", _mha_rows(v["out"], bm), ld=s["ldo"])      # out and dout share ldo: the ABI says so
    dout, _ = A.mat_in("dout", _mha_rows(v["dout"], bm), ld=s["ldo"])
    lse = A.vec_in("lse", v["lse"])
    dq, lddq = A.mat_out("dq", Lq * B, E, dt, ld=s["lddq"])
    if c.opts["separate"]:
        dk, lddkv = A.mat_out("dk", Lk * B, E, dt, ld=s["lddkv"])
        dv, _ = A.mat_out("dv", Lk * B, E, dt, ld=s["lddkv"])
    else:
        dk, lddkv = A.mat_out("dkv", Lk * B, 2 * E, dt, ld=s["lddkv"])
        dv = dk + E * es
    return A.launch(lib.fmmt_mha_bwd, _mha_flags(c), Lq, Lk, B, E, nh, q, ldq, k, vp, ldkv, (E // nh) ** -0.5, kb, s["p"], v["seed"], None, out, dout, ldo, lse,
                    dq, lddq, dk, dv, lddkv, _st())


def _mha_bwd_parity(c, v, A, F):
    s, bm = c.shape, c.opts["batch_major"]
    B, Lq, Lk, E = s["B"], s["Lq"], s["Lk"], s["E"]
    q64, k64, v64 = (v[n].double().requires_grad_(True) for n in ("q", "k", "vv"))
    ref, _, _ = _mha_ref(c, v, q64, k64, v64)
    gq, gk, gv = torch.autograd.grad(ref, [q64, k64, v64], v["dout"].double())
    tol = 2 * _mha_tol(c)
    F.scale("dq", _mha_unrows(A.result("dq"), B, Lq, bm), gq, tol)
    if c.opts["separate"]:
        dk, dv = A.result("dk"), A.result("dv")
    else:
        dk, dv = A.result("dkv")[:, :E], A.result("dkv")[:, E:]
    F.scale("dk", _mha_unrows(dk, B, Lk, bm), gk, tol)
    F.scale("dv", _mha_unrows(dv, B, Lk, bm), gv, tol)


def _mha_avg_run(lib, c, v, A):
    s = c.shape
    B, Lq, Lk, E, nh = s["B"], s["Lq"], s["Lk"], s["E"], s["heads"]
    q, ldq, k, _, ldkv = _mha_inputs(c, v, A)
    kb = A.vec_in("key_bias", v["kb"].reshape(-1) if v["kb"] is not None else None)
    lse = A.vec_in("lse", v["lse"])
    w = A.vec_out("weights", B * Lq * Lk)
    return A.launch(lib.fmmt_mha_avg_weights, _code(c), Lq, Lk, B, E, nh, q, ldq, k, ldkv, (E // nh) ** -0.5, kb, s["p"], v["seed"], None, lse, w, _st())


def _mha_avg_parity(c, v, A, F):
    _, pr, _ = _mha_ref(c, v, v["q"].double(), v["k"].double(), v["vv"].double())
    F.scale("weights", A.result("weights"), pr.mean(1).reshape(-1), _mha_tol(c))      # the forward's quantity (probabilities): support_op_cases.t_mha


# ---- ragged mode
def _ragged_values(c):
    g, s = _gen(c), c.shape
    bf = torch.bfloat16
    rows, E, nh, T, B = s["rows"], s["E"], s["heads"], s["T"], s["B"]
    lens = torch.tensor(s["lens"], dtype=torch.int32, device=DEV)
    off = (torch.cumsum(lens, 0) - lens).to(torch.int32)
    v = dict(q=_randn(g, (rows, E), bf), kv=_randn(g, (rows, 2 * E), bf), dout=_randn(g, (rows, E), bf), seed=_seed(c), lens=lens, off=off, kb=None)
    lib = _lib.load()
    v["keep"] = _mha_keep(lib, _lib.BF16 | _lib.BATCH_MAJOR, bf, E, nh, T, T, B, s["p"], v["seed"], True)      # the padded call's counters (fmmt_tokens.h)
    if c.entry == "fmmt_mha_bwd_ragged":
        P = SB.Arena(DEV, False)
        assert _ragged_fwd_run(lib, c._replace(entry="fmmt_mha_fwd_ragged"), v, P) == 0
        v["out"], v["lse"] = P.result("out").clone(), P.result("lse").clone()
    return v


def _ragged_code():
    return _lib.BF16 | _lib.RAGGED


def _ragged_inputs(c, v, A):
    s = c.shape
    off, lens = A.vec_in("seq_off", v["off"]), A.vec_in("seq_len", v["lens"])
    q, ldq = A.mat_in("q", v["q"], ld=s["ldq"])
    k, ldkv = A.mat_in("kv", v["kv"], ld=s["ldkv"])
    return off, lens, q, ldq, k, k + s["E"] * 2, ldkv


def _ragged_fwd_run(lib, c, v, A):
    s = c.shape
    off, lens, q, ldq, k, vp, ldkv = _ragged_inputs(c, v, A)
    out, ldo = A.mat_out("out", s["rows"], s["E"], torch.bfloat16, ld=s["ldo"])
    lse = A.vec_out("lse", s["B"] * s["heads"] * s["T"])
    return A.launch(lib.fmmt_mha_fwd_ragged, _ragged_code(), s["T"], s["B"], s["E"], s["heads"], s["rows"], off, lens, q, ldq, k, vp, ldkv, 0.125, s["p"], v["seed"], None,
                    out, ldo, lse, _st())


def _ragged_bwd_run(lib, c, v, A):
    s = c.shape
    off, lens, q, ldq, k, vp, ldkv = _ragged_inputs(c, v, A)
    out, ldo = A.mat_in("out", v["out"], ld=s["ldo"])
    dout, _ = A.mat_in("dout", v["dout"], ld=s["ldo"])
    lse = A.vec_in("lse", torch.nan_to_num(v["lse"], nan=0.0))       # (entries of padded queries were never written: any finite value)
    dq, lddq = A.mat_out("dq", s["rows"], s["E"], torch.bfloat16, ld=s["lddq"])
    dk, lddkv = A.mat_out("dkv", s["rows"], 2 * s["E"], torch.bfloat16, ld=s["lddkv"])
    return A.launch(lib.fmmt_mha_bwd_ragged, _ragged_code(), s["T"], s["B"], s["E"], s["heads"], s["rows"], off, lens, q, ldq, k, vp, ldkv, 0.125, s["p"], v["seed"], None,
                    out, dout, ldo, lse, dq, lddq, dk, dk + s["E"] * 2, lddkv, _st())


def _ragged_ref(c, v, q64, kv64):
    """out (rows, E) in fp64: sequence b attends among its own lens[b] rows, on the padded call's keep-mask; zero rows behind the last sequence"""
    s = c.shape
    E, nh = s["E"], s["heads"]
    hd = E // nh
    outs, r0 = [], 0
    for b, n in enumerate(s["lens"]):
        hs = lambda t: t.reshape(n, nh, hd).transpose(0, 1)
        sc = hs(q64[r0:r0 + n]) @ hs(kv64[r0:r0 + n, :E]).transpose(-1, -2) * 0.125
        pr = torch.softmax(sc, -1) * v["keep"][b, :, :n, :n].double() * _drop_inv(s["p"])
        outs.append((pr @ hs(kv64[r0:r0 + n, E:])).transpose(0, 1).reshape(n, E))
        r0 += n
    outs.append(torch.zeros(s["rows"] - r0, E, dtype=torch.float64, device=DEV))
    return torch.cat(outs, 0)


def _ragged_fwd_parity(c, v, A, F):
    F.scale("out", A.result("out"), _ragged_ref(c, v, v["q"].double(), v["kv"].double()), 2e-2)      # support_op_cases.t_mha, bf16
    total = sum(c.shape["lens"])
    if not bool((A.result("out")[total:] == 0).all()):
        F.append("out: rows behind the last sequence are not zero-filled")
    lse = A.result("lse").reshape(c.shape["B"], c.shape["heads"], c.shape["T"])
    for b, n in enumerate(c.shape["lens"]):
        if not bool(torch.isfinite(lse[b, :, :n]).all()):
            F.append(f"lse: sequence {b} has unwritten entries among its {n} real queries")


def _ragged_bwd_parity(c, v, A, F):
    s = c.shape
    q64, kv64 = v["q"].double().requires_grad_(True), v["kv"].double().requires_grad_(True)
    gq, gkv = torch.autograd.grad(_ragged_ref(c, v, q64, kv64), [q64, kv64], v["dout"].double())
    total = sum(s["lens"])
    gq[total:], gkv[total:] = 0.0, 0.0
    F.scale("dq", A.result("dq"), gq, 4e-2)                          # support_op_cases.t_mha, bf16 gradients
    F.scale("dk", A.result("dkv")[:, :s["E"]], gkv[:, :s["E"]], 4e-2)
    F.scale("dv", A.result("dkv")[:, s["E"]:], gkv[:, s["E"]:], 4e-2)
    if not bool((A.result("dq")[total:] == 0).all() and (A.result("dkv")[total:] == 0).all()):
        F.append("dq / dk / dv: rows behind the last sequence are not zero-filled")


# ================================================================================================ the table -> functions
# entry point -> (values, run, parity, names of outputs documented as partly unwritten)
ENTRY = {
    "fmmt_layernorm_fwd": (_ln_values, _ln_fwd_run, _ln_fwd_parity, ()),
    "fmmt_layernorm_bwd": (_ln_values, _ln_bwd_run, _ln_bwd_parity, ()),
    "fmmt_mlp_fwd": (_mlp_values, _mlp_fwd_run, _mlp_fwd_parity, ()),
    "fmmt_mlp_ln_fwd": (_mlp_values, _mlp_fwd_run, _mlp_fwd_parity, ()),
    "fmmt_mlp_bwd_input": (_mlp_values, _mlp_bwd_run, _mlp_bwd_parity, ()),
    "fmmt_mlp_ln_bwd_input": (_mlp_values, _mlp_bwd_run, _mlp_bwd_parity, ()),
    "fmmt_linear_ln_bwd": (_lin_values, _lin_run, _lin_parity, ()),
    "fmmt_patch_embed_ln_fwd": (_patch_values, _patch_run, _patch_parity, ()),
    "fmmt_layernorm_bwd_bf16": (_tail_values, _tail_bwd_run, _tail_bwd_parity, ()),
    "fmmt_dropadd_ln_fwd": (_tail_values, _tail_fwd_run, _tail_fwd_parity, ()),
    "fmmt_dropadd_ln_bwd": (_tail_values, _tail_bwd_run, _tail_bwd_parity, ()),
    "fmmt_plm_dropadd_ln_fwd": (_tail_values, _tail_fwd_run, _tail_fwd_parity, ()),
    "fmmt_plm_dropadd_ln_bwd": (_tail_values, _tail_bwd_run, _tail_bwd_parity, ()),
    "fmmt_plm_gelu_bwd_colsum": (_tail_values, _colsum_run, _colsum_parity, ()),
    "fmmt_window_attn_fwd": (_wattn_values, _wattn_fwd_run, _wattn_fwd_parity, ()),
    "fmmt_window_attn_bwd": (_wattn_values, _wattn_bwd_run, _wattn_bwd_parity, ()),
    "fmmt_window_block_fwd": (_wblock_values, _wblock_fwd_run, _wblock_fwd_parity, ()),
    "fmmt_window_block_attn_bwd": (_wblock_values, _wblock_bwd_run, _wblock_bwd_parity, ()),
    "fmmt_mha_fwd": (_mha_values, _mha_fwd_run, _mha_fwd_parity, ()),
    "fmmt_mha_bwd": (_mha_values, _mha_bwd_run, _mha_bwd_parity, ()),
    "fmmt_mha_avg_weights": (_mha_values, _mha_avg_run, _mha_avg_parity, ()),
    "fmmt_mha_fwd_ragged": (_mha_values, _ragged_fwd_run, _ragged_fwd_parity, ("lse",)),
    "fmmt_mha_bwd_ragged": (_mha_values, _ragged_bwd_run, _ragged_bwd_parity, ()),
}


def test_every_entry_point_of_the_table_has_its_functions():
    assert {c.entry for c in BC.CASES} == set(ENTRY)


@pytest.mark.parametrize("c", BC.CASES, ids=lambda c: c.id)
def test_kernel_bounds(c):
    lib = _lib.load()
    values, run, parity, unwritten_ok = ENTRY[c.entry]
    v = values(c)
    P = SB.Arena(DEV, guarded=False)
    assert run(lib, c, v, P) == 0, "the plain call was refused"
    G = SB.Arena(DEV, guarded=True)
    rc = run(lib, c, v, G)
    assert rc == 0, f"the call on views was refused: {rc}"
    assert set(G.outputs) == set(P.outputs)
    # 1. bit-identity with the plain call
    for name in G.outputs:
        same = torch.equal(SB.bits(G.result(name)), SB.bits(P.result(name)))
        assert same, f"{name}: what lies around the operands (or in the workspace) changed the result"
    # 2. parity with the fp64 restatement
    F = Findings(c)
    parity(c, v, G, F)
    assert F == [], list(F)
    # 3. - 5. no stray write, nothing unwritten and no padding in a result, inputs unchanged
    found = G.problems(unwritten_ok)
    assert found == [], found
    # 6. a workspace one byte short
    if G.ws:
        S = SB.Arena(DEV, guarded=True, short=True)
        assert run(lib, c, v, S) == EWORKSPACE
        assert all(bool(torch.isnan(S.result(n)).all()) for n in S.outputs), "a refused call wrote into an output"
        assert [p for p in S.problems(tuple(S.outputs)) if "stray" in p or "modified" in p] == []
