"""The normalisation, softmax and GELU kernels on hard input VALUES (tests/support_value_cases.py has the classes, the class-local metric and the
yardstick; tests/test_value_cases_cpu.py shows on the CPU that the honest restatement passes them and each wrong one misses by >= 10x).

Every parity check reads: ref = the fp64 restatement on the same, already rounded, inputs; stock = the stock torch composition of the op in the same
element type on the same device and inputs; a class passes at max(base, K * stock) with `base` the tolerance the op's existing test holds it to (named
at each check).  Constant rows have the derived bound of support_value_cases.const_row_bound instead, and get a zero upstream gradient: their x-hat is
0 +- that bound, which no summation over rows should have to absorb.

Far-tail GELU: identity weights put +-{8.5, 20, 1e3, 1e30} on the epilogues themselves, as support_op_cases.t_gelu_tail does on [-8, 8].

Non-finite footprint: each op runs clean, then with one input element NaN and again +inf.  Every output element that depends on that element must be
non-finite; every other one bit-identical to the clean run (a NaN leaking through a shared maximum, a shared reduction or a neighbouring lane).  Two
places where the dependence is not what a first guess says: d(beta) of a LayerNorm does not depend on x at all (it is the column sum of dy) and is held
to the clean bits; a value element v[j, b, h, d] reaches channel d of head h only.  The bf16 GELU forms are the documented exception of
include/fmmt.h (a NaN pre-activation comes out finite: keeping it cost bench time), held here at the level where the property survives: the stored
pre-activation, and the poisoned element itself through the residual of x + Mlp(x) and x + Mlp(LayerNorm(x)).  A key at +inf legitimately gives weight 0 to a query whose
logit with it is -inf, so keys are poisoned with NaN only."""
import math

import pytest
import torch
import torch.nn.functional as F

from facialmmt_amd import ops
from facialmmt_amd._lib import EPI_GELU, EPI_GELU_BWD, EPI_GELU_DG, EPI_MUL_AUX, EPI_NONE
from tests import support_value_cases as V

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
EPS = 1e-5
LN_BASE = {F32: 1e-5, BF16: 1.5e-2}           # support_op_cases.t_layernorm (forward; gradients 2x)
ATTN_BASE = {F32: 2e-5, BF16: 2e-2}           # support_op_cases.t_mha / t_wattn (forward; gradients 2x)
BF16_STEP = 2.0 ** -8                          # half a bf16 rounding step, relative


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _leaf(t, dev, dtype=None):
    t = t.to(dev)
    if dtype is not None:
        t = t.to(dtype)
    return t.detach().clone().requires_grad_(True)


def _finite(**tensors):
    bad = [k for k, t in tensors.items() if not bool(torch.isfinite(t.detach().float()).all())]
    assert not bad, f"non-finite outputs: {bad}"


# ====================================================================================================================== LayerNorm statistics
def _norm_case(M, C, dtype, seed, classes=V.NORM_CLASSES):
    x, cls, omask = V.norm_rows(M, C, dtype, seed=seed, classes=classes)
    g = V.randn((C,), seed + 2) * 0.2 + 1
    b = V.randn((C,), seed + 3) * 0.1
    dy = V.randn((M, C), seed + 4)
    for i, name in enumerate(classes):
        if name in V.CONST_CLASSES:
            dy[cls == i] = 0.0
    return x, g, b, dy.to(dtype), cls, omask


def _check_const_rows(y, beta, gamma, cls, classes, dtype, eps=EPS):
    """rows of equal elements: |y - beta| <= const_row_bound (plus the output's own rounding in bf16); c = 0 gives beta exactly"""
    y, beta = y.detach().float().cpu(), beta.detach().float().cpu()
    for i, name in enumerate(classes):
        if name not in V.CONST_CLASSES:
            continue
        c = V.CONST_CLASSES[name]
        rows = y[cls == i]
        want = beta.to(dtype).float() if c == 0.0 else beta
        bar = V.const_row_bound(gamma, c, eps)
        if dtype == BF16 and c != 0.0:
            bar = bar + BF16_STEP * (float(beta.abs().max()) + bar)
        dev_ = float((rows - want).abs().max())
        print(f"     const row c={c:g}: max|y - beta| = {dev_:.3e} (bound {bar:.3e})")
        assert bool(torch.isfinite(rows).all()) and dev_ <= bar, (name, dev_, bar)


def _judge_norm(case, got, ref, stock, cls, omask, classes, base, failures):
    skip = tuple(V.CONST_CLASSES)
    V.judge(case, V.class_errors(got, ref, cls, classes, omask, skip=skip), V.class_errors(stock, ref, cls, classes, omask, skip=skip), base, failures)


@DTYPES
@pytest.mark.parametrize("C", V.LN_CHANNELS)
def test_layer_norm_row_classes(dev, dtype, C):
    """ops.layer_norm (csrc/layernorm.hip) forward and backward, M = 66 rows of every class"""
    M, base = 66, LN_BASE[dtype]
    x, g, b, dy, cls, omask = _norm_case(M, C, dtype, seed=C)
    xd, gd, bd = _leaf(x, dev), _leaf(g, dev), _leaf(b, dev)
    y = ops.layer_norm(xd, gd, bd, EPS)
    dx, dg, db = torch.autograd.grad(y, [xd, gd, bd], dy.to(dev))
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, g, b))
    yr = V.layer_norm64(x64, g64, b64, EPS)
    rx, rg, rb = torch.autograd.grad(yr, [x64, g64, b64], dy.double())
    xs, gs, bs = _leaf(x, dev), _leaf(g, dev, dtype), _leaf(b, dev, dtype)
    ys = F.layer_norm(xs, (C,), gs, bs, EPS)
    sx, sg, sb = torch.autograd.grad(ys, [xs, gs, bs], dy.to(dev))
    _finite(y=y, dx=dx, dgamma=dg, dbeta=db)
    failures = []
    tag = f"layer_norm {str(dtype)[6:]} C={C}"
    _judge_norm(f"{tag} y", y, yr, ys, cls, omask, V.NORM_CLASSES, base, failures)                      # base: t_layernorm
    _judge_norm(f"{tag} dx", dx, rx, sx, cls, omask, V.NORM_CLASSES, 2 * base, failures)                # base: t_layernorm, gradients
    V.judge(f"{tag} dparam", {"dgamma": V.rel_err(dg, rg), "dbeta": V.rel_err(db, rb)}, {"dgamma": V.rel_err(sg, rg), "dbeta": V.rel_err(sb, rb)}, 2 * base, failures)
    _check_const_rows(y, b, g, cls, V.NORM_CLASSES, dtype)
    assert not failures, failures


def _unmerge(rows, n, H, Cq):
    """inverse of Swin's patch-merging gather: merged rows (n * H/2 * H/2, 4 Cq) -> x (n, H * H, Cq)"""
    r = rows.reshape(n, H // 2, H // 2, 4, Cq)
    x = torch.empty(n, H // 2, 2, H // 2, 2, Cq, dtype=rows.dtype)
    x[:, :, 0, :, 0], x[:, :, 1, :, 0], x[:, :, 0, :, 1], x[:, :, 1, :, 1] = r[..., 0, :], r[..., 1, :], r[..., 2, :], r[..., 3, :]
    return x.reshape(n, H * H, Cq)


def _merge(x, n, H, Cq):
    gq = x.reshape(n, H // 2, 2, H // 2, 2, Cq)
    return torch.cat([gq[:, :, 0, :, 0], gq[:, :, 1, :, 0], gq[:, :, 0, :, 1], gq[:, :, 1, :, 1]], -1).reshape(-1, 4 * Cq)


@DTYPES
def test_layer_norm_merge_row_classes(dev, dtype):
    """the patch-merging LayerNorm (merge_hw): the classes laid on the MERGED rows (49 rows of 4 * 96 channels), forward and d(x)"""
    n, H, Cq, base = 1, 14, 96, LN_BASE[dtype]
    M, C = n * (H // 2) ** 2, 4 * Cq
    rows, g, b, dy, cls, omask = _norm_case(M, C, dtype, seed=41)
    x = _unmerge(rows, n, H, Cq)
    assert torch.equal(_merge(x, n, H, Cq), rows)
    xd = _leaf(x, dev)
    y = ops.layer_norm(xd, g.to(dev), b.to(dev), EPS, H)
    (dx,) = torch.autograd.grad(y, [xd], dy.to(dev).reshape(y.shape))
    x64 = x.double().requires_grad_(True)
    yr = V.layer_norm64(_merge(x64, n, H, Cq), g.double(), b.double(), EPS)
    (rx,) = torch.autograd.grad(yr, [x64], dy.double())
    xs = _leaf(x, dev)
    ys = F.layer_norm(_merge(xs, n, H, Cq), (C,), g.to(dev).to(dtype), b.to(dev).to(dtype), EPS)
    (sx,) = torch.autograd.grad(ys, [xs], dy.to(dev))
    _finite(y=y, dx=dx)
    failures = []
    tag = f"layer_norm merge {str(dtype)[6:]}"
    _judge_norm(f"{tag} y", y.reshape(M, C), yr, ys, cls, omask, V.NORM_CLASSES, base, failures)        # base: t_layernorm (ln merge fwd)
    mg = lambda t: _merge(t.detach().cpu().double(), n, H, Cq)
    _judge_norm(f"{tag} dx", mg(dx), mg(rx), mg(sx), cls, omask, V.NORM_CLASSES, 2 * base, failures)
    _check_const_rows(y.reshape(M, C), b, g, cls, V.NORM_CLASSES, dtype)
    assert not failures, failures


@DTYPES
def test_residual_layer_norm_row_classes(dev, dtype):
    """ops.residual_layer_norm (the LayerNorm in front of a fused Swin half, csrc/misc.hip): forward and backward through the normalised output"""
    M, C, base = 66, 96, LN_BASE[dtype]
    x, g, b, dy, cls, omask = _norm_case(M, C, dtype, seed=43)
    xd, gd, bd = _leaf(x, dev), _leaf(g, dev), _leaf(b, dev)
    xr, xn = ops.residual_layer_norm(xd, gd, bd, EPS)
    assert torch.equal(xr.detach(), xd.detach())
    dres = (V.randn((M, C), 44) * (dy.float() != 0)).to(dtype)                   # the residual branch's gradient: the `add` operand of the backward kernel
    dx, dg, db = torch.autograd.grad([xr, xn], [xd, gd, bd], [dres.to(dev), dy.to(dev)])
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, g, b))
    yr = V.layer_norm64(x64, g64, b64, EPS)
    rx, rg, rb = torch.autograd.grad([x64 * 1.0, yr], [x64, g64, b64], [dres.double(), dy.double()])
    xs, gs, bs = _leaf(x, dev), _leaf(g, dev, dtype), _leaf(b, dev, dtype)
    ys = F.layer_norm(xs, (C,), gs, bs, EPS)
    sx, sg, sb = torch.autograd.grad([xs * 1.0, ys], [xs, gs, bs], [dres.to(dev), dy.to(dev)])
    _finite(xn=xn, dx=dx, dgamma=dg, dbeta=db)
    failures = []
    tag = f"residual_layer_norm {str(dtype)[6:]}"
    _judge_norm(f"{tag} y", xn, yr, ys, cls, omask, V.NORM_CLASSES, base, failures)                    # base: t_layernorm
    _judge_norm(f"{tag} dx", dx, rx, sx, cls, omask, V.NORM_CLASSES, 2 * base, failures)
    V.judge(f"{tag} dparam", {"dgamma": V.rel_err(dg, rg), "dbeta": V.rel_err(db, rb)}, {"dgamma": V.rel_err(sg, rg), "dbeta": V.rel_err(sb, rb)}, 2 * base, failures)
    _check_const_rows(xn, b, g, cls, V.NORM_CLASSES, dtype)
    assert not failures, failures


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dropadd_layer_norm_offset_through_the_operands(dev, p):
    """ops.dropadd_layer_norm (bf16 operands, fp32 parameters, eps 1e-12; M 76, C 768): LayerNorm(dropout(h) + res) where the offset rows carry
    h = +1024 + a and res = -1024 + b (both rounded to bf16, a and b of scale 8: the grid there): the sum is exact only if it is formed in fp32.
    p = 0.1: on the mask the kernel drew, read back by a launch on h = 1, res = 0 (the recipe of tests/test_gpu_glue.py) -- a dropped element of an
    offset row leaves -1024 beside kept ones near +120, a row with |mean| and spread both in the hundreds."""
    from facialmmt_amd import _lib
    M, C, eps, dtype = 76, 768, 1e-12, BF16
    classes = ("unit", "offset", "outlier", "tiny")
    base, gbase = (1e-2, 3e-2) if p == 0.0 else (2e-2, 3e-2)                     # tests/test_gpu_glue.py: forward at p = 0 / on the mask, gradients
    h, cls, omask = V.norm_rows(M, C, dtype, seed=51, classes=("unit", "unit", "outlier", "tiny"))
    res = (0.05 * V.randn((M, C), 52)).to(dtype)
    off = cls == 1
    h[off] = (1024.0 + 8.0 * V.randn((int(off.sum()), C), 53)).to(dtype)
    res[off] = (-1024.0 + 8.0 * V.randn((int(off.sum()), C), 54)).to(dtype)
    g = V.randn((C,), 55) * 0.1 + 1
    b = V.randn((C,), 56) * 0.1
    dy = V.randn((M, C), 57).to(dtype)
    seed = torch.tensor([777], device=dev, dtype=torch.int64)
    hd, rd, gd, bd = _leaf(h, dev), _leaf(res, dev), _leaf(g, dev), _leaf(b, dev)
    keep = torch.ones((M, C), dtype=torch.bool, device=dev)
    if p > 0.0:
        ones, zeros = torch.ones(M, C, device=dev, dtype=dtype), torch.zeros(M, C, device=dev, dtype=dtype)
        probe, junk = torch.empty_like(ones), torch.empty_like(ones)
        _lib.check(_lib.load().fmmt_dropadd_ln_fwd(_lib.dtype_code(F32), M, C, eps, ones.data_ptr(), zeros.data_ptr(), gd.data_ptr(), bd.data_ptr(), p, 0,
                                                   seed.data_ptr(), 3, probe.data_ptr(), junk.data_ptr(), torch.cuda.current_stream().cuda_stream), "probe")
        keep = probe != 0
        assert abs(float(keep.float().mean()) - (1 - p)) < 0.01
    y = ops.dropadd_layer_norm(hd, rd, gd, bd, eps, p, seed, 3)
    dh, dr, dg, db = torch.autograd.grad(y, [hd, rd, gd, bd], dy.to(dev))
    k64 = keep.cpu().double() / (1.0 - p)
    h64, r64, g64, b64 = (t.double().requires_grad_(True) for t in (h, res, g, b))
    yr = V.layer_norm64(h64 * k64 + r64, g64, b64, eps)
    rh, rr, rg, rb = torch.autograd.grad(yr, [h64, r64, g64, b64], dy.double())
    hs, rs, gs, bs = _leaf(h, dev), _leaf(res, dev), _leaf(g, dev, dtype), _leaf(b, dev, dtype)
    ys = F.layer_norm(hs * (keep.to(dtype) * (1.0 / (1.0 - p))) + rs, (C,), gs, bs, eps)      # the bf16 module, op by op, on the same mask
    sh, sr, sg, sb = torch.autograd.grad(ys, [hs, rs, gs, bs], dy.to(dev))
    _finite(y=y, dh=dh, dres=dr, dgamma=dg, dbeta=db)
    if p > 0.0:
        assert bool((dh[~keep] == 0).all())
    failures = []
    tag = f"dropadd_ln p={p:g}"
    _judge_norm(f"{tag} y", y, yr, ys, cls, omask, classes, base, failures)
    _judge_norm(f"{tag} dh", dh, rh, sh, cls, omask, classes, gbase, failures)
    _judge_norm(f"{tag} dres", dr, rr, sr, cls, omask, classes, gbase, failures)
    V.judge(f"{tag} dparam", {"dgamma": V.rel_err(dg, rg), "dbeta": V.rel_err(db, rb)}, {"dgamma": V.rel_err(sg, rg), "dbeta": V.rel_err(sb, rb)}, gbase, failures)
    assert not failures, failures


@DTYPES
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("n", [2, 7])
def test_batch_norm_1d_column_classes(dev, dtype, training, n):
    """ops.batch_norm_1d (csrc/bn1d_core.h): the columns play the role of rows -- column c of the (n, 512) input is row c of norm_rows(512, n)"""
    Cn, base = 512, LN_BASE[dtype]                                               # base: t_misc's bn bars (forward tol, gradients 4x)
    classes = tuple(c for c in V.NORM_CLASSES if not (n == 2 and c == "outlier"))
    cols, cls, omask = V.norm_rows(Cn, n, dtype, seed=60 + n, classes=classes)
    x = cols.t().contiguous()
    g = V.randn((Cn,), 61) * 0.2 + 1
    b = V.randn((Cn,), 62) * 0.1
    rm, rv = V.randn((Cn,), 63) * 0.1, V.randn((Cn,), 64).abs() + 0.5
    dy = V.randn((n, Cn), 65)
    for i, name in enumerate(classes):
        if name in V.CONST_CLASSES:
            dy[:, cls == i] = 0.0
    dy = dy.to(dtype)
    xd, gd, bd = _leaf(x, dev), _leaf(g, dev), _leaf(b, dev)
    y = ops.batch_norm_1d(xd, gd, bd, rm.clone().to(dev), rv.clone().to(dev), 0.1, EPS, training)
    dx, dg = torch.autograd.grad(y, [xd, gd], dy.to(dev))
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, g, b))
    yr = F.batch_norm(x64, rm.double(), rv.double(), g64, b64, training, 0.1, EPS)
    rx, rg = torch.autograd.grad(yr, [x64, g64], dy.double())
    xs, gs, bs = _leaf(x, dev), _leaf(g, dev, dtype), _leaf(b, dev, dtype)
    ys = F.batch_norm(xs, rm.to(dev).to(dtype), rv.to(dev).to(dtype), gs, bs, training, 0.1, EPS)
    sx, sg = torch.autograd.grad(ys, [xs, gs], dy.to(dev))
    _finite(y=y, dx=dx, dgamma=dg)
    failures = []
    tag = f"batch_norm_1d {str(dtype)[6:]} n={n} {'train' if training else 'eval'}"
    T = lambda t: t.detach().cpu().double().t()
    skip = tuple(V.CONST_CLASSES) if training else ()
    V.judge(f"{tag} y", V.class_errors(T(y), T(yr), cls, classes, omask, skip=skip), V.class_errors(T(ys), T(yr), cls, classes, omask, skip=skip), base, failures)
    V.judge(f"{tag} dx", V.class_errors(T(dx), T(rx), cls, classes, omask, skip=skip), V.class_errors(T(sx), T(rx), cls, classes, omask, skip=skip), 4 * base, failures)
    for i, name in enumerate(classes):                                           # d(gamma) is per column: judged per class of columns
        m = cls == i
        if name in V.CONST_CLASSES and training:
            continue
        V.judge(f"{tag} dgamma", {name: V.rel_err(dg.cpu()[m], rg[m])}, {name: V.rel_err(sg.cpu()[m], rg[m])}, 4 * base, failures)
    if training:
        for i, name in enumerate(classes):
            if name in V.CONST_CLASSES:
                c, m = V.CONST_CLASSES[name], cls == i
                bar = float(g[m].abs().max()) * abs(c) * 2.0 ** -22 / math.sqrt(EPS)
                if dtype == BF16 and c != 0.0:
                    bar = bar + BF16_STEP * (float(b[m].abs().max()) + bar)
                want = b[m].to(dtype).float() if c == 0.0 else b[m]
                dev_ = float((y.detach().float().cpu()[:, m] - want).abs().max())
                assert dev_ <= bar, (name, dev_, bar)
    assert not failures, failures


def _mlp_ln_params(C, seed):
    return dict(g=V.randn((C,), seed + 1) * 0.2 + 1, b=V.randn((C,), seed + 2) * 0.1, w1=V.randn((4 * C, C), seed + 3) * C ** -0.5, b1=V.randn((4 * C,), seed + 4) * 0.1,
                w2=V.randn((C, 4 * C), seed + 5) * (4 * C) ** -0.5, b2=V.randn((C,), seed + 6) * 0.1)


def _mlp_ln_ref(x, P, eps=EPS):
    return x + (F.gelu(F.layer_norm(x, (x.shape[-1],), P["g"], P["b"], eps) @ P["w1"].t() + P["b1"]) @ P["w2"].t() + P["b2"])


@DTYPES
@pytest.mark.parametrize("C", [96, 192])
def test_mlp_ln_row_classes(dev, dtype, C, monkeypatch):
    """ops.mlp_ln (x + Mlp(LayerNorm(x)); csrc/mlp_fused.hip in bf16, csrc/mlp_ref.hip in fp32; the backward through fmmt_mlp_ln_bwd_input at C = 96) at
    M = 4096, the fused threshold.  The `big` rows are left out: x + Mlp(.) of 1e15 loses the Mlp in any arithmetic.  The judged outputs are y - x's
    carrier x-hat (the saved LayerNorm output is internal), so: y and d(x), per class."""
    monkeypatch.setattr(ops, "_MLP_FUSED_WIDTHS", (96, 192))
    M = 4096
    classes = ("unit", "offset", "outlier", "tiny", "const0", "const1024")
    fwd, bwd = {F32: (1e-4, 1e-3), BF16: (2e-2, 4e-2)}[dtype]                    # base: tests/test_gpu_wblock.py (fp32 instantiation / bf16 mlp half)
    x, cls, omask = V.norm_rows(M, C, dtype, seed=70 + C, classes=classes)
    P = _mlp_ln_params(C, 80 + C)
    dy = V.randn((M, C), 77)
    const = torch.zeros(M, dtype=torch.bool)
    for i, name in enumerate(classes):
        if name in V.CONST_CLASSES:
            const |= cls == i
    dy[const] = 0.0
    dy = dy.to(dtype)
    xd = _leaf(x, dev)
    Pd = {k: _leaf(v, dev) for k, v in P.items()}
    assert ops.mlp_ln_fusable(xd, Pd["w1"], Pd["w2"], Pd["b1"], Pd["b2"])
    y = ops.mlp_ln(xd, Pd["g"], Pd["b"], EPS, Pd["w1"], Pd["b1"], Pd["w2"], Pd["b2"])
    names = ["g", "b", "w1", "b1", "w2", "b2"]
    grads = torch.autograd.grad(y, [xd] + [Pd[k] for k in names], dy.to(dev))
    x64 = x.double().requires_grad_(True)
    P64 = {k: (v.to(dtype).double() if k in ("w1", "w2") else v.double()).requires_grad_(True) for k, v in P.items()}     # the GEMM weights are read in `dtype`
    yr = _mlp_ln_ref(x64, P64)
    gref = torch.autograd.grad(yr, [x64] + [P64[k] for k in names], dy.double())
    xs = _leaf(x, dev)
    Ps = {k: _leaf(v, dev, dtype) for k, v in P.items()}
    ys = _mlp_ln_ref(xs, Ps)
    gst = torch.autograd.grad(ys, [xs] + [Ps[k] for k in names], dy.to(dev))
    _finite(y=y, **{"d" + k: t for k, t in zip(["x"] + names, grads)})
    failures = []
    tag = f"mlp_ln {str(dtype)[6:]} C={C}"
    # y = x + Mlp: on offset / const1024 rows the Mlp's share is what is judged, so the residual is taken off all three first (exactly: |x| <= 1040)
    sub = lambda t: t.detach().cpu().double() - x.double()
    # (constant rows: x-hat is 0 +- const_row_bound, which the Mlp turns into an O(bound) change of its output -- finite is what is asked of them)
    skip = tuple(V.CONST_CLASSES)
    V.judge(f"{tag} y - x", V.class_errors(sub(y), sub(yr), cls, classes, omask, skip), V.class_errors(sub(ys), sub(yr), cls, classes, omask, skip), fwd, failures)
    d1 = lambda t: t.detach().cpu().double() - dy.double()                       # d(x) = dy + the branch's share
    V.judge(f"{tag} dx - dy", V.class_errors(d1(grads[0]), d1(gref[0]), cls, classes, omask, skip), V.class_errors(d1(gst[0]), d1(gref[0]), cls, classes, omask, skip), bwd,
            failures)
    V.judge(f"{tag} dparam", {"d" + k: V.rel_err(a, r) for k, a, r in zip(names, grads[1:], gref[1:])},
            {"d" + k: V.rel_err(s, r) for k, s, r in zip(names, gst[1:], gref[1:])}, bwd, failures)
    assert not failures, failures


# ====================================================================================================================== softmax: multi-head attention
MHA_SHAPES = [(70, 130, 2, 768, 12), (70, 33, 2, 256, 8)]
MHA_CASES = [(s, None) for s in V.SCORE_KINDS] + [("unit", kb) for kb in V.KEY_BIAS_KINDS]


@DTYPES
@pytest.mark.parametrize("packed", [True, False], ids=["packed-kv", "separate-kv"])
@pytest.mark.parametrize("shape", MHA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mha_core_score_classes(dev, dtype, packed, shape):
    """ops.mha_core forward and backward: the MFMA kernels (bf16, head_dim 64: csrc/mha_mfma.hip) and the VALU ones (fp32, and head_dim 32:
    csrc/attn.hip), k | v packed and separate, over the score classes and every key_bias variant"""
    Lq, Lk, B, E, nh = shape
    scale, base = (E // nh) ** -0.5, ATTN_BASE[dtype]
    failures = []
    for score, bias in MHA_CASES:
        q, k, v = V.mha_inputs(score, Lq, Lk, B, E, nh, dtype, seed=90)
        kb = V.key_bias(bias, B, Lk, seed=90) if bias else None
        dy = V.randn((Lq, B, E), 94).to(dtype)
        qd, kd, vd = _leaf(q, dev), _leaf(k, dev), _leaf(v, dev)
        kbd = kb.to(dev) if kb is not None else None
        if packed:
            kv = torch.cat([kd, vd], -1).detach().requires_grad_(True)
            out = ops.mha_core(qd, kv, None, nh, scale, 0.0, 0, kbd)
            dq, dkv = torch.autograd.grad(out, [qd, kv], dy.to(dev))
            dk, dv = dkv[..., :E], dkv[..., E:]
        else:
            out = ops.mha_core(qd, kd, vd, nh, scale, 0.0, 0, kbd)
            dq, dk, dv = torch.autograd.grad(out, [qd, kd, vd], dy.to(dev))
        q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
        ref = V.attention(q64, k64, v64, nh, scale, kb)
        rq, rk, rv = torch.autograd.grad(ref, [q64, k64, v64], dy.double())
        qs, ks, vs = _leaf(q, dev), _leaf(k, dev), _leaf(v, dev)
        st = V.attention(qs, ks, vs, nh, scale, kbd)
        sq, sk, sv = torch.autograd.grad(st, [qs, ks, vs], dy.to(dev))
        tag = f"mha {str(dtype)[6:]} {Lq}x{Lk} E{E} {'kv' if packed else 'k,v'} {score} {bias or '-'}"
        got = dict(out=out, dq=dq, dk=dk, dv=dv)
        bad = [n for n, t in got.items() if not bool(torch.isfinite(t.float()).all())]
        if bad:
            failures.append(f"{tag}: non-finite {bad}")
        V.judge(tag, {"out": V.rel_err(out, ref)}, {"out": V.rel_err(st, ref)}, base, failures)                     # base: t_mha forward
        V.judge(tag, {"dq": V.rel_err(dq, rq), "dk": V.rel_err(dk, rk), "dv": V.rel_err(dv, rv)},
                {"dq": V.rel_err(sq, rq), "dk": V.rel_err(sk, rk), "dv": V.rel_err(sv, rv)}, 2 * base, failures)    # base: t_mha gradients
        if bias == "one":                       # one key left: out is that key's v, dq and dk are 0 absolutely (t_mha's Lk = 1 check)
            for b_ in range(B):
                want = v[V.one_key(b_, Lk), b_].float()
                e = float((out[:, b_].float().cpu() - want).abs().max())
                if not e <= base * float(want.abs().max()):
                    failures.append(f"{tag}: out of batch element {b_} is not the surviving key's v ({e:.3e})")
            for nm, t in (("dq", dq), ("dk", dk)):
                if not float(t.float().abs().max()) <= 1e-5:
                    failures.append(f"{tag}: |{nm}| = {float(t.float().abs().max()):.3e} > 1e-5 with a single live key")
    assert not failures, failures


def test_mha_avg_weights_under_minus_inf_bias(dev):
    """ops.mha_avg_weights (the head-averaged probabilities the cross-modal encoder returns) from the saved log-sum-exp, with -inf on leading keys"""
    Lq, Lk, B, E, nh = 70, 130, 2, 768, 12
    scale = (E // nh) ** -0.5
    failures = []
    for dtype in (F32, BF16):
        for bias in ("lead8", "lead70", "scatter", "one"):
            q, k, v = V.mha_inputs("unit", Lq, Lk, B, E, nh, dtype, seed=100)
            kb = V.key_bias(bias, B, Lk, seed=100)
            qd, kd, vd, kbd = q.to(dev), k.to(dev), v.to(dev), kb.to(dev)
            with torch.no_grad():
                out, lse = ops.mha_core(qd, kd, vd, nh, scale, 0.0, 0, kbd, return_lse=True)
                w = ops.mha_avg_weights(qd, kd, lse, nh, scale, 0.0, 0, kbd)
            s64 = (V.heads(q.double(), nh) * scale) @ V.heads(k.double(), nh).transpose(-1, -2) + kb.double()[:, None, None, :]
            ref = torch.softmax(s64, -1).mean(1)
            ss = (V.heads(qd, nh) * scale) @ V.heads(kd, nh).transpose(-1, -2) + kbd.to(dtype)[:, None, None, :]
            stock = torch.softmax(ss, -1).float().mean(1)
            assert tuple(w.shape) == tuple(ref.shape), (w.shape, ref.shape)
            if not bool(torch.isfinite(w.float()).all()):
                failures.append(f"avg_weights {dtype} {bias}: non-finite")
            V.judge(f"mha_avg_weights {str(dtype)[6:]} {bias}", {"w": V.rel_err(w, ref)}, {"w": V.rel_err(stock, ref)}, ATTN_BASE[dtype], failures)   # base: t_mha
            if not float(w.float().cpu()[~torch.isfinite(kb)[:, None, :].expand_as(ref)].abs().max()) == 0.0:
                failures.append(f"avg_weights {dtype} {bias}: weight on a key at -inf")
    assert not failures, failures


# ====================================================================================================================== softmax: window attention
def _wattn_ref(qkv, table, mask, n_img, H, C, nh, shift):
    """support_op_cases._wattn_ref (that module opens the device at import: restated here on the oracle's index helpers)"""
    from oracle import swin as OS
    idx = OS.window_token_index(H, H, 7, shift).to(qkv.device)
    nW, hd = idx.shape[0], C // nh
    t = qkv.reshape(n_img, H * H, 3, nh, hd)[:, idx.reshape(-1)].reshape(n_img * nW, 49, 3, nh, hd)
    q = t[:, :, 0].transpose(1, 2) * hd ** -0.5
    k, v = t[:, :, 1].transpose(1, 2), t[:, :, 2].transpose(1, 2)
    s = q @ k.transpose(-1, -2) + table[OS.relative_position_index(7).to(qkv.device).reshape(-1)].reshape(49, 49, nh).permute(2, 0, 1)
    if mask is not None:
        s = (s.reshape(n_img, nW, nh, 49, 49) + mask[None, :, None]).reshape(n_img * nW, nh, 49, 49)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(n_img, nW * 49, C)
    out = torch.empty(n_img, H * H, C, dtype=o.dtype, device=o.device)
    out[:, idx.reshape(-1)] = o
    return out.reshape(-1, C)


@DTYPES
@pytest.mark.parametrize("geom", [(2, 14, 96, 3, 0), (2, 14, 96, 3, 3), (1, 7, 768, 24, 0)], ids=lambda g: "n%d-H%d-C%d-h%d-s%d" % g)
def test_window_attention_with_a_steep_position_table(dev, dtype, geom):
    """ops.window_attn_core (csrc/wattn_mfma.hip in bf16, csrc/attn.hip in fp32; backward csrc/wattn_bwd_ref.hip / attn.hip): relative-position table
    entries +-50 (logits 100 apart inside a row: near-one-hot, and a running max that moves by 100 between key tiles), sharp q / k on top, with and
    without the SW-MSA mask"""
    from oracle import swin as OS
    n_img, H, C, nh, shift = geom
    base = ATTN_BASE[dtype]
    index = OS.relative_position_index(7).to(dev).int().contiguous()
    failures = []
    for score in ("unit", "sharp"):
        for mis in ((False, True) if shift else (False,)):
            qkv = V.randn((n_img * H * H, 3 * C), 110) * (math.sqrt(30.0) if score == "sharp" else 1.0)
            qkv[:, 2 * C:] = V.randn((n_img * H * H, C), 111)
            qkv = qkv.to(dtype)
            table = 50.0 * torch.sign(V.randn((169, nh), 112))
            mask = OS.shift_mask(H, H, 7, shift) if shift else None
            dy = V.randn((n_img * H * H, C), 113).to(dtype)
            qd, td = _leaf(qkv, dev), _leaf(table, dev)
            md = mask.to(dev) if mask is not None else None
            out = ops.window_attn_core(qd, td, index, md, n_img, H, H, nh, shift, 32 ** -0.5, mis)
            dq, dt_ = torch.autograd.grad(out, [qd, td], dy.to(dev))
            q64, t64 = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
            ref = _wattn_ref(q64, t64, mask.double() if mask is not None else None, n_img, H, C, nh, shift)
            rq, rt = torch.autograd.grad(ref, [q64, t64], dy.double())
            qs, ts = _leaf(qkv, dev), _leaf(table, dev, dtype)
            st = _wattn_ref(qs, ts, md.to(dtype) if md is not None else None, n_img, H, C, nh, shift)
            sq, stt = torch.autograd.grad(st, [qs, ts], dy.to(dev))
            tag = f"wattn {str(dtype)[6:]} n{n_img} H{H} C{C} s{shift} std{int(mis)} {score}"
            bad = [n for n, t in dict(out=out, dqkv=dq, dtable=dt_).items() if not bool(torch.isfinite(t.float()).all())]
            if bad:
                failures.append(f"{tag}: non-finite {bad}")
            V.judge(tag, {"out": V.rel_err(out, ref)}, {"out": V.rel_err(st, ref)}, base, failures)                # base: t_wattn forward
            V.judge(tag, {"dqkv": V.rel_err(dq, rq), "dtable": V.rel_err(dt_, rt)}, {"dqkv": V.rel_err(sq, rq), "dtable": V.rel_err(stt, rt)}, 2 * base, failures)
    assert not failures, failures


# ====================================================================================================================== softmax: loss and head logits
@DTYPES
@pytest.mark.parametrize("B", [1, 5])
def test_ce_loss_logit_classes(dev, dtype, B):
    """ops.ce_loss (csrc/ce_loss.hip) with class weights and label smoothing on: logits +-1e4, one class ahead by 100, all classes equal"""
    NL, eps, dloss = 7, 0.1, 0.37
    w = torch.linspace(0.2, 3.0, NL)
    floor = 2e-6                                                                 # tests/test_gpu_ce_loss.py FLOOR; d(logits) in bf16: + one rounding (BF16_ROUNDING)
    failures = []
    for kind in V.LOGIT_KINDS:
        x32, y = V.logits(kind, B, NL, seed=120 + B)
        x = x32.to(dtype)
        xd = _leaf(x, dev)
        loss = ops.ce_loss(xd, y.to(dev), w.to(dev), eps)
        (g,) = torch.autograd.grad(loss * dloss, xd)
        x64 = x.double().requires_grad_(True)
        lr = F.cross_entropy(x64, y, weight=w.double(), label_smoothing=eps)
        (gr,) = torch.autograd.grad(lr * dloss, x64)
        xs = _leaf(x, dev)
        ls = F.cross_entropy(xs, y.to(dev), weight=w.to(dev).to(dtype), label_smoothing=eps)
        (gs,) = torch.autograd.grad(ls * dloss, xs)
        tag = f"ce_loss {str(dtype)[6:]} B={B} {kind}"
        if not (bool(torch.isfinite(loss)) and bool(torch.isfinite(g.float()).all())):
            failures.append(f"{tag}: non-finite")
        V.judge(tag, {"loss": V.rel_err(loss, lr)}, {"loss": V.rel_err(ls, lr)}, floor, failures)
        V.judge(tag, {"dlogits": V.rel_err(g, gr)}, {"dlogits": V.rel_err(gs, gr)}, floor + (BF16_STEP if dtype == BF16 else 0.0), failures)
    assert not failures, failures


def _head64(feats, w1, b1, w2, b2, tau):
    h = torch.relu(feats.double() @ w1.double().t() + b1.double())
    p = torch.softmax((h @ w2.double().t() + b2.double()) / tau, dim=1)
    return p, (p * p).sum(1)


def _head_case(kind, N, dtype, seed):
    NL = 7
    feats = (V.randn((N, 512), seed) * 1.5).to(dtype)
    w1, b1 = V.randn((64, 512), seed + 1) * 512 ** -0.5, V.randn((64,), seed + 2) * 0.1
    w2, b2 = V.randn((NL, 64), seed + 3) * 0.5, V.randn((NL,), seed + 4) * 0.1
    if kind == "pm1e4":
        b2 = b2 + torch.tensor([1e4, -1e4] * 4)[:NL]
    elif kind == "ahead100":
        b2[3] += 100.0
    elif kind == "equal":
        w2, b2 = torch.zeros_like(w2), torch.full((NL,), 3.0)
    return feats, w1, b1, w2, b2


@DTYPES
@pytest.mark.parametrize("N", [1, 5])
def test_emotion_head_logit_classes(dev, dtype, N):
    """ops.emotion_head_raw (csrc/eval.hip): the class logits +-1e4, one ahead by 100, all equal (through the classifier's bias), tau 1 and 0.5"""
    failures = []
    for kind in V.LOGIT_KINDS:
        for tau in (1.0, 0.5):
            feats, w1, b1, w2, b2 = _head_case(kind, N, dtype, 130 + N)
            with torch.no_grad():
                preds, imp = ops.emotion_head_raw(feats.to(dev), w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev), tau)
            want, want_imp = _head64(feats, w1, b1, w2, b2, tau)
            fs = feats.to(dev).float()
            hs = torch.relu(fs @ w1.to(dev).t() + b1.to(dev))
            ps = torch.softmax((hs @ w2.to(dev).t() + b2.to(dev)) / tau, dim=1)
            tag = f"emotion_head {str(dtype)[6:]} N={N} {kind} tau={tau}"
            if not (bool(torch.isfinite(preds).all()) and bool(torch.isfinite(imp).all())):
                failures.append(f"{tag}: non-finite")
            V.judge(tag, {"preds": V.rel_err(preds, want), "importance": V.rel_err(imp, want_imp)},
                    {"preds": V.rel_err(ps, want), "importance": V.rel_err((ps * ps).sum(1), want_imp)}, 1e-3, failures)      # base: tests/test_gpu_eval_step.py
            if kind == "equal" and not torch.equal(preds.cpu(), torch.full((N, 7), 1.0 / 7)):
                failures.append(f"{tag}: equal logits must give exactly 1/7")
    assert not failures, failures


# ====================================================================================================================== GELU beyond +-8
FAR = (8.5, 20.0, 1e3, 1e30)


def _far_sweep(M, N, dtype, dev):
    vals = torch.tensor([s * v for v in FAR for s in (1.0, -1.0)]).to(dtype)
    idx = (torch.arange(N)[None, :] + torch.arange(M)[:, None] * 7) % len(vals)
    return vals[idx].to(dev).contiguous()


def _check_far(name, got, x, positive_is, failures):
    """positive x: exactly `positive_is` (x itself for gelu, 1 for gelu'); negative x: <= 0 and |.| <= 1e-15"""
    got, x = got.float(), x.float()
    pos, neg = x > 0, x < 0
    want = x[pos] if positive_is == "x" else torch.ones_like(x[pos])
    if not bool(torch.isfinite(got).all()):
        failures.append(f"{name}: non-finite")
    elif not torch.equal(got[pos], want):
        failures.append(f"{name}: positive side off by {float((got[pos] - want).abs().max()):.3e}")
    elif not (float(got[neg].max()) <= 0.0 and float(got[neg].abs().max()) <= 1e-15):
        failures.append(f"{name}: negative side max {float(got[neg].max()):.3e}, |.| {float(got[neg].abs().max()):.3e}")


@DTYPES
def test_gelu_epilogues_beyond_the_sweep(dev, dtype):
    """the few-token GEMM epilogues at (300, 384) on +-{8.5, 20, 1e3, 1e30} through identity weights: EPI_GELU, _DG, _BWD, MUL_AUX"""
    M, N = 300, 384
    x = _far_sweep(M, N, dtype, dev)
    w = torch.eye(N, dtype=dtype, device=dev)
    ones = torch.ones((M, N), dtype=dtype, device=dev)
    failures = []
    ypre = torch.empty_like(x)
    y = ops.linear_raw(x, w, None, epi=EPI_GELU, y_pre=ypre)
    assert torch.equal(ypre, x)
    _check_far("EPI_GELU", y, x, "x", failures)
    _check_far("EPI_GELU_BWD", ops.linear_raw(ones, w, None, epi=EPI_GELU_BWD, aux=x), x, "1", failures)
    ydg = torch.empty_like(x)
    y = ops.linear_raw(x, w, None, epi=EPI_GELU_DG, y_pre=ydg)
    _check_far("EPI_GELU_DG value", y, x, "x", failures)
    _check_far("EPI_GELU_DG derivative", ydg, x, "1", failures)
    _check_far("EPI_MUL_AUX on the stored derivative", ops.linear_raw(ones, w, None, epi=EPI_MUL_AUX, aux=ydg), x, "1", failures)
    assert not failures, failures


@pytest.mark.parametrize("C", [96, 192])
def test_fused_mlp_gelu_beyond_the_sweep(dev, C):
    """the fused Mlp forward (activation, stored derivative) and input-gradient kernels at (4096, C), bf16, stacked-identity fc1 as in t_gelu_tail"""
    M, dtype = 4096, BF16
    x = _far_sweep(M, C, dtype, dev)
    w1 = torch.eye(C, dtype=dtype, device=dev).repeat(4, 1).contiguous()
    b1, b2 = torch.zeros(4 * C, device=dev), torch.zeros(C, device=dev)
    w2 = torch.zeros((C, 4 * C), dtype=dtype, device=dev)
    xx = x.repeat(1, 4).contiguous()
    failures = []
    hp, ha = torch.empty((M, 4 * C), dtype=dtype, device=dev), torch.empty((M, 4 * C), dtype=dtype, device=dev)
    ops.mlp_fused_raw(x, w1, b1, w2, b2, None, None, 49, hp, ha)
    assert torch.equal(hp, xx)
    _check_far(f"mlp fwd activation C={C}", ha, xx, "x", failures)
    hd, ha2 = torch.empty_like(hp), torch.empty_like(hp)
    ops.mlp_fused_raw(x, w1, b1, w2, b2, None, None, 49, hd, ha2, dg=True)
    _check_far(f"mlp fwd activation (dg) C={C}", ha2, xx, "x", failures)
    _check_far(f"mlp fwd stored derivative C={C}", hd, xx, "1", failures)
    dy = torch.zeros((M, C), dtype=dtype, device=dev)
    dy[:, 0] = 1.0
    w2b = torch.zeros((C, 4 * C), dtype=dtype, device=dev)
    w2b[0] = 1.0
    dh, _ = ops.mlp_bwd_input_raw(dy, xx, w1, w2b, None, 49)
    _check_far(f"mlp bwd gelu' C={C}", dh, xx, "1", failures)
    dh2, _ = ops.mlp_bwd_input_raw(dy, hd, w1, w2b, None, 49, dg=True)
    _check_far(f"mlp bwd stored gelu' C={C}", dh2, xx, "1", failures)
    assert not failures, failures


# ====================================================================================================================== non-finite footprint
POISONS = [float("nan"), float("inf")]


def _footprint(name, clean, dirty, dep, failures, require=None):
    """dep: bool mask (broadcastable) of the elements that depend on the poisoned input.  `require` (default dep): those that must be non-finite;
    elements in dep but not in require are not judged.  Everything outside dep: the clean bits."""
    clean, dirty = clean.detach(), dirty.detach()
    dep = dep.to(clean.device).expand(clean.shape)
    require = dep if require is None else require.to(clean.device).expand(clean.shape)
    fin = torch.isfinite(dirty.float())
    if bool((fin & require).any()):
        failures.append(f"{name}: {int((fin & require).sum())} of {int(require.sum())} dependent elements came out finite")
    same = (clean == dirty) | (torch.isnan(clean.float()) & torch.isnan(dirty.float()))
    if bool((~same & ~dep).any()):
        failures.append(f"{name}: {int((~same & ~dep).sum())} independent elements changed")


def _rowmask(shape, r, dev):
    m = torch.zeros(shape, dtype=torch.bool, device=dev)
    m[r] = True
    return m


@DTYPES
@pytest.mark.parametrize("C", [96, 768])
def test_footprint_layer_norm(dev, dtype, C):
    M, r0, c0 = 66, 37, C - 3
    x, g, b, dy, _, _ = _norm_case(M, C, dtype, seed=140, classes=("unit",))
    failures = []

    def run(xv):
        xd, gd, bd = _leaf(xv, dev), _leaf(g, dev), _leaf(b, dev)
        y = ops.layer_norm(xd, gd, bd, EPS)
        return (y,) + torch.autograd.grad(y, [xd, gd, bd], dy.to(dev))
    clean = run(x)
    for p in POISONS:
        xp = x.clone()
        xp[r0, c0] = p
        y, dx, dg, db = run(xp)
        row = _rowmask((M, 1), r0, dev)
        tag = f"layer_norm {dtype} C={C} x[{r0},{c0}]={p}"
        _footprint(f"{tag} y", clean[0], y, row, failures)
        _footprint(f"{tag} dx", clean[1], dx, row, failures)
        _footprint(f"{tag} dgamma", clean[2], dg, torch.ones(C, dtype=torch.bool), failures)
        _footprint(f"{tag} dbeta", clean[3], db, torch.zeros(C, dtype=torch.bool), failures)         # the column sum of dy: no x in it
    assert not failures, failures


@DTYPES
def test_footprint_gemm_epilogues(dev, dtype):
    """fmmt_linear_fwd at (300, 384, 96), every epilogue: x[r, k] reaches row r, w[n, k] and bias[n] column n, aux[r, n] and res[r, n] that element"""
    M, N, K, r0, n0, k0 = 300, 384, 96, 201, 77, 5
    x = V.randn((M, K), 150).to(dtype).to(dev)
    w = (V.randn((N, K), 151) * K ** -0.5).to(dtype).to(dev)
    bias = (V.randn((N,), 152) * 0.1).to(dev)
    aux = V.randn((M, N), 153).to(dtype).to(dev)
    res = V.randn((M, N), 154).to(dtype).to(dev)
    failures = []

    def run(epi, x, w, aux, bias=bias, res=res):
        ypre = torch.empty((M, N), dtype=dtype, device=dev) if epi in (EPI_GELU, EPI_GELU_DG) else None
        kw = dict(res=res) if epi == EPI_NONE else {}
        y = ops.linear_raw(x, w, None if epi in (EPI_GELU_BWD, EPI_MUL_AUX) else bias, epi=epi, y_pre=ypre, aux=aux if epi in (EPI_GELU_BWD, EPI_MUL_AUX) else None, **kw)
        return y, ypre
    names = {EPI_NONE: "NONE+res", EPI_GELU: "GELU", EPI_GELU_BWD: "GELU_BWD", EPI_GELU_DG: "GELU_DG", EPI_MUL_AUX: "MUL_AUX"}
    row = _rowmask((M, 1), r0, dev)
    col = torch.zeros((1, N), dtype=torch.bool, device=dev)
    col[0, n0] = True
    one = row & col
    none = torch.zeros((1, 1), dtype=torch.bool, device=dev)
    for epi, label in names.items():
        cy, cpre = run(epi, x, w, aux)
        for p in POISONS:
            for what in ("x", "w", "aux", "bias", "res"):
                if (what == "aux") != (epi in (EPI_GELU_BWD, EPI_MUL_AUX)) and what in ("aux", "bias"):
                    continue                                                     # aux: the two backward epilogues only; they take no bias
                if what == "res" and epi != EPI_NONE:
                    continue
                xx, ww, aa = x.clone(), w.clone(), aux.clone()
                bb, rr = bias.clone(), res.clone()
                if what == "x":
                    xx[r0, k0] = p
                    dep = row
                    pre_plus = (w[:, k0] > 0)[None, :] & row                    # +inf * w[n, k0]: the pre-activation's sign
                elif what == "w":
                    ww[n0, k0] = p
                    dep = col
                    pre_plus = (x[:, k0] > 0)[:, None] & col
                elif what == "aux":
                    aa[r0, n0] = p
                    dep = one
                    pre_plus = one
                elif what == "bias":
                    bb[n0] = p
                    dep = pre_plus = col
                else:
                    rr[r0, n0] = p
                    dep = pre_plus = one
                y, ypre = run(epi, xx, ww, aa, bb, rr)
                tag = f"linear {dtype} {label} {what}={p}"
                # fp32: everything that depends on the element.  bf16: the documented exception of include/fmmt.h -- the GELU forms clamp with a maximum and
                # return gelu(NaN) ~ -1e-18, gelu'(NaN) = gelu'(+inf) = 1 (keeping the NaN cost bench time) -- so there the GELU value is required
                # non-finite only for a pre-activation of +inf, the derivative never; the stored pre-activation and everything else stay strict, and no
                # independent element may change in any case.
                req_y = req_pre = None
                if dtype == BF16:
                    if epi in (EPI_GELU, EPI_GELU_DG) and what in ("x", "w", "bias"):
                        req_y = pre_plus if math.isinf(p) else none
                        req_pre = none if epi == EPI_GELU_DG else None
                    elif epi == EPI_GELU_BWD and what == "aux":
                        req_y = none
                _footprint(f"{tag} y", cy, y, dep, failures, require=req_y)
                if ypre is not None:
                    _footprint(f"{tag} y_pre", cpre, ypre, dep, failures, require=req_pre)
    assert not failures, failures


@DTYPES
@pytest.mark.parametrize("shape", MHA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_footprint_mha_forward(dev, dtype, shape):
    """q[i, b, h, d] reaches head h of output row (i, b); k[j, b, h, d] every query of (b, h); v[j, b, h, d] channel d of head h for every query of b"""
    Lq, Lk, B, E, nh = shape
    hd, scale = E // nh, (E // nh) ** -0.5
    q, k, v = (t.to(dev) for t in V.mha_inputs("unit", Lq, Lk, B, E, nh, dtype, seed=160))
    i0, j0, b0, h0, d0 = Lq - 5, Lk - 2, 1, nh - 2, 3
    ch = h0 * hd + d0
    with torch.no_grad():
        clean = ops.mha_core(q, k, v, nh, scale)
    head = torch.zeros((Lq, B, E), dtype=torch.bool, device=dev)
    head[:, b0, h0 * hd:(h0 + 1) * hd] = True
    qdep = head.clone()
    qdep[:i0] = False
    qdep[i0 + 1:] = False
    vreq = torch.zeros_like(head)
    vreq[:, b0, ch] = True
    failures = []
    for what, poisons, dep, req in (("q", POISONS, qdep, None), ("k", POISONS[:1], head, None), ("v", POISONS, vreq, None)):
        for p in poisons:
            qq, kk, vv = q.clone(), k.clone(), v.clone()
            {"q": qq, "k": kk, "v": vv}[what][(i0 if what == "q" else j0), b0, ch] = p
            with torch.no_grad():
                out = ops.mha_core(qq, kk, vv, nh, scale)
            _footprint(f"mha {dtype} {Lq}x{Lk} {what}={p}", clean, out, dep, failures, require=req)
    assert not failures, failures


@pytest.mark.parametrize("C", [96, 192])
def test_footprint_fused_mlp(dev, C, monkeypatch):
    """the fused Mlp (bf16, M = 4096) as y = x + Mlp(x), and ops.mlp_ln, y = x + Mlp(LayerNorm(x)), with x[r, c] poisoned.  The bf16 GELU is the documented
    exception of include/fmmt.h (gelu(NaN) is finite), so the property is held where it still holds: the stored pre-activation row is non-finite, the
    residual carries the poisoned element into y[r, c] (the next LayerNorm spreads it over the row), +inf reaches the whole row of y through gelu(+inf) = +inf;
    and no other row changes a bit."""
    monkeypatch.setattr(ops, "_MLP_FUSED_WIDTHS", (96, 192))
    M, dtype, r0, c0 = 4096, BF16, 2999, C - 1
    x = V.randn((M, C), 170).to(dtype).to(dev)
    P = {k: t.to(dev) for k, t in _mlp_ln_params(C, 171).items()}
    w1, w2 = P["w1"].to(dtype).contiguous(), P["w2"].to(dtype).contiguous()
    failures = []

    def run(xv):
        hp, ha = torch.empty((M, 4 * C), dtype=dtype, device=dev), torch.empty((M, 4 * C), dtype=dtype, device=dev)
        y = ops.mlp_fused_raw(xv, w1, P["b1"], w2, P["b2"], xv, None, 49, hp, ha)
        hd = torch.empty_like(hp)
        y2 = ops.mlp_fused_raw(xv, w1, P["b1"], w2, P["b2"], xv, None, 49, hd, None, dg=True)
        with torch.no_grad():
            y3 = ops.mlp_ln(xv, P["g"], P["b"], EPS, P["w1"], P["b1"], P["w2"], P["b2"])
        return dict(y=y, h_pre=hp, h_act=ha, y_dg=y2, y_mlp_ln=y3)
    clean = run(x)
    row = _rowmask((M, 1), r0, dev)
    elem = torch.zeros((M, C), dtype=torch.bool, device=dev)
    elem[r0, c0] = True
    none = torch.zeros((1, 1), dtype=torch.bool, device=dev)
    plus = (w1[:, c0] > 0)[None, :] & row                                         # +inf * w1[j, c0] = +inf, and gelu(+inf) = +inf
    for p in POISONS:
        xp = x.clone()
        xp[r0, c0] = p
        inf = math.isinf(p)
        require = dict(y=None if inf else elem, h_pre=None, h_act=plus if inf else none, y_dg=None if inf else elem, y_mlp_ln=elem)
        for k_, t in run(xp).items():
            _footprint(f"mlp C={C} x={p} {k_}", clean[k_], t, row, failures, require=require[k_])
    assert not failures, failures


@DTYPES
def test_footprint_emotion_head_and_ce_loss(dev, dtype):
    """a poisoned feature reaches its row of the head's probabilities and its importance score (relu(NaN) is NaN); a poisoned logit reaches the loss"""
    N, r0 = 21, 17
    feats, w1, b1, w2, b2 = (t.to(dev) for t in _head_case("unit", N, dtype, 180))
    failures = []
    with torch.no_grad():
        cp, ci = ops.emotion_head_raw(feats, w1, b1, w2, b2, 1.0)
    row = _rowmask((N, 1), r0, dev)
    for p in POISONS:
        f = feats.clone()
        f[r0, 300] = p
        with torch.no_grad():
            preds, imp = ops.emotion_head_raw(f, w1, b1, w2, b2, 1.0)
        _footprint(f"emotion_head {dtype} feats={p} preds", cp, preds, row, failures)
        _footprint(f"emotion_head {dtype} feats={p} importance", ci, imp, row.reshape(N), failures)
    x, y = V.logits("unit", 5, 7, seed=181)
    w = torch.linspace(0.2, 3.0, 7).to(dev)
    for p in POISONS:
        for c in range(7):
            xp = x.clone()
            xp[3, c] = p
            xd = _leaf(xp, dev, dtype)
            loss = ops.ce_loss(xd, y.to(dev), w, 0.1)
            (g,) = torch.autograd.grad(loss, xd)
            if bool(torch.isfinite(loss)):
                failures.append(f"ce_loss {dtype} logits[3,{c}]={p}: loss {float(loss)} is finite")
            if bool(torch.isfinite(g[3].float()).all()):
                failures.append(f"ce_loss {dtype} logits[3,{c}]={p}: d(logits) of the poisoned row is finite")
    assert not failures, failures


# ====================================================================================================================== more call sites of the same statistics / softmax
def _self_qkv(kind, S, B, E, nh, dtype, seed):
    """batch-major packed projection (B, S, 3E) = [q | k | v] of the score class, and its time-major parts"""
    q, k, v = V.mha_inputs(kind, S, S, B, E, nh, dtype, seed=seed)
    return torch.cat([t.transpose(0, 1) for t in (q, k, v)], -1).contiguous(), (q, k, v)


def test_batch_major_self_attention_score_classes(dev):
    """the text encoder's attention (ops.PlmSelfAttnFn's two launches, fmmt_mha_fwd / _bwd with FMMT_BATCH_MAJOR on the packed projection): S 130, E 1024,
    16 heads, bf16"""
    S, B, E, nh, dtype = 130, 2, 1024, 16, BF16
    scale, base = (E // nh) ** -0.5, ATTN_BASE[dtype]
    failures = []
    for score, bias in MHA_CASES:
        qkv, (q, k, v) = _self_qkv(score, S, B, E, nh, dtype, 200)
        kb = V.key_bias(bias, B, S, seed=200) if bias else None
        dy = V.randn((B, S, E), 204).to(dtype)
        kbd = kb.to(dev).contiguous() if kb is not None else None
        qd = qkv.to(dev)
        out, lse = ops.mha_packed_bm_fwd_raw(qd, nh, scale, 0.0, 0, None, kbd)
        d = ops.mha_packed_bm_bwd_raw(qd, out, dy.to(dev), lse, nh, scale, 0.0, 0, None, kbd)
        q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
        ref = V.attention(q64, k64, v64, nh, scale, kb)
        rgrads = torch.autograd.grad(ref, [q64, k64, v64], dy.double().transpose(0, 1))
        qs, ks, vs = _leaf(q, dev), _leaf(k, dev), _leaf(v, dev)
        st = V.attention(qs, ks, vs, nh, scale, kbd)
        sgrads = torch.autograd.grad(st, [qs, ks, vs], dy.to(dev).transpose(0, 1))
        tag = f"mha batch-major bf16 S{S} E{E} {score} {bias or '-'}"
        if not (bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(d.float()).all())):
            failures.append(f"{tag}: non-finite")
        tm = lambda t: t.transpose(0, 1)
        V.judge(tag, {"out": V.rel_err(tm(out), ref)}, {"out": V.rel_err(st, ref)}, base, failures)                 # base: t_mha
        V.judge(tag, {n: V.rel_err(tm(d[..., i * E:(i + 1) * E]), rgrads[i]) for i, n in enumerate(("dq", "dk", "dv"))},
                {n: V.rel_err(sgrads[i], rgrads[i]) for i, n in enumerate(("dq", "dk", "dv"))}, 2 * base, failures)
    assert not failures, failures


def test_ragged_self_attention_score_classes(dev):
    """ops.mha_ragged_fwd_raw / _bwd_raw on packed rows of lengths [70, 130, 1]: each sequence against its own fp64 attention"""
    T, lens, E, nh, dtype = 130, (70, 130, 1), 1024, 16, BF16
    B, total = len(lens), sum(lens)
    cap, scale, base = total + 5, (E // nh) ** -0.5, ATTN_BASE[dtype]
    mask = torch.zeros(B, T)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    real = mask.bool()
    lay = ops.token_layout_raw(mask.to(dev), cap)
    assert lay.seq_len.tolist() == list(lens)
    failures = []
    for score in V.SCORE_KINDS:
        qkv, (q, k, v) = _self_qkv(score, T, B, E, nh, dtype, 210)
        dy = V.randn((B, T, E), 214).to(dtype)
        filler = lambda w: torch.full((cap - total, w), 3.0e4, dtype=dtype)
        qkv_p = torch.cat([qkv[real], filler(3 * E)]).contiguous().to(dev)
        dy_p = torch.cat([dy[real], filler(E)]).contiguous().to(dev)
        out, lse = ops.mha_ragged_fwd_raw(qkv_p, lay, nh, scale, 0.0, 0, None)
        d = ops.mha_ragged_bwd_raw(qkv_p, lay, out, dy_p, lse, nh, scale, 0.0, 0, None)
        if not (bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(d.float()).all())):
            failures.append(f"ragged {score}: non-finite")
        off = 0
        for b, n in enumerate(lens):
            parts = [t[:n, b:b + 1] for t in (q, k, v)]
            p64 = [t.double().requires_grad_(True) for t in parts]
            ref = V.attention(*p64, nh, scale)
            rg = torch.autograd.grad(ref, p64, dy[b, :n].double()[:, None])
            ps = [_leaf(t, dev) for t in parts]
            st = V.attention(*ps, nh, scale)
            sg = torch.autograd.grad(st, ps, dy[b, :n].to(dev)[:, None])
            tag = f"mha ragged bf16 len {n} {score}"
            rows = slice(off, off + n)
            V.judge(tag, {"out": V.rel_err(out[rows], ref[:, 0])}, {"out": V.rel_err(st[:, 0], ref[:, 0])}, base, failures)            # base: t_mha
            if n > 1:
                V.judge(tag, {nm: V.rel_err(d[rows, i * E:(i + 1) * E], rg[i][:, 0]) for i, nm in enumerate(("dq", "dk", "dv"))},
                        {nm: V.rel_err(sg[i][:, 0], rg[i][:, 0]) for i, nm in enumerate(("dq", "dk", "dv"))}, 2 * base, failures)
            elif not float(d[rows, :2 * E].float().abs().max()) <= 1e-5:      # a single key: dq = dk = 0 absolutely (t_mha's Lk = 1 check)
                failures.append(f"{tag}: |dq|, |dk| = {float(d[rows, :2 * E].float().abs().max()):.3e} > 1e-5")
            off += n
    assert not failures, failures


def _wblock_params(C, nh, seed, steep):
    P = dict(g=V.randn((C,), seed + 1) * 0.2 + 1, b=V.randn((C,), seed + 2) * 0.1, wqkv=V.randn((3 * C, C), seed + 3) * C ** -0.5, bqkv=V.randn((3 * C,), seed + 4) * 0.1,
             wproj=V.randn((C, C), seed + 5) * C ** -0.5, bproj=V.randn((C,), seed + 6) * 0.1, table=V.randn((169, nh), seed + 7) * 0.5)
    if steep:
        P["table"] = 50.0 * torch.sign(P["table"])
    return P


def _wblock_ref(x, P, mask, n_img, H, nh, shift):
    C = x.shape[-1]
    xn = F.layer_norm(x, (C,), P["g"], P["b"], EPS)
    qkv = xn.reshape(-1, C) @ P["wqkv"].t() + P["bqkv"]
    o = _wattn_ref(qkv, P["table"], mask, n_img, H, C, nh, shift)
    return x.reshape(-1, C) + (o @ P["wproj"].t() + P["bproj"])


@DTYPES
@pytest.mark.parametrize("steep", [False, True], ids=["smooth-table", "steep-table"])
@pytest.mark.parametrize("shift", [0, 3])
def test_window_block_row_classes(dev, dtype, shift, steep):
    """ops.window_block (LayerNorm + qkv + window attention + proj + residual in one launch: csrc/wblock.hip in bf16, csrc/wblock_ref.hip in fp32; backward
    through csrc/lin_lnbwd.hip) at n_img 2, 14 x 14, C 96: the row classes on the tokens (its LayerNorm statistics), and a position table of +-50 (its
    softmax).  Without `big` (x + branch loses the branch) and `const1024` (its x-hat is 0 +- const_row_bound, and a window shares keys and values).
    Judged: the branch y - x per class of the query token, d(x) - dy likewise, every parameter gradient."""
    from oracle import swin as OS
    n_img, H, C, nh = 2, 14, 96, 3
    classes = ("unit", "offset", "outlier", "tiny", "const0")
    fwd, bwd = {F32: (1e-4, 1e-3), BF16: (2e-2, 4e-2)}[dtype]                    # base: tests/test_gpu_wblock.py (fp32 instantiation / bf16 block half)
    M = n_img * H * H
    x2, cls, omask = V.norm_rows(M, C, dtype, seed=220 + shift, classes=classes)
    x = x2.reshape(n_img, H * H, C)
    P = _wblock_params(C, nh, 230, steep)
    dy = V.randn((n_img, H * H, C), 227).to(dtype)
    index = OS.relative_position_index(7).to(dev).int().contiguous()
    mask = OS.shift_mask(H, H, 7, shift) if shift else None
    md = mask.to(dev) if mask is not None else None
    xd = _leaf(x, dev)
    Pd = {k: _leaf(v, dev) for k, v in P.items()}
    assert ops.window_block_fusable(xd, C, nh, (7, 7), shift, md, md is not None)
    y = ops.window_block(xd, Pd["g"], Pd["b"], EPS, Pd["wqkv"], Pd["bqkv"], Pd["wproj"], Pd["bproj"], Pd["table"], index, md, n_img, H, H, nh, shift, 32 ** -0.5)
    names = ["g", "b", "wqkv", "bqkv", "wproj", "bproj", "table"]
    grads = torch.autograd.grad(y, [xd] + [Pd[k] for k in names], dy.to(dev))
    x64 = x.double().requires_grad_(True)
    P64 = {k: (v.to(dtype).double() if k in ("wqkv", "wproj") else v.double()).requires_grad_(True) for k, v in P.items()}
    yr = _wblock_ref(x64, P64, mask.double() if mask is not None else None, n_img, H, nh, shift)
    gref = torch.autograd.grad(yr, [x64] + [P64[k] for k in names], dy.double().reshape(-1, C))
    xs = _leaf(x, dev)
    Ps = {k: _leaf(v, dev, dtype) for k, v in P.items()}
    ys = _wblock_ref(xs, Ps, md.to(dtype) if md is not None else None, n_img, H, nh, shift)
    gst = torch.autograd.grad(ys, [xs] + [Ps[k] for k in names], dy.to(dev).reshape(-1, C))
    _finite(y=y, **{"d" + k: t for k, t in zip(["x"] + names, grads)})
    failures = []
    tag = f"window_block {str(dtype)[6:]} s{shift} {'steep' if steep else 'smooth'}"
    sub = lambda t: t.detach().cpu().double().reshape(M, C) - x2.double()
    V.judge(f"{tag} y - x", V.class_errors(sub(y), sub(yr), cls, classes, omask), V.class_errors(sub(ys), sub(yr), cls, classes, omask), fwd, failures)
    d1 = lambda t: t.detach().cpu().double().reshape(M, C) - dy.double().reshape(M, C)
    V.judge(f"{tag} dx - dy", V.class_errors(d1(grads[0]), d1(gref[0]), cls, classes, omask), V.class_errors(d1(gst[0]), d1(gref[0]), cls, classes, omask), bwd, failures)
    V.judge(f"{tag} dparam", {"d" + k: V.rel_err(a, r) for k, a, r in zip(names, grads[1:], gref[1:])},
            {"d" + k: V.rel_err(s, r) for k, s, r in zip(names, gst[1:], gref[1:])}, bwd, failures)
    assert not failures, failures


# The row offset the patch kernels get through the projection's bias.  fp32: 1000, as the `offset` rows.  bf16: the kernel rounds acc + bias to bf16
# BEFORE the statistics, on purpose (csrc/patch_ln_core.h: the backward re-reads those rounded rows), so its LayerNorm operand is a bf16 tensor and the
# rule for bf16 operands holds -- an offset the format carries without losing the spread: at 8 the bf16 step is 2^-4, a sixteenth of the rows' unit
# spread.  (At 1000 the step is 4 .. 8: the operand's spread is gone in any bf16 LayerNorm, this kernel's and the stock one's alike -- measured once,
# both were wrong by 50 % .. 1000 % of the scale, and their ratio is then chance.)
PATCH_OFFSET = {F32: 1000.0, BF16: 8.0}


@DTYPES
@pytest.mark.parametrize("large", [False, True], ids=["small-bias", "large-bias"])
def test_patch_proj_ln_offset_through_the_bias(dev, dtype, large):
    """ops.patch_proj_ln (LayerNorm(cols W^T + b) of PatchEmbed in one launch, csrc/patch_ln.hip) on one 224 x 224 image: the LayerNorm operand exists in
    fp32 only inside the kernel, so a row offset of 1000 reaches it through the projection's bias"""
    M, K, C = 3136, 48, 96
    offset = PATCH_OFFSET[dtype] if large else 0.0
    fwd, bwd = {F32: (1e-5, 1e-4), BF16: (2e-2, 4e-2)}[dtype]                    # base: tests/test_gpu_wblock.py (patch embed: fp32 instantiation / bf16)
    cols = V.randn((M, K), 240).to(dtype)
    P = dict(w=V.randn((C, K), 241) * K ** -0.5, bias=offset + V.randn((C,), 242), g=V.randn((C,), 243) * 0.2 + 1, b=V.randn((C,), 244) * 0.1)
    dy = V.randn((M, C), 245).to(dtype)
    cd = _leaf(cols, dev)
    Pd = {k: _leaf(v, dev) for k, v in P.items()}
    y = ops.patch_proj_ln(cd, Pd["w"], Pd["bias"], Pd["g"], Pd["b"], EPS)
    names = ["w", "bias", "g", "b"]
    grads = torch.autograd.grad(y, [cd] + [Pd[k] for k in names], dy.to(dev))
    ref_of = lambda c, Q: F.layer_norm(c @ Q["w"].t() + Q["bias"], (C,), Q["g"], Q["b"], EPS)
    c64 = cols.double().requires_grad_(True)
    P64 = {k: (v.to(dtype).double() if k == "w" else v.double()).requires_grad_(True) for k, v in P.items()}
    yr = ref_of(c64, P64)
    gref = torch.autograd.grad(yr, [c64] + [P64[k] for k in names], dy.double())
    cs = _leaf(cols, dev)
    Ps = {k: _leaf(v, dev, dtype) for k, v in P.items()}
    ys = ref_of(cs, Ps)
    gst = torch.autograd.grad(ys, [cs] + [Ps[k] for k in names], dy.to(dev))
    _finite(y=y, **{"d" + k: t for k, t in zip(["cols"] + names, grads)})
    failures = []
    tag = f"patch_proj_ln {str(dtype)[6:]} bias {offset:g}"
    V.judge(tag, {"y": V.rel_err(y, yr)}, {"y": V.rel_err(ys, yr)}, fwd, failures)
    V.judge(tag, {"d" + k: V.rel_err(a, r) for k, a, r in zip(["cols"] + names, grads, gref)},
            {"d" + k: V.rel_err(s, r) for k, s, r in zip(["cols"] + names, gst, gref)}, bwd, failures)
    assert not failures, failures


def _pool_head_stock(d, dtype, dloss):
    """the head as stock torch ops in `dtype` on the device: tanh, masked softmax over tokens, weighted sum, Linear, cross-entropy"""
    t = {k: v.detach().to(dtype).requires_grad_(True) for k, v in d.items() if k not in ("mask", "labels")}
    score = torch.tanh(t["ph"] + t["qq"]) @ t["value_w"].reshape(-1) + t["value_b"]
    alpha = torch.softmax(score.masked_fill(d["mask"] == 0, float("-inf")), -1)
    logits = torch.einsum("bt,bth->bh", alpha, t["h"]) @ t["cls_w"].t() + t["cls_b"]
    loss = F.cross_entropy(logits, d["labels"])
    names = ("h", "ph", "qq", "value_w", "cls_w", "cls_b")
    g = dict(zip(names, torch.autograd.grad(loss * dloss, [t[k] for k in names])))
    return dict(loss=loss.detach(), logits=logits.detach(), alpha=alpha.detach(), dh=g["h"], dph=g["ph"], dqq=g["qq"], dv=g["value_w"].reshape(-1), dW=g["cls_w"], db=g["cls_b"])


@DTYPES
@pytest.mark.parametrize("B", [1, 5])
def test_pool_head_single_live_token_and_logit_classes(dev, dtype, B):
    """ops.pool_head_loss (csrc/pool_head.hip: masked softmax over tokens, classifier, cross-entropy): every token masked but one -- at the last
    position, behind whole waves of masked ones, at the first, in the middle -- beside a fully valid row, and the class logits +-1e4, one ahead by 100,
    all equal through the classifier's bias"""
    from tests import support_unimodal_oracle as UO
    L, H, NL, dloss = 160, 768, 7, 0.37
    fwd, bwd = {F32: (1e-3, 1e-3), BF16: (2e-2, 4e-2)}[dtype]                    # base: tests/test_gpu_pool_head.py BARS
    live = [L - 1, 0, 77, 130]
    failures = []
    for kind in V.LOGIT_KINDS:
        cpu, _ = UO.head_inputs(B, L, H, NL, 250)
        mask = torch.ones(B, L)
        single = list(range(B)) if B == 1 else list(range(1, B))
        for i, b_ in enumerate(single):
            mask[b_] = 0
            mask[b_, live[i % len(live)]] = 1
        cpu["mask"] = mask
        if kind == "pm1e4":
            cpu["cls_b"] = cpu["cls_b"] + torch.tensor([1e4, -1e4] * 4)[:NL]
        elif kind == "ahead100":
            cpu["cls_b"][3] += 100.0
        elif kind == "equal":
            cpu["cls_w"], cpu["cls_b"] = torch.zeros_like(cpu["cls_w"]), torch.full((NL,), 3.0)
        cpu["h"], cpu["ph"] = cpu["h"].to(dtype).float(), cpu["ph"].to(dtype).float()
        d = {k: v.to(dev) for k, v in cpu.items()}
        d["h"], d["ph"] = d["h"].to(dtype).requires_grad_(True), d["ph"].to(dtype).requires_grad_(True)
        d["value_w"] = d["value_w"].reshape(1, H)
        for k in ("qq", "value_w", "value_b", "cls_w", "cls_b"):
            d[k].requires_grad_(True)
        loss, logits = ops.pool_head_loss(d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"], 0.0, 0)
        (loss * dloss).backward()
        with torch.no_grad():
            alpha = ops.pool_head_fwd_raw(d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"], 0.0, 0)[2]
        got = dict(loss=loss.detach(), logits=logits, alpha=alpha, dh=d["h"].grad, dph=d["ph"].grad, dqq=d["qq"].grad, dv=d["value_w"].grad.reshape(-1),
                   dW=d["cls_w"].grad, db=d["cls_b"].grad)
        ref = UO.head_reference(**cpu, keep=torch.ones(B, H), dloss=dloss)
        stock = _pool_head_stock(d, dtype, dloss)
        tag = f"pool_head {str(dtype)[6:]} B={B} {kind}"
        bad = [k for k, t in got.items() if not bool(torch.isfinite(t.float()).all())]
        if bad:
            failures.append(f"{tag}: non-finite {bad}")
        grads = ("dh", "dph", "dqq", "dv", "dW", "db")
        if len(single) == B:
            # every row has one live token: d(score) = alpha (d(pooled) . h_t - d(pooled) . pooled) is identically 0 (pooled IS h_t), and with it dph, dqq
            # and dv -- the fp64 reference holds only its own rounding there, nothing to scale by.  A cancelling difference is judged against its
            # summands (tests/test_gpu_pool_head.py does so for d(v_b)): |d(score)| <= bar * sum_h |d(pooled)_h h_th|, times max|v| for dph and dqq
            # (|1 - tanh^2| <= 1), times 1 for dv (|tanh| <= 1).  d(pooled) of a row is its dh at the live token.
            grads = ("dh", "dW", "db")
            S = max(float((ref["dh"][b_, live[i % len(live)]] * cpu["h"][b_, live[i % len(live)]].double()).abs().sum()) for i, b_ in enumerate(single))
            vmax = float(cpu["value_w"].abs().max())
            for k, lim in (("dph", bwd * S * vmax), ("dqq", bwd * S * vmax * B), ("dv", bwd * S * B)):
                e = float(got[k].float().abs().max())
                print(f"     {tag} {k}: |got| = {e:.3e} (identically 0; bound {lim:.3e})")
                if not e <= lim:
                    failures.append(f"{tag} [{k}]: {e:.3e} > {lim:.3e} with one live token per row")
        for keys, base in ((("loss", "logits", "alpha"), fwd), (grads, bwd)):
            V.judge(tag, {k: V.rel_err(got[k].reshape(-1), ref[k].reshape(-1)) for k in keys}, {k: V.rel_err(stock[k].reshape(-1), ref[k].reshape(-1)) for k in keys},
                    base, failures)
        for i, b_ in enumerate(single):                                           # one live token: all the weight on it, exactly
            want = torch.zeros(L)
            want[live[i % len(live)]] = 1.0
            if not torch.equal(alpha[b_].float().cpu(), want):
                failures.append(f"{tag}: alpha of row {b_} is not one-hot on its live token")
    assert not failures, failures


# ====================================================================================================================== the text encoder's LayerNorm call sites (csrc/plm_fused.hip)
PLM_C, PLM_M = 1024, 128
PLM_FWD, PLM_BWD = 3e-2, 4e-2                 # tests/test_gpu_text_encoder.py: forward within 3e-2 of the scale, gradients 4e-2 (bf16 activations and parameters)


def _plm_rows(seed, classes=V.NORM_CLASSES):
    """(h, res, class_of_row, outlier mask, dy): the LayerNorm operand h + res carries the row classes; the offset rows as h = +1024 + a, res = -1024 + b
    (scale 8, rounded to bf16), the unit rows with a small residual, the constant rows with res = 0; dy = 0 on the constant rows"""
    s, cls, omask = V.norm_rows(PLM_M, PLM_C, BF16, seed=seed, classes=tuple("unit" if c == "offset" else c for c in classes))
    h, res = s.clone(), torch.zeros_like(s)
    dy = V.randn((PLM_M, PLM_C), seed + 5)
    for i, name in enumerate(classes):
        m = cls == i
        if name == "offset":
            h[m] = (1024.0 + 8.0 * V.randn((int(m.sum()), PLM_C), seed + 1)).to(BF16)
            res[m] = (-1024.0 + 8.0 * V.randn((int(m.sum()), PLM_C), seed + 2)).to(BF16)
        elif name == "unit":
            res[m] = (0.05 * V.randn((int(m.sum()), PLM_C), seed + 3)).to(BF16)
        elif name in V.CONST_CLASSES:
            dy[m] = 0.0
    return h, res, cls, omask, dy.to(BF16)


def _plm_const_rows_exact(y, beta, cls, classes):
    """C = 1024: 1 / C is exact, so a constant row gives y == beta, bit for bit, for c = 0 and for c = 1024"""
    for i, name in enumerate(classes):
        if name in V.CONST_CLASSES:
            rows = y.detach().cpu()[cls == i]
            assert torch.equal(rows, beta.to(BF16).expand_as(rows)), f"{name}: y != beta on a constant row at C = 1024"


def test_plm_sublayer_tail_row_classes(dev):
    """ops.PlmSublayerTailFn (y = LayerNorm(x W^T + b + res), fmmt_plm_dropadd_ln_fwd / _bwd) at C 1024, M 128, p 0: an identity dense layer puts x itself
    on the kernel, so the operands are exactly the classes"""
    classes = V.NORM_CLASSES
    h, res, cls, omask, dy = _plm_rows(300)
    P = dict(w=torch.eye(PLM_C), bias=torch.zeros(PLM_C), g=V.randn((PLM_C,), 306) * 0.1 + 1, b=V.randn((PLM_C,), 307) * 0.1)
    P = {k: v.to(BF16) for k, v in P.items()}
    seed = torch.tensor([4242], device=dev, dtype=torch.int64)
    names = ["w", "bias", "g", "b"]
    xd, rd = _leaf(h, dev), _leaf(res, dev)
    Pd = {k: _leaf(v, dev) for k, v in P.items()}
    y = ops.PlmSublayerTailFn.apply(xd, rd, Pd["w"], Pd["bias"], Pd["g"], Pd["b"], EPS, 0.0, seed, 7 << 40)
    grads = torch.autograd.grad(y, [xd, rd] + [Pd[k] for k in names], dy.to(dev))
    ref_of = lambda x, r, Q: F.layer_norm(x @ Q["w"].t() + Q["bias"] + r, (PLM_C,), Q["g"], Q["b"], EPS)
    x64, r64 = h.double().requires_grad_(True), res.double().requires_grad_(True)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    yr = ref_of(x64, r64, P64)
    gref = torch.autograd.grad(yr, [x64, r64] + [P64[k] for k in names], dy.double())
    xs, rs = _leaf(h, dev), _leaf(res, dev)
    Ps = {k: _leaf(v, dev) for k, v in P.items()}
    ys = ref_of(xs, rs, Ps)
    gst = torch.autograd.grad(ys, [xs, rs] + [Ps[k] for k in names], dy.to(dev))
    _finite(y=y, **{"d" + k: t for k, t in zip(["x", "res"] + names, grads)})
    failures = []
    _judge_norm("plm tail y", y, yr, ys, cls, omask, classes, PLM_FWD, failures)
    _judge_norm("plm tail dx", grads[0], gref[0], gst[0], cls, omask, classes, PLM_BWD, failures)
    _judge_norm("plm tail dres", grads[1], gref[1], gst[1], cls, omask, classes, PLM_BWD, failures)
    V.judge("plm tail dparam", {"d" + k: V.rel_err(a, r) for k, a, r in zip(names, grads[2:], gref[2:])},
            {"d" + k: V.rel_err(s, r) for k, s, r in zip(names, gst[2:], gref[2:])}, PLM_BWD, failures)
    _plm_const_rows_exact(y, P["b"], cls, classes)
    assert not failures, failures


def test_plm_ffn_row_classes(dev):
    """ops.PlmFfnFn (y = LayerNorm(gelu(x W1^T + b1) W2^T + b2 + x)) at C 1024, M 128, p 0: with W2 = 0 and b2 = 0 the LayerNorm operand is x, the row
    classes themselves (bf16 offset rows on the grid {1024, 1032, 1040}); the gradients still run the whole node.  Without `big`: 1e15 through a random
    fc1 is no LayerNorm question."""
    classes = tuple(c for c in V.NORM_CLASSES if c != "big")
    x, cls, omask = V.norm_rows(PLM_M, PLM_C, BF16, seed=310, classes=classes)
    dy = V.randn((PLM_M, PLM_C), 315)
    for i, name in enumerate(classes):
        if name in V.CONST_CLASSES:
            dy[cls == i] = 0.0
    dy = dy.to(BF16)
    P = dict(w1=V.randn((4 * PLM_C, PLM_C), 311) * 0.02, b1=V.randn((4 * PLM_C,), 312) * 0.1, w2=torch.zeros(PLM_C, 4 * PLM_C), b2=torch.zeros(PLM_C),
             g=V.randn((PLM_C,), 313) * 0.1 + 1, b=V.randn((PLM_C,), 314) * 0.1)
    P = {k: v.to(BF16) for k, v in P.items()}
    seed = torch.tensor([4243], device=dev, dtype=torch.int64)
    names = ["w1", "b1", "w2", "b2", "g", "b"]
    xd = _leaf(x, dev)
    Pd = {k: _leaf(v, dev) for k, v in P.items()}
    y = ops.PlmFfnFn.apply(xd, Pd["w1"], Pd["b1"], Pd["w2"], Pd["b2"], Pd["g"], Pd["b"], EPS, 0.0, seed, 9 << 40)
    grads = torch.autograd.grad(y, [xd] + [Pd[k] for k in names], dy.to(dev))
    ref_of = lambda t, Q: F.layer_norm(F.gelu(t @ Q["w1"].t() + Q["b1"]) @ Q["w2"].t() + Q["b2"] + t, (PLM_C,), Q["g"], Q["b"], EPS)
    x64 = x.double().requires_grad_(True)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    yr = ref_of(x64, P64)
    gref = torch.autograd.grad(yr, [x64] + [P64[k] for k in names], dy.double())
    xs = _leaf(x, dev)
    Ps = {k: _leaf(v, dev) for k, v in P.items()}
    ys = ref_of(xs, Ps)
    gst = torch.autograd.grad(ys, [xs] + [Ps[k] for k in names], dy.to(dev))
    _finite(y=y, **{"d" + k: t for k, t in zip(["x"] + names, grads)})
    failures = []
    _judge_norm("plm ffn y", y, yr, ys, cls, omask, classes, PLM_FWD, failures)
    _judge_norm("plm ffn dx", grads[0], gref[0], gst[0], cls, omask, classes, PLM_BWD, failures)
    keep = [k for k in names if k not in ("w1", "b1")]                            # W2 = 0: d(w1) and d(b1) are identically 0
    V.judge("plm ffn dparam", {"d" + k: V.rel_err(grads[1 + names.index(k)], gref[1 + names.index(k)]) for k in keep},
            {"d" + k: V.rel_err(gst[1 + names.index(k)], gref[1 + names.index(k)]) for k in keep}, PLM_BWD, failures)
    for k in ("w1", "b1"):
        if not float(grads[1 + names.index(k)].float().abs().max()) == 0.0:
            failures.append(f"plm ffn d{k}: not 0 with W2 = 0")
    _plm_const_rows_exact(y, P["b"], cls, classes)
    assert not failures, failures


def test_plm_layer_norm_backward_row_classes(dev):
    """ops.PlmLayerNormFn: torch's forward, fmmt_layernorm_bwd_bf16 backward -- which recomputes the row statistics from x in fp32 -- at C 1024, M 128"""
    classes = V.NORM_CLASSES
    x, g, b, dy, cls, omask = _norm_case(PLM_M, PLM_C, BF16, seed=320)
    g, b = g.to(BF16), b.to(BF16)
    xd, gd, bd = _leaf(x, dev), _leaf(g, dev), _leaf(b, dev)
    y = ops.PlmLayerNormFn.apply(xd, gd, bd, EPS)
    dx, dg, db = torch.autograd.grad(y, [xd, gd, bd], dy.to(dev))
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, g, b))
    yr = V.layer_norm64(x64, g64, b64, EPS)
    rx, rg, rb = torch.autograd.grad(yr, [x64, g64, b64], dy.double())
    xs, gs, bs = _leaf(x, dev), _leaf(g, dev), _leaf(b, dev)
    ys = F.layer_norm(xs, (PLM_C,), gs, bs, EPS)
    sx, sg, sb = torch.autograd.grad(ys, [xs, gs, bs], dy.to(dev))
    _finite(y=y, dx=dx, dgamma=dg, dbeta=db)
    failures = []
    _judge_norm("plm layer_norm dx", dx, rx, sx, cls, omask, classes, PLM_BWD, failures)
    V.judge("plm layer_norm dparam", {"dgamma": V.rel_err(dg, rg), "dbeta": V.rel_err(db, rb)}, {"dgamma": V.rel_err(sg, rg), "dbeta": V.rel_err(sb, rb)}, PLM_BWD, failures)
    assert not failures, failures


@DTYPES
@pytest.mark.parametrize("large", [False, True], ids=["small-bias", "large-bias"])
def test_patch_embed_u8_ln_offset_through_the_bias(dev, dtype, large):
    """ops.patch_embed_u8_ln (uint8 crop -> resize -> projection -> LayerNorm in one launch) on one image: the patch matrix of ops.patch_embed_u8
    (bit-exact against the oracle elsewhere) is the reference's input; the row offset reaches the LayerNorm through the projection's bias"""
    import numpy as np
    from facialmmt_amd import synth
    K, C = 48, 96
    offset = PATCH_OFFSET[dtype] if large else 0.0
    fwd, bwd = {F32: (1e-5, 1e-4), BF16: (2e-2, 4e-2)}[dtype]                    # base: tests/test_gpu_wblock.py (patch embed: fp32 instantiation / bf16)
    crops = torch.from_numpy(synth.randint("value_crop", (1, 112, 112, 3), 0, 256, seed=9).astype(np.uint8)).to(dev)
    cols = ops.patch_embed_u8(crops, "pil", dtype).cpu()
    M = cols.shape[0]
    P = dict(w=V.randn((C, K), 331) * K ** -0.5, bias=offset + V.randn((C,), 332), g=V.randn((C,), 333) * 0.2 + 1, b=V.randn((C,), 334) * 0.1)
    dy = V.randn((M, C), 335).to(dtype)
    names = ["w", "bias", "g", "b"]
    Pd = {k: _leaf(v, dev) for k, v in P.items()}
    y = ops.patch_embed_u8_ln(crops, "pil", Pd["w"], Pd["bias"], Pd["g"], Pd["b"], EPS, dtype)
    grads = torch.autograd.grad(y, [Pd[k] for k in names], dy.to(dev))
    ref_of = lambda c, Q: F.layer_norm(c @ Q["w"].t() + Q["bias"], (C,), Q["g"], Q["b"], EPS)
    P64 = {k: (v.to(dtype).double() if k == "w" else v.double()).requires_grad_(True) for k, v in P.items()}
    yr = ref_of(cols.double(), P64)
    gref = torch.autograd.grad(yr, [P64[k] for k in names], dy.double())
    Ps = {k: _leaf(v, dev, dtype) for k, v in P.items()}
    ys = ref_of(cols.to(dev), Ps)
    gst = torch.autograd.grad(ys, [Ps[k] for k in names], dy.to(dev))
    _finite(y=y, **{"d" + k: t for k, t in zip(names, grads)})
    failures = []
    tag = f"patch_embed_u8_ln {str(dtype)[6:]} bias {offset:g}"
    V.judge(tag, {"y": V.rel_err(y, yr)}, {"y": V.rel_err(ys, yr)}, fwd, failures)
    V.judge(tag, {"d" + k: V.rel_err(a, r) for k, a, r in zip(names, grads, gref)}, {"d" + k: V.rel_err(s, r) for k, s, r in zip(names, gst, gref)}, bwd, failures)
    assert not failures, failures


# ====================================================================================================================== further footprints and the window kernel's -inf guard
@DTYPES
def test_window_attention_with_minus_inf_mask_blocks(dev, dtype):
    """ops.window_attn_core with a mask of its own (not the SW-MSA one): -inf on the first seven keys of every query -- a whole key tile of the fp32 kernel
    (csrc/attn.hip, whose running maximum starts at -inf) -- and on scattered keys; torch.softmax is the reference.  Forward and backward."""
    from oracle import swin as OS
    n_img, H, C, nh, shift = 2, 14, 96, 3, 3
    base = ATTN_BASE[dtype]
    index = OS.relative_position_index(7).to(dev).int().contiguous()
    mask = OS.shift_mask(H, H, 7, shift).clone()
    mask[:, :, :7] = float("-inf")
    mask[:, :, 20::5] = float("-inf")
    qkv = V.randn((n_img * H * H, 3 * C), 340).to(dtype)
    table = V.randn((169, nh), 341) * 0.5
    dy = V.randn((n_img * H * H, C), 342).to(dtype)
    qd, td, md = _leaf(qkv, dev), _leaf(table, dev), mask.to(dev)
    out = ops.window_attn_core(qd, td, index, md, n_img, H, H, nh, shift, 32 ** -0.5, False)
    dq, dt_ = torch.autograd.grad(out, [qd, td], dy.to(dev))
    q64, t64 = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    ref = _wattn_ref(q64, t64, mask.double(), n_img, H, C, nh, shift)
    rq, rt = torch.autograd.grad(ref, [q64, t64], dy.double())
    qs, ts = _leaf(qkv, dev), _leaf(table, dev, dtype)
    st = _wattn_ref(qs, ts, md.to(dtype), n_img, H, C, nh, shift)
    sq, stt = torch.autograd.grad(st, [qs, ts], dy.to(dev))
    _finite(out=out, dqkv=dq, dtable=dt_)
    failures = []
    tag = f"wattn {str(dtype)[6:]} -inf mask blocks"
    V.judge(tag, {"out": V.rel_err(out, ref)}, {"out": V.rel_err(st, ref)}, base, failures)                    # base: t_wattn
    V.judge(tag, {"dqkv": V.rel_err(dq, rq), "dtable": V.rel_err(dt_, rt)}, {"dqkv": V.rel_err(sq, rq), "dtable": V.rel_err(stt, rt)}, 2 * base, failures)
    assert not failures, failures


@DTYPES
def test_footprint_pool_head(dev, dtype):
    """a poisoned h[b, t, c] or ph[b, t, c] of a valid token reaches the logits row b and the loss, and no other logits row"""
    from tests import support_unimodal_oracle as UO
    B, L, H, NL, b0, t0, c0 = 4, 160, 768, 7, 2, 5, 700
    cpu, lengths = UO.head_inputs(B, L, H, NL, 350)
    assert lengths[b0] > t0
    d = {k: v.to(dev) for k, v in cpu.items()}
    d["value_w"] = d["value_w"].reshape(1, H)

    def run(h, ph):
        with torch.no_grad():
            return ops.pool_head_fwd_raw(h.to(dtype), ph.to(dtype), d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"], 0.0, 0)[:2]
    closs, clogits = run(d["h"], d["ph"])
    assert bool(torch.isfinite(closs)) and bool(torch.isfinite(clogits).all())
    row = _rowmask((B, 1), b0, dev)
    failures = []
    for p in POISONS:
        for what in ("h", "ph"):
            if what == "ph" and math.isinf(p):
                continue                                   # tanh(+inf) = 1: a finite, legitimate score
            t = {"h": d["h"].clone(), "ph": d["ph"].clone()}
            t[what][b0, t0, c0] = p
            loss, logits = run(t["h"], t["ph"])
            tag = f"pool_head {dtype} {what}={p}"
            if bool(torch.isfinite(loss)):
                failures.append(f"{tag}: the loss {float(loss)} is finite")
            _footprint(f"{tag} logits", clogits, logits, row, failures)
    assert not failures, failures


@DTYPES
@pytest.mark.parametrize("shift", [0, 3])
def test_footprint_window_block(dev, dtype, shift):
    """ops.window_block with x[img, token, c] poisoned: the token's LayerNorm row, so its q, k and v rows, so every query of its window -- all 49 rows of
    that window of y are non-finite (the Swin block keeps the property the bf16 GELU does not); every other row keeps its bits"""
    from oracle import swin as OS
    n_img, H, C, nh, img0, tok0, c0 = 2, 14, 96, 3, 1, 100, 17
    x = V.randn((n_img, H * H, C), 360).to(dtype).to(dev)
    P = {k: v.to(dev) for k, v in _wblock_params(C, nh, 361, False).items()}
    index = OS.relative_position_index(7).to(dev).int().contiguous()
    md = OS.shift_mask(H, H, 7, shift).to(dev) if shift else None
    widx = OS.window_token_index(H, H, 7, shift)                                  # (nW, 49) token of each window slot
    win = widx[(widx == tok0).any(1)].reshape(-1)
    dep = torch.zeros((n_img, H * H, 1), dtype=torch.bool, device=dev)
    dep[img0, win.to(dev)] = True

    def run(xv):
        with torch.no_grad():
            return ops.window_block(xv, P["g"], P["b"], EPS, P["wqkv"], P["bqkv"], P["wproj"], P["bproj"], P["table"], index, md, n_img, H, H, nh, shift, 32 ** -0.5)
    clean = run(x)
    assert bool(torch.isfinite(clean.float()).all())
    failures = []
    for p in POISONS:
        xp = x.clone()
        xp[img0, tok0, c0] = p
        _footprint(f"window_block {dtype} s{shift} x={p}", clean, run(xp), dep, failures)
    assert not failures, failures


@pytest.mark.parametrize("C", [96, 192])
def test_footprint_fused_mlp_fp32(dev, C, monkeypatch):
    """the fp32 instantiations (csrc/mlp_ref.hip, erf GELU): ops.mlp with the residual and ops.mlp_ln at M = 4096 -- here the whole row of y is non-finite,
    for NaN and for +inf (gelu(-inf) = -inf * 0 in the erf form), and no other row changes"""
    monkeypatch.setattr(ops, "_MLP_FUSED_WIDTHS", (96, 192))
    M, r0, c0 = 4096, 2999, C - 1
    x = V.randn((M, C), 370).to(dev)
    P = {k: t.to(dev) for k, t in _mlp_ln_params(C, 371).items()}

    def run(xv):
        with torch.no_grad():
            return dict(y_mlp=ops.mlp(xv, P["w1"], P["b1"], P["w2"], P["b2"], res=xv),
                        y_mlp_ln=ops.mlp_ln(xv, P["g"], P["b"], EPS, P["w1"], P["b1"], P["w2"], P["b2"]))
    clean = run(x)
    row = _rowmask((M, 1), r0, dev)
    failures = []
    for p in POISONS:
        xp = x.clone()
        xp[r0, c0] = p
        for k_, t in run(xp).items():
            _footprint(f"mlp fp32 C={C} x={p} {k_}", clean[k_], t, row, failures)
    assert not failures, failures
