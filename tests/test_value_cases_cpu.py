"""The value cases of tests/support_value_cases.py judged on the CPU, without a kernel: fp32 torch restatements of LayerNorm and of the online softmax go
through the generators, the class-local metric and the yardstick max(base, K * stock).  The honest restatements (two-pass variance; max-subtracted
online softmax over tiles of 64 and of 8 keys, rescale guarded) pass every class; each deliberately wrong one misses its bound by at least 10x on
the class built for it.  That is the condition K is chosen under: tests/test_gpu_value_edges.py applies the same generators, metric and K to the kernels."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import support_value_cases as V

LN_BASE = 1e-5          # support_op_cases.t_layernorm, fp32
MHA_BASE = 2e-5         # support_op_cases.t_mha, fp32
EPS = 1e-5
MISS = 10.0


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm restatements (fp32)
def ln_two_pass(x, g, b, eps=EPS):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps) * g + b


def ln_one_pass(x, g, b, eps=EPS):
    """WRONG on rows with |mean| >> std: var = E[x^2] - E[x]^2 cancels"""
    mean = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
    return (x - mean) * torch.rsqrt(var + eps) * g + b


def ln_eps_outside(x, g, b, eps=EPS):
    """WRONG where var <~ eps: 1 / (sqrt(var) + eps)"""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    return d / ((d * d).mean(-1, keepdim=True).sqrt() + eps) * g + b


def ln_row_scaled(x, g, b, eps=EPS):
    """WRONG in the ordinary channels of a row with an outlier: x - mean kept on a grid of 1.5 * 2^-17 of the row's largest |x - mean| (a block-scaled
    intermediate).  The error is far below the outlier channels' scale and far above the ordinary channels' rounding."""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    step = d.abs().amax(-1, keepdim=True).clamp_min(1e-30) * 1.5 * 2.0 ** -17
    d = torch.round(d / step) * step
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps) * g + b


def _ln_case(C, fn, M=66, seed=5):
    x, cls, omask = V.norm_rows(M, C, torch.float32, seed=seed)
    g = V.randn((C,), 2) * 0.2 + 1
    b = V.randn((C,), 3) * 0.1
    ref = V.layer_norm64(x.double(), g.double(), b.double(), EPS)
    return x, g, b, cls, omask, ref, fn(x, g, b), F.layer_norm(x, (C,), g, b, EPS)


@pytest.mark.parametrize("C", V.LN_CHANNELS)
def test_two_pass_layer_norm_passes_every_class(C):
    x, g, b, cls, omask, ref, got, stock = _ln_case(C, ln_two_pass)
    failures = []
    V.judge(f"cpu two-pass LN C={C}", V.class_errors(got, ref, cls, V.NORM_CLASSES, omask, skip=V.CONST_CLASSES),
            V.class_errors(stock, ref, cls, V.NORM_CLASSES, omask, skip=V.CONST_CLASSES), LN_BASE, failures)
    assert not failures, failures
    assert bool(torch.isfinite(got).all())
    for i, name in enumerate(V.NORM_CLASSES):
        if name in V.CONST_CLASSES:
            dev = float((got[cls == i] - b).abs().max())
            assert dev <= V.const_row_bound(g, V.CONST_CLASSES[name], EPS), (name, dev)


@pytest.mark.parametrize("C", V.LN_CHANNELS)
@pytest.mark.parametrize("fn,klass", [(ln_one_pass, "offset"), (ln_eps_outside, "tiny"), (ln_row_scaled, "outlier/rest")],
                         ids=["one-pass-variance", "eps-outside-sqrt", "row-scaled-intermediate"])
def test_wrong_layer_norm_misses_by_10x(C, fn, klass):
    x, g, b, cls, omask, ref, got, stock = _ln_case(C, fn)
    e = V.class_errors(got, ref, cls, V.NORM_CLASSES, omask)[klass]
    s = V.class_errors(stock, ref, cls, V.NORM_CLASSES, omask)[klass]
    bar = V.bound(LN_BASE, s)
    print(f"{fn.__name__} C={C} [{klass}]: got={e:.3e} stock={s:.3e} bound={bar:.3e} miss={e / bar:.1f}x")
    assert e >= MISS * bar, (fn.__name__, klass, e, bar)


@pytest.mark.parametrize("C", V.LN_CHANNELS)
def test_global_scale_hides_what_the_class_metric_sees(C):
    """the row-scaled LayerNorm passes support_op_cases.report()'s metric (max|err| over the tensor's global max|ref|) at t_layernorm's tolerance and
    misses the class-local one by >= 10x in the ordinary channels of the outlier rows"""
    x, g, b, cls, omask, ref, got, stock = _ln_case(C, ln_row_scaled)
    glob = V.global_errors(got, ref, cls, V.NORM_CLASSES, omask)["outlier/rest"]
    loc = V.class_errors(got, ref, cls, V.NORM_CLASSES, omask)["outlier/rest"]
    s = V.class_errors(stock, ref, cls, V.NORM_CLASSES, omask)["outlier/rest"]
    print(f"C={C}: global-scale metric {glob:.3e} (tolerance {LN_BASE:g}), class-local {loc:.3e} (bound {V.bound(LN_BASE, s):.3e})")
    assert glob <= LN_BASE
    assert loc >= MISS * V.bound(LN_BASE, s)


@pytest.mark.parametrize("C", V.LN_CHANNELS + (1024,))
def test_const_row_bound_holds_for_stock_layer_norm(C):
    g = V.randn((C,), 2) * 0.2 + 1
    b = V.randn((C,), 3) * 0.1
    for c in V.CONST_CLASSES.values():
        y = F.layer_norm(torch.full((5, C), c), (C,), g, b, EPS)
        dev = float((y - b).abs().max())
        assert bool(torch.isfinite(y).all()) and dev <= V.const_row_bound(g, c, EPS), (C, c, dev)
        if c == 0.0 or C == 1024:
            assert torch.equal(y, b.expand(5, C)), (C, c)


# ------------------------------------------------------------------------------------------------------------------------ softmax restatements (fp32)
def online_attention(q, k, v, nh, scale, kb, tile=64, guard=True, rescale_acc=True):
    """the kernels' scheme: keys in tiles, running max m and sum l, accumulator o rescaled by exp(m - mnew).  guard=False: the rescale and the
    exponentials subtract mnew even where it is -inf (-inf - -inf = NaN).  rescale_acc=False: o is not rescaled (l is)."""
    qh, kh, vh = V.heads(q, nh) * scale, V.heads(k, nh), V.heads(v, nh)
    s = qh @ kh.transpose(-1, -2)
    if kb is not None:
        s = s + kb[:, None, None, :]
    B, _, Lq, Lk = s.shape
    m = torch.full((B, nh, Lq), float("-inf"))
    l = torch.zeros((B, nh, Lq))
    o = torch.zeros((B, nh, Lq, vh.shape[-1]))
    for j0 in range(0, Lk, tile):
        st = s[..., j0:j0 + tile]
        mnew = torch.maximum(m, st.amax(-1))
        mref = torch.where(torch.isinf(mnew) & (mnew < 0), torch.zeros_like(mnew), mnew) if guard else mnew
        alpha = torch.exp(m - mref)
        e = torch.exp(st - mref[..., None])
        l = l * alpha + e.sum(-1)
        o = (o * alpha[..., None] if rescale_acc else o) + e @ vh[:, :, j0:j0 + tile]
        m = mnew
    o = o / l[..., None]
    return o.permute(2, 0, 1, 3).reshape(Lq, B, -1)


def plain_exp_attention(q, k, v, nh, scale, kb):
    """WRONG: exp(s) / sum exp(s) without subtracting the maximum"""
    s = (V.heads(q, nh) * scale) @ V.heads(k, nh).transpose(-1, -2)
    if kb is not None:
        s = s + kb[:, None, None, :]
    e = torch.exp(s)
    o = (e / e.sum(-1, keepdim=True)) @ V.heads(v, nh)
    return o.permute(2, 0, 1, 3).reshape(q.shape)


SHAPE = dict(Lq=70, Lk=130, B=2, E=128, nh=2)
CASES = [(s, None) for s in V.SCORE_KINDS] + [("unit", kb) for kb in V.KEY_BIAS_KINDS]


def _mha_case(score, bias):
    nh, hd = SHAPE["nh"], SHAPE["E"] // SHAPE["nh"]
    q, k, v = V.mha_inputs(score, dtype=torch.float32, seed=20, **SHAPE)
    kb = V.key_bias(bias, SHAPE["B"], SHAPE["Lk"], seed=20) if bias else None
    ref = V.attention(q.double(), k.double(), v.double(), nh, hd ** -0.5, kb)
    stock = V.attention(q, k, v, nh, hd ** -0.5, kb)
    return q, k, v, kb, nh, hd ** -0.5, ref, stock


def _miss(fn, score, bias, **kw):
    q, k, v, kb, nh, scale, ref, stock = _mha_case(score, bias)
    e, s = V.rel_err(fn(q, k, v, nh, scale, kb, **kw), ref), V.rel_err(stock, ref)
    bar = V.bound(MHA_BASE, s)
    print(f"{fn.__name__} {kw} [{score}, {bias}]: got={e:.3e} stock={s:.3e} bound={bar:.3e}")
    return e / bar


@pytest.mark.parametrize("tile", [64, 8])
@pytest.mark.parametrize("score,bias", CASES)
def test_guarded_online_softmax_passes_every_class(score, bias, tile):
    q, k, v, kb, nh, scale, ref, stock = _mha_case(score, bias)
    got = online_attention(q, k, v, nh, scale, kb, tile=tile)
    failures = []
    V.judge(f"cpu online softmax tile={tile} {score} {bias}", {"out": V.rel_err(got, ref)}, {"out": V.rel_err(stock, ref)}, MHA_BASE, failures)
    assert not failures, failures
    if bias == "one":        # every key but one at -inf: the output is that key's v
        vh = V.heads(v, nh)
        for b in range(SHAPE["B"]):
            want = vh[b, :, V.one_key(b, SHAPE["Lk"])].reshape(-1)
            assert float((got[:, b] - want).abs().max()) <= 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("score", ["shift+", "shift-"])
def test_softmax_without_max_subtraction_misses(score):
    assert _miss(plain_exp_attention, score, None) >= MISS


@pytest.mark.parametrize("bias,tile", [("lead8", 8), ("lead64", 8), ("lead64", 64), ("lead70", 8), ("lead70", 64)])
def test_unguarded_rescale_misses_on_leading_minus_inf(bias, tile):
    assert _miss(online_attention, "unit", bias, tile=tile, guard=False) >= MISS


def test_forgotten_accumulator_rescale_misses_on_sharp():
    assert _miss(online_attention, "sharp", None, rescale_acc=False) >= MISS


def test_generators_are_what_they_say():
    """the classes have the properties the cases rely on"""
    x, cls, omask = V.norm_rows(66, 96, torch.float32, seed=5)
    off = x[cls == V.NORM_CLASSES.index("offset")]
    assert float(off.mean(-1).abs().min()) > 500 * float(off.std(-1).max())
    xb, _, _ = V.norm_rows(66, 96, torch.bfloat16, seed=5)
    assert set(xb[cls == V.NORM_CLASSES.index("offset")].float().unique().tolist()) <= set(V.BF16_OFFSET_GRID)
    rows = omask.any(1)
    assert bool((omask.sum(1)[rows] == 2).all()) and bool(omask[:, 0].any()) and bool(omask[:, -1].any())
    assert float(x[cls == V.NORM_CLASSES.index("tiny")].var(-1).max()) < EPS
    assert float(x.abs().max()) ** 2 * 1536 < torch.finfo(torch.float32).max
    nh, hd = SHAPE["nh"], SHAPE["E"] // SHAPE["nh"]
    for kind, centre in (("shift+", V.SHIFT), ("shift-", -V.SHIFT)):
        q, k, _ = V.mha_inputs(kind, dtype=torch.float32, seed=20, **SHAPE)
        s = (V.heads(q.double(), nh) * hd ** -0.5) @ V.heads(k.double(), nh).transpose(-1, -2)
        assert float((s - centre).abs().max()) < 12.0
    q, k, _ = V.mha_inputs("sharp", dtype=torch.float32, seed=20, **SHAPE)
    s = (V.heads(q.double(), nh) * hd ** -0.5) @ V.heads(k.double(), nh).transpose(-1, -2)
    assert 25.0 < float(s.std()) < 35.0
    for kind in V.KEY_BIAS_KINDS:
        kb = V.key_bias(kind, 2, 130)
        assert bool(torch.isfinite(kb).any(1).all())
    assert bool(torch.isinf(V.key_bias("lead70", 2, 130)[0, :70]).all()) and math.isfinite(float(V.key_bias("lead70", 2, 130)[0, 70]))
