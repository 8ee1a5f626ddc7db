"""ops.pool_head_loss (csrc/pool_head.hip: additive-attention pooling -> dropout -> classifier -> cross-entropy, two launches per direction) against the
fp64 restatement tests/support_unimodal_oracle.head_reference, itself held to autograd of oracle.multimodal.additive_attention at 1e-10 in
tests/test_unimodal_oracle_cpu.py.

Shapes: the V-only model's (L = 160, B = 1 / 4), the multimodal tail's (320, 326 = 38 + 128 + 160, 486 at B = 16) and a two-token corner; NL = 7; ragged masks
with a fully valid row and a row of exactly one valid token; labels over all classes (B = 16).
Bars: fp32 -- every output and gradient within 1e-3 of max|ref| of its tensor (the fp32 bar of tests/test_gpu_step_oracle.py); d(v_b), identically zero by the
softmax's shift invariance, within 1e-3 of sum |d(score_t)| (a cancelling sum is judged against its summands, as that file's docstring explains).
bf16 -- the inputs are rounded first and the ROUNDED values go to the reference: forward within 2e-2, gradients within 4e-2 of the tensor's scale.
Dropout -- the reference runs on the kernel's own keep mask (the recipe of tests/test_gpu_glue.py), and the mask's statistics are held to 4 sigma."""
import math

import pytest
import torch

from tests import support_unimodal_oracle as UO

pytestmark = pytest.mark.gpu

SHAPES = [(1, 160, 768), (4, 160, 768), (4, 320, 768), (4, 326, 768), (16, 486, 768), (3, 2, 64)]
NL = 7
DLOSS = 0.37
FWD = ("loss", "logits", "alpha")
GRADS = ("dh", "dph", "dqq", "dv", "dW", "db")
BARS = {torch.float32: (1e-3, 1e-3), torch.bfloat16: (2e-2, 4e-2)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def inputs(dev, shape, dtype, seed=40):
    """CPU inputs (rounded to `dtype` where the kernel reads `dtype`) and their device copies as leaves, the parameters in the modules' own shapes"""
    B, L, H = shape
    cpu, lengths = UO.head_inputs(B, L, H, NL, seed)
    assert lengths[0] == L and (B == 1 or lengths[-1] == 1)
    cpu["h"], cpu["ph"] = cpu["h"].to(dtype).float(), cpu["ph"].to(dtype).float()
    d = {k: v.to(dev) for k, v in cpu.items()}
    d["h"], d["ph"] = d["h"].to(dtype).requires_grad_(True), d["ph"].to(dtype).requires_grad_(True)
    d["value_w"] = d["value_w"].reshape(1, H)                # nn.Linear(H, 1).weight
    for k in ("qq", "value_w", "value_b", "cls_w", "cls_b"):
        d[k].requires_grad_(True)
    return cpu, d


def run_op(d, p, seed):
    """forward + backward through the public op; returns everything the reference has a counterpart for, plus keep / pooled from the raw entry point"""
    from facialmmt_amd import ops
    for t in d.values():
        t.grad = None
    loss, logits = ops.pool_head_loss(d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"], p, seed)
    assert not logits.requires_grad
    (loss * DLOSS).backward()
    with torch.no_grad():
        rloss, rlogits, alpha, pooled, keep = ops.pool_head_fwd_raw(d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"],
                                                                    d["labels"], p, seed)
    torch.cuda.synchronize()
    assert torch.equal(rlogits, logits) and torch.equal(rloss, loss.detach())       # the same seed: the same bits
    return dict(loss=loss.detach(), logits=logits, alpha=alpha, pooled=pooled, keep=keep, dh=d["h"].grad, dph=d["ph"].grad, dqq=d["qq"].grad,
                dv=d["value_w"].grad.reshape(-1), dvb=d["value_b"].grad, dW=d["cls_w"].grad, db=d["cls_b"].grad)


def compare(got, ref, dtype, label):
    fwd_bar, grad_bar = BARS[dtype]
    bad = []
    for k in FWD + GRADS:
        g, r = got[k].detach().double().cpu().reshape(-1), ref[k].reshape(-1)
        scale = float(r.abs().max())
        err = float((g - r).abs().max())
        bar = fwd_bar if k in FWD else grad_bar
        print(f"{label} {k}: max|got - ref| {err:.3e} = {err / scale:.3e} of max|ref| {scale:.3e} (bar {bar:.0e})")
        if not (scale > 0 and err <= bar * scale):
            bad.append((k, err, scale))
    cancel = float(ref["dscore"].abs().sum())                # (the upstream gradient is already in it)
    dvb = float(got["dvb"].detach().double().abs().max())
    print(f"{label} dvb: |got| {dvb:.3e} against sum|dscore| {cancel:.3e} (bar {grad_bar:.0e})")
    if not dvb <= grad_bar * cancel:
        bad.append(("dvb", dvb, cancel))
    assert not bad, (label, bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_every_gradient(dev, shape, dtype):
    cpu, d = inputs(dev, shape, dtype)
    got = run_op(d, 0.0, 0)
    assert float(got["keep"].min()) == 1.0 and float(got["keep"].max()) == 1.0
    ref = UO.head_reference(**cpu, keep=torch.ones(shape[0], shape[2]), dloss=DLOSS)
    assert got["dh"].dtype == dtype and got["dph"].dtype == dtype and got["dW"].shape == (NL, shape[2]) and d["value_w"].grad.shape == (1, shape[2])
    compare(got, ref, dtype, f"{shape} {dtype}")
    if shape[0] > 1:                                          # the row with one valid token: all weight on it, none elsewhere
        assert float(got["alpha"][-1, 0]) == 1.0 and float(got["alpha"][-1, 1:].abs().max()) == 0.0
    if shape[0] >= NL:
        assert sorted(set(cpu["labels"].tolist())) == list(range(NL))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", [(4, 160, 768), (16, 486, 768)], ids=lambda s: "x".join(map(str, s)))
def test_dropout_against_the_reference_on_the_kernels_own_mask(dev, shape, p, dtype):
    B, _, H = shape
    cpu, d = inputs(dev, shape, dtype)
    got = run_op(d, p, 1234567)
    keep = got["keep"].cpu()
    values = sorted(set(keep.reshape(-1).tolist()))
    assert len(values) == 2 and values[0] == 0.0, values
    s = values[1]
    share = float((keep != 0).double().mean())
    n = B * H
    print(f"{shape} p={p}: kept share {share:.5f} (1 - p = {1 - p}), scale {s:.6f}, bars {4 * math.sqrt(p * (1 - p) / n):.4f} / {4 * math.sqrt(p / ((1 - p) * n)):.4f}")
    assert abs(share - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n)
    assert abs(s * (1 - p) - 1) <= 4 * math.sqrt(p / ((1 - p) * n))
    ref = UO.head_reference(**cpu, keep=keep, dloss=DLOSS)
    compare(got, ref, dtype, f"{shape} p={p} {dtype}")


def test_seeds(dev):
    """another seed: another mask; the same seed: the same bits -- as a python integer and as a device word (what a captured graph reads)"""
    from facialmmt_amd import ops
    _, d = inputs(dev, (4, 160, 768), torch.bfloat16)
    args = (d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"])
    with torch.no_grad():
        a = ops.pool_head_fwd_raw(*args, 0.5, 11)
        b = ops.pool_head_fwd_raw(*args, 0.5, 12)
        c = ops.pool_head_fwd_raw(*args, 0.5, 11)
        word = torch.tensor([11], dtype=torch.int64, device=dev)
        e = ops.pool_head_fwd_raw(*args, 0.5, word)
        word.fill_(12)
        f = ops.pool_head_fwd_raw(*args, 0.5, word)
    assert not torch.equal(a[4], b[4]) and float((a[4] != b[4]).double().mean()) > 0.3
    for x, y in ((a, c), (a, e), (b, f)):
        assert all(torch.equal(u, v) for u, v in zip(x, y))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_runs_are_bit_identical(dev, dtype):
    _, d = inputs(dev, (16, 486, 768), dtype)
    one = {k: v.clone() for k, v in run_op(d, 0.1, 77).items()}
    two = run_op(d, 0.1, 77)
    for k in one:
        assert torch.equal(one[k], two[k]), k


def test_a_row_without_a_valid_token_gives_nan_and_leaves_the_other_rows_alone(dev):
    from facialmmt_amd import ops
    cpu, d = inputs(dev, (3, 2, 64), torch.float32)
    with torch.no_grad():
        ok = ops.pool_head_fwd_raw(d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"])
        mask = d["mask"].clone()
        mask[1] = 0
        loss, logits, alpha, pooled, _ = ops.pool_head_fwd_raw(d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], mask, d["cls_w"], d["cls_b"], d["labels"])
    assert torch.isnan(loss) and torch.isnan(logits[1]).all() and torch.isnan(alpha[1]).all() and torch.isnan(pooled[1]).all()
    assert torch.equal(logits[[0, 2]], ok[1][[0, 2]]) and torch.equal(alpha[[0, 2]], ok[2][[0, 2]])


def test_bad_arguments(dev):
    from facialmmt_amd import _lib, ops

    def call(B=2, L=4, H=64, nl=NL, device=dev):
        t = lambda *s: torch.zeros(*s, device=device)
        return ops.pool_head_loss(t(B, L, H), t(B, L, H), t(H), t(1, H), t(1), torch.ones(B, L, device=device), t(nl, H), t(nl),
                                  torch.zeros(B, dtype=torch.int64, device=device), 0.0, 0)
    loss, logits = call()
    assert abs(float(loss) - math.log(NL)) < 1e-6 and logits.shape == (2, NL)
    for kw in (dict(L=1), dict(H=12), dict(nl=9), dict(L=1025), dict(H=1032), dict(device="cpu")):
        with pytest.raises(_lib.FmmtError):
            call(**kw)
    lib = _lib.load()
    assert lib.fmmt_pool_head_bwd_workspace(4, 1, 768) == 0 and lib.fmmt_pool_head_bwd_workspace(4, 160, 768) > 0
    assert lib.fmmt_pool_head_fwd(0, 4, 1, 768, 7, *([None] * 9), 0.0, 0, *([None] * 7), 0, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_pool_head_bwd(1, 4, 160, 768, 9, *([None] * 19), 0, None) == _lib.FMMT_EINVAL
    with pytest.raises(_lib.FmmtError):                       # dropout probability outside [0, 1)
        ops.pool_head_fwd_raw(*[torch.zeros(s, device=dev) for s in ((2, 4, 64), (2, 4, 64), (64,), (64,), (1,))], torch.ones(2, 4, device=dev),
                              torch.zeros(NL, 64, device=dev), torch.zeros(NL, device=dev), torch.zeros(2, dtype=torch.int64, device=dev), 1.0, 0)
