"""ops.pool_head_loss(..., valid_mean=True) (fmmt_pool_head_fwd_rows / _bwd_rows: the pooling head's loss as a mean over the rows that have a label) on
batches whose trailing rows are padded rows -- h, ph and mask copies of row 0, label -100 (train_step.pad_unimodal_batch's rule).

  (a) every label valid: loss, logits, alpha, pooled, keep and every gradient are BIT-equal to the plain pair's, and n_rows == B;
  (b) some rows unlabelled: loss, logits, alpha and every gradient against the fp64 restatement tests/support_pad_rows.head_reference_rows (validated in
      tests/test_pad_rows_cpu.py) on the kernel's own keep mask, with the comparison and the bars of tests/test_gpu_pool_head.py (imported: fp32 1e-3 /
      1e-3, bf16 2e-2 / 4e-2 of the tensor's scale; d(v_b) against sum |d(score)|); dh and dph of the unlabelled rows exactly zero; n_rows the count;
  (c) no labelled row: loss 0, every gradient 0, nothing non-finite, n_rows == 0;
  (d) two runs give the same bits;
  (e) limits and alignment: the plain pair's errors (the return codes themselves are compared without a GPU in tests/test_pad_rows_cpu.py).

Shapes: B in {1, 3, 5} with 0, 1, B - 1 and B unlabelled rows; L = 2, L = 7 (one split, odd) and L = 320 (several splits: the meld_utt_320 length);
H = 8 and the model's 768; NL = 7; fp32 and bf16; dropout 0 and 0.3.

Inputs: tests/support_unimodal_oracle.head_inputs.  At L = 2 its ragged lengths are (2, 1, 1, ...): a row with one valid token has d(score) = 0 exactly, so dph, dqq
and dv of the whole batch hang on ONE cancelling dot product, d(pooled) . (h_0 - h_1) of row 0, and a bar relative to max|ref| measures that scalar's luck.
test_valid_mean therefore gives every L = 2 row both tokens (each labelled row then brings a dot product of its own); test_valid_mean_ragged_two_tokens keeps the
ragged L = 2 batches for everything that does not cancel: n_rows, loss, logits, alpha, dh, dW, db at the same bars, and the exact zeros."""
import pytest
import torch

from tests import support_pad_rows as PR
from tests import support_unimodal_oracle as UO
from tests import test_gpu_pool_head as TP

pytestmark = pytest.mark.gpu

NL, DLOSS = TP.NL, TP.DLOSS
ROWS = [(B, u) for B in (1, 3, 5) for u in sorted({0, 1, B - 1, B})]
OUT = ("loss", "logits", "alpha", "pooled", "keep", "dh", "dph", "dqq", "dv", "dvb", "dW", "db")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def inputs(dev, B, L, H, unlabelled, dtype, ragged=False):
    cpu, _ = UO.head_inputs(B, L, H, NL, 40, lengths=[2] * B if L == 2 and not ragged else None)      # L == 2: module docstring
    cpu = PR.pad_head_inputs(cpu, unlabelled)
    cpu["h"], cpu["ph"] = cpu["h"].to(dtype).float(), cpu["ph"].to(dtype).float()
    d = {k: v.to(dev) for k, v in cpu.items()}
    d["h"], d["ph"] = d["h"].to(dtype).requires_grad_(True), d["ph"].to(dtype).requires_grad_(True)
    d["value_w"] = d["value_w"].reshape(1, H)
    for k in ("qq", "value_w", "value_b", "cls_w", "cls_b"):
        d[k].requires_grad_(True)
    return cpu, d


def run_op(d, p, seed, valid_mean):
    from facialmmt_amd import ops
    for t in d.values():
        t.grad = None
    args = (d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"], p, seed)
    loss, logits = ops.pool_head_loss(*args, valid_mean=valid_mean)
    (loss * DLOSS).backward()
    with torch.no_grad():
        raw = ops.pool_head_fwd_raw(*args, valid_mean=valid_mean)
    torch.cuda.synchronize()
    assert torch.equal(raw[0], loss.detach()) and torch.equal(raw[1], logits)
    out = dict(loss=loss.detach(), logits=logits, alpha=raw[2], pooled=raw[3], keep=raw[4], dh=d["h"].grad, dph=d["ph"].grad, dqq=d["qq"].grad,
               dv=d["value_w"].grad.reshape(-1), dvb=d["value_b"].grad, dW=d["cls_w"].grad, db=d["cls_b"].grad)
    out = {k: v.detach().clone() for k, v in out.items()}
    if valid_mean:
        out["n_rows"] = int(raw[5])
    return out


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [8, 768])
@pytest.mark.parametrize("L", [2, 7, 320])
@pytest.mark.parametrize("B,unlabelled", ROWS)
def test_valid_mean(dev, B, unlabelled, L, H, dtype, p):
    cpu, d = inputs(dev, B, L, H, unlabelled, dtype)
    seed = 1234567
    got = run_op(d, p, seed, True)
    label = f"B={B} unlabelled={unlabelled} L={L} H={H} {dtype} p={p}"
    assert got["n_rows"] == B - unlabelled, label
    assert all(torch.isfinite(got[k]).all() for k in OUT), label
    again = run_op(d, p, seed, True)                                              # (d)
    assert all(torch.equal(got[k], again[k]) for k in OUT) and again["n_rows"] == got["n_rows"], label
    if unlabelled == 0:                                                            # (a)
        plain = run_op(d, p, seed, False)
        for k in OUT:
            assert torch.equal(got[k], plain[k]), (label, k)
        return
    if unlabelled == B:                                                            # (c)
        assert float(got["loss"]) == 0.0, label
        for k in ("dh", "dph", "dqq", "dv", "dvb", "dW", "db"):
            assert float(got[k].abs().max()) == 0.0, (label, k)
        return
    ref = PR.head_reference_rows(**cpu, keep=got["keep"].cpu(), dloss=DLOSS)      # (b)
    TP.compare(got, ref, dtype, label)
    assert float(got["dh"][B - unlabelled:].abs().max()) == 0.0 and float(got["dph"][B - unlabelled:].abs().max()) == 0.0, label
    assert float(got["dh"][:B - unlabelled].abs().max()) > 0.0


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [8, 768])
@pytest.mark.parametrize("B,unlabelled", [(B, u) for B, u in ROWS if 0 < u < B])
def test_valid_mean_ragged_two_tokens(dev, B, unlabelled, H, dtype, p):
    """L = 2 with the generator's ragged lengths (row 0 two tokens, the others one): the quantities that do not hang on the one cancelling dot product"""
    cpu, d = inputs(dev, B, 2, H, unlabelled, dtype, ragged=True)
    assert cpu["mask"].sum(1).tolist() == [2.0] + [1.0] * (B - 1 - unlabelled) + [2.0] * unlabelled
    got = run_op(d, p, 1234567, True)
    label = f"ragged B={B} unlabelled={unlabelled} L=2 H={H} {dtype} p={p}"
    ref = PR.head_reference_rows(**cpu, keep=got["keep"].cpu(), dloss=DLOSS)
    assert got["n_rows"] == B - unlabelled and all(torch.isfinite(got[k]).all() for k in OUT), label
    fwd_bar, grad_bar = TP.BARS[dtype]
    bad = []
    for k in ("loss", "logits", "alpha", "dh", "dW", "db"):
        r = ref[k].reshape(-1)
        scale, err = float(r.abs().max()), float((got[k].double().cpu().reshape(-1) - r).abs().max())
        bar = fwd_bar if k in TP.FWD else grad_bar
        print(f"{label} {k}: max|got - ref| {err:.3e} = {err / scale:.3e} of max|ref| {scale:.3e} (bar {bar:.0e})")
        if not (scale > 0 and err <= bar * scale):
            bad.append((k, err, scale))
    assert not bad, (label, bad)
    assert float(got["dh"][B - unlabelled:].abs().max()) == 0.0 and float(got["dph"][B - unlabelled:].abs().max()) == 0.0, label


def test_limits_and_alignment_are_the_plain_pairs(dev):
    from facialmmt_amd import _lib, ops

    def call(valid_mean, B=2, L=4, H=64, nl=NL, device=dev):
        t = lambda *s: torch.zeros(*s, device=device)
        return ops.pool_head_loss(t(B, L, H), t(B, L, H), t(H), t(1, H), t(1), torch.ones(B, L, device=device), t(nl, H), t(nl),
                                  torch.zeros(B, dtype=torch.int64, device=device), 0.0, 0, valid_mean)
    assert torch.equal(call(True)[0], call(False)[0])
    for kw in (dict(L=1), dict(H=12), dict(nl=9), dict(L=1025), dict(H=1032), dict(device="cpu")):
        for valid_mean in (False, True):
            with pytest.raises(_lib.FmmtError):
                call(valid_mean, **kw)
    lib = _lib.load()
    assert lib.fmmt_pool_head_fwd_rows(0, 4, 1, 768, 7, *([None] * 9), 0.0, 0, *([None] * 8), 0, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_pool_head_bwd_rows(1, 4, 160, 768, 9, *([None] * 20), 0, None) == _lib.FMMT_EINVAL
