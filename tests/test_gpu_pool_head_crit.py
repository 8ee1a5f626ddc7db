"""ops.pool_head_loss(..., criterion=) (fmmt_pool_head_fwd_crit / _bwd_crit: the pooling head with the class-weighted, label-smoothed loss of
include/fmmt_loss.h behind its classifier) on the batches of tests/test_gpu_pool_head_rows.py -- trailing rows padded (h, ph, mask of row 0, label -100).

  (a) no weights and eps = 0: loss, logits, alpha, pooled, keep and every gradient are BIT-equal (torch.equal) to valid_mean=True, and den == n_rows;
  (b) weighted and smoothed: loss, logits, alpha and every gradient against the fp64 restatement tests/support_criterion.head_reference_crit (validated in
      tests/test_criterion_cpu.py against autograd through torch.nn.CrossEntropyLoss) on the kernel's own keep mask, with the comparison and the bars
      tests/test_gpu_pool_head.py exports (fp32 1e-3 / 1e-3, bf16 2e-2 / 4e-2 of the tensor's scale; d(v_b) against sum |d(score)|); dh and dph of the
      unlabelled rows exactly zero; den the fp64 denominator to 1e-6;
  (c) no labelled row: loss 0, every gradient 0, nothing non-finite;
  (d) two runs give the same bits.

Shapes: B in {1, 3, 5} with 0, 1, B - 1 and B unlabelled rows; L in {2, 7, 320}; H in {8, 768}; NL = 7; fp32 and bf16; dropout 0 and 0.3.  Every L = 2 row has
both tokens, for the reason the docstring of tests/test_gpu_pool_head_rows.py gives (a one-token row has d(score) = 0 exactly)."""
import types

import pytest
import torch

from tests import support_criterion as SC
from tests import test_gpu_pool_head as TP
from tests import test_gpu_pool_head_rows as TR

pytestmark = pytest.mark.gpu

NL, DLOSS, ROWS, OUT = TP.NL, TP.DLOSS, TR.ROWS, TR.OUT
EPS = 0.1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run_crit(d, p, seed, weight, eps):
    from facialmmt_amd import ops
    crit = types.SimpleNamespace(weight=weight, label_smoothing=eps)
    for t in d.values():
        t.grad = None
    args = (d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"], p, seed)
    loss, logits = ops.pool_head_loss(*args, criterion=crit)
    assert not logits.requires_grad
    (loss * DLOSS).backward()
    with torch.no_grad():
        raw = ops.pool_head_fwd_crit_raw(*args, weight, eps)
    torch.cuda.synchronize()
    assert torch.equal(raw[0], loss.detach()) and torch.equal(raw[1], logits)
    out = dict(loss=loss.detach(), logits=logits, alpha=raw[2], pooled=raw[3], keep=raw[4], dh=d["h"].grad, dph=d["ph"].grad, dqq=d["qq"].grad,
               dv=d["value_w"].grad.reshape(-1), dvb=d["value_b"].grad, dW=d["cls_w"].grad, db=d["cls_b"].grad)
    out = {k: v.detach().clone() for k, v in out.items()}
    out["den"] = float(raw[5])
    return out


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [8, 768])
@pytest.mark.parametrize("L", [2, 7, 320])
@pytest.mark.parametrize("B,unlabelled", ROWS)
def test_plain_criterion_has_the_bits_of_the_rows_pair(dev, B, unlabelled, L, H, dtype, p):
    """(a), on every row pattern: class_w == NULL, eps == 0"""
    cpu, d = TR.inputs(dev, B, L, H, unlabelled, dtype)
    got = run_crit(d, p, 1234567, None, 0.0)
    rows = TR.run_op(d, p, 1234567, True)
    for k in OUT:
        assert torch.equal(got[k], rows[k]), (B, unlabelled, L, H, dtype, p, k)
    assert got["den"] == float(rows["n_rows"]) == B - unlabelled


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [8, 768])
@pytest.mark.parametrize("L", [2, 7, 320])
@pytest.mark.parametrize("B,unlabelled", ROWS)
def test_weighted_and_smoothed(dev, B, unlabelled, L, H, dtype, p):
    cpu, d = TR.inputs(dev, B, L, H, unlabelled, dtype)
    kind = "zero_class" if (B + L) % 2 else "random"          # both kinds over the grid; the zeroed class is one the labels use
    w = SC.weights_for(kind, NL, seed=int(cpu["labels"][0]) - 1 if kind == "zero_class" else 0)
    wd = w.to(dev)
    seed = 1234567
    got = run_crit(d, p, seed, wd, EPS)
    label = f"B={B} unlabelled={unlabelled} L={L} H={H} {dtype} p={p} {kind}"
    assert all(torch.isfinite(got[k]).all() for k in OUT), label
    again = run_crit(d, p, seed, wd, EPS)                                          # (d)
    assert all(torch.equal(got[k], again[k]) for k in OUT) and again["den"] == got["den"], label
    ref = SC.head_reference_crit(**cpu, keep=got["keep"].cpu(), weight=w, eps=EPS, dloss=DLOSS)
    assert abs(got["den"] - float(ref["den"])) <= 1e-6 * max(float(ref["den"]), 1e-30), label
    if float(ref["den"]) == 0.0:                                                   # (c): no labelled row, or only rows of the class whose weight is 0
        assert float(got["loss"]) == 0.0, label
        for k in ("dh", "dph", "dqq", "dv", "dvb", "dW", "db"):
            assert float(got[k].abs().max()) == 0.0, (label, k)
        return
    TP.compare(got, ref, dtype, label)                                             # (b)
    if unlabelled:
        assert float(got["dh"][B - unlabelled:].abs().max()) == 0.0 and float(got["dph"][B - unlabelled:].abs().max()) == 0.0, label
    assert float(got["dh"][:B - unlabelled].abs().max()) > 0.0


def test_limits_and_the_registered_operator(dev):
    from facialmmt_amd import _lib, ops
    import facialmmt_amd.torch_ops  # noqa: F401
    crit = types.SimpleNamespace(weight=torch.ones(NL, device=dev), label_smoothing=0.1)

    def call(c=crit, B=2, L=4, H=64, nl=NL, device=dev):
        t = lambda *s: torch.zeros(*s, device=device)
        return ops.pool_head_loss(t(B, L, H), t(B, L, H), t(H), t(1, H), t(1), torch.ones(B, L, device=device), t(nl, H), t(nl),
                                  torch.zeros(B, dtype=torch.int64, device=device), 0.0, 0, criterion=c)
    assert abs(float(call()[0]) - 1.9459101) < 1e-6           # uniform logits: log 7 whatever the weights and the smoothing
    ns = types.SimpleNamespace
    for kw in (dict(L=1), dict(H=12), dict(nl=9), dict(L=1025), dict(device="cpu"), dict(c=ns(weight=torch.ones(6, device=dev), label_smoothing=0.0)),
               dict(c=ns(weight=torch.ones(NL), label_smoothing=0.0)), dict(c=ns(weight=None, label_smoothing=1.0)),
               dict(c=ns(weight=torch.ones(NL, device=dev, dtype=torch.float64), label_smoothing=0.0))):
        with pytest.raises(_lib.FmmtError):
            call(**kw)
    cpu, d = TR.inputs(dev, 3, 7, 8, 1, torch.float32)
    w = SC.weights_for("random", NL).to(dev)
    got = run_crit(d, 0.3, 99, w, EPS)
    for t in d.values():
        t.grad = None
    out = torch.ops.fmmt.pool_head_loss_crit(d["h"], d["ph"], d["qq"], d["value_w"], d["value_b"], d["mask"], d["cls_w"], d["cls_b"], d["labels"], 0.3, 99, w, EPS)
    (out[0] * DLOSS).backward()
    assert torch.equal(out[0].detach(), got["loss"]) and torch.equal(out[1], got["logits"]) and torch.equal(out[4], got["keep"]) and float(out[5].detach()) == got["den"]
    for k, t in (("dh", d["h"]), ("dph", d["ph"]), ("dqq", d["qq"]), ("dW", d["cls_w"]), ("db", d["cls_b"]), ("dvb", d["value_b"])):
        assert torch.equal(t.grad, got[k]), k
