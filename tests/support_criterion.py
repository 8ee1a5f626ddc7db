"""The independent side of the criterion tests (class-weighted, label-smoothed cross-entropy as a construction argument of the training steps).

  * head_reference_crit: tests/support_pad_rows.head_reference_rows with the row loss of include/fmmt_loss.h -- the pooling head's forward and backward
    written out in fp64 (no autograd) on a given keep mask; d(logits) = dloss / den (p sum_c t_c - t), everything behind it as
    tests/support_unimodal_oracle.head_reference states it.  Validated in tests/test_criterion_cpu.py against autograd through
    torch.nn.CrossEntropyLoss(weight, label_smoothing) (head_autograd_crit: support_unimodal_oracle.head_autograd's construction with that loss).
  * loss_replaced: the fp64 steps of tests/support_step_oracle.py and tests/support_unimodal_oracle.py with their F.cross_entropy replaced by
    Criterion.reference -- the name `F` of those two modules is bound, for the length of the block, to torch.nn.functional with that one function
    replaced, so their loops (accumulation, total norm, clip, SGD) run as they are written.
  * cases / weights_for: the weight, smoothing and ignored-row cases the CPU and GPU tests share."""
from __future__ import annotations

import contextlib

import torch

from oracle.multimodal import additive_attention

from tests import support_step_oracle as SO
from tests import support_unimodal_oracle as UO

WEIGHT_KINDS = ("none", "random", "zero_class")


def weights_for(kind, NL, seed=0):
    """None; NL numbers in [0.2, 3]; the same with one class at 0 (fp32 values, as a Criterion holds them)"""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(1000 + 17 * NL + seed)
    w = (0.2 + 2.8 * torch.rand(NL, generator=g, dtype=torch.float64)).float()
    if kind == "zero_class":
        w[(seed + 1) % NL] = 0.0
    return w


def ignored_rows(B, which):
    """the rows whose label becomes -100: which in ("none", "one", "all_but_one")"""
    n = {"none": 0, "one": min(1, B), "all_but_one": B - 1}[which]
    return list(range(B - n, B)) if which != "one" else ([B // 2] if B else [])


def logits_and_labels(B, NL, seed, ignored="none", scale=3.0):
    """fp32 logits in [-scale, scale] and labels over all classes, the chosen rows ignored (one of them with a label >= NL instead of -100 when
    there are two or more)"""
    g = torch.Generator().manual_seed(seed * 7919 + B * 31 + NL)
    x = ((torch.rand(B, NL, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()
    y = (torch.arange(B) * 3 + seed) % NL
    rows = ignored_rows(B, ignored)
    for i, r in enumerate(rows):
        y[r] = NL + 2 if (i == 1) else -100
    return x, y


def head_reference_crit(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, keep, weight=None, eps=0.0, dloss=1.0):
    """fp64, by hand: the forward of support_unimodal_oracle.head_reference up to the logits; the loss and d(logits) of include/fmmt_loss.h (a label
    outside [0, NL): no loss, a zero gradient row; den == 0: loss 0, every gradient 0); the backward behind d(logits) as head_reference writes it."""
    dd = torch.float64
    h, ph, qq, v, vb, mask, W, b, keep = (t.detach().to(dd) for t in (h, ph, qq.reshape(-1), value_w.reshape(-1), value_b.reshape(-1), mask, cls_w, cls_b, keep))
    B, NL = h.shape[0], W.shape[0]
    th = torch.tanh(ph + qq)
    score = th @ v + vb
    score = torch.where(mask == 0, torch.full_like(score, float("-inf")), score)
    e = torch.exp(score - score.max(dim=1, keepdim=True).values)
    alpha = e / e.sum(dim=1, keepdim=True)
    pooled = torch.einsum("bt,bth->bh", alpha, h)
    pd = pooled * keep
    logits = pd @ W.t() + b
    mx = logits.max(dim=1, keepdim=True).values
    lse = mx + torch.log(torch.exp(logits - mx).sum(dim=1, keepdim=True))
    logp = logits - lse
    valid = ((labels >= 0) & (labels < NL)).to(dd)
    y = labels.clamp(0, NL - 1)
    w = torch.ones(NL, dtype=dd) if weight is None else weight.detach().to(dd)
    onehot = torch.zeros_like(logits)
    onehot[torch.arange(B), y] = 1.0
    t = valid[:, None] * ((1.0 - eps) * w[y][:, None] * onehot + (eps / NL) * w[None, :])
    num = -(t * logp).sum()
    den = (valid * w[y]).sum()
    if float(den) > 0:
        loss = num / den
        dlogits = float(dloss) / den * (torch.exp(logp) * t.sum(1, keepdim=True) - t)
    else:
        loss = torch.zeros((), dtype=dd)
        dlogits = torch.zeros_like(logits)
    dpooled = keep * (dlogits @ W)
    dscore = alpha * (torch.einsum("bh,bth->bt", dpooled, h) - (dpooled * pooled).sum(1, keepdim=True))
    dh = alpha[:, :, None] * dpooled[:, None, :]
    dph = dscore[:, :, None] * v * (1.0 - th * th)
    return dict(loss=loss, logits=logits, alpha=alpha, pooled=pooled, den=den, dh=dh, dph=dph, dqq=dph.sum((0, 1)), dv=torch.einsum("bt,bth->h", dscore, th),
                dvb=dscore.sum().reshape(1), dW=dlogits.t() @ pd, db=dlogits.sum(0), dscore=dscore)


def head_autograd_crit(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, keep, weight=None, eps=0.0, dloss=1.0):
    """the same quantities from autograd through oracle.multimodal.additive_attention + classifier + torch.nn.CrossEntropyLoss(weight, label_smoothing)
    with ignore_index at the labels outside [0, NL) -- the construction of support_unimodal_oracle.head_autograd (x = [ph | h], P = [I 0])"""
    dd = torch.float64
    H, NL = h.shape[-1], cls_w.shape[0]
    lv = dict(h=h, u=ph, qb=qq.reshape(-1), v=value_w.reshape(1, H), vb=value_b.reshape(1), W=cls_w, b=cls_b)
    lv = {k: t.detach().to(dd).clone().requires_grad_(True) for k, t in lv.items()}
    sd = {"a.P.weight": torch.cat((torch.eye(H, dtype=dd), torch.zeros(H, H, dtype=dd)), dim=1), "a.P.bias": torch.zeros(H, dtype=dd),
          "a.Q.weight": torch.zeros(H, 2 * H, dtype=dd), "a.Q.bias": lv["qb"], "a.query_vector": torch.zeros(2 * H, dtype=dd),
          "a.value.weight": lv["v"], "a.value.bias": lv["vb"]}
    x = torch.cat((lv["u"], lv["h"]), dim=-1)
    pooled = additive_attention(sd, "a.", x, mask.detach().to(dd))[:, H:]
    logits = (pooled * keep.detach().to(dd)) @ lv["W"].t() + lv["b"]
    lab = torch.where((labels >= 0) & (labels < NL), labels, torch.full_like(labels, -100))
    loss = torch.nn.CrossEntropyLoss(weight=None if weight is None else weight.detach().to(dd), label_smoothing=eps)(logits, lab)
    g = dict(zip(lv, torch.autograd.grad(loss * float(dloss), list(lv.values()))))
    return dict(loss=loss.detach(), logits=logits.detach(), dh=g["h"], dph=g["u"], dqq=g["qb"], dv=g["v"].reshape(-1), dvb=g["vb"], dW=g["W"], db=g["b"])


@contextlib.contextmanager
def loss_replaced(criterion):
    """inside the block tests/support_step_oracle.py and tests/support_unimodal_oracle.py compute criterion.reference where they say F.cross_entropy"""
    saved = (SO.F, UO.F)

    class _Functional:                                        # torch.nn.functional with one name replaced: every other F.* stays what it is
        cross_entropy = staticmethod(criterion.reference)

        def __getattr__(self, name):
            return getattr(saved[0], name)
    ns = _Functional()
    SO.F, UO.F = ns, ns
    try:
        yield
    finally:
        SO.F, UO.F = saved
