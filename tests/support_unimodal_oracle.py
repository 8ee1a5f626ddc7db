"""The V-only training step assembled from oracle/ only, and the pooling head restated by hand: the independent side of
tests/test_gpu_pool_head.py and tests/test_gpu_unimodal_step.py (validated in tests/test_unimodal_oracle_cpu.py).

Nothing of facialmmt_amd's arithmetic is imported: the tests hand over state dicts, settings from config.default_args and synth inputs.
  * step_loss / run: oracle.multimodal.meld_utt_logits, F.cross_entropy and the loops of train.py:245-273 written out -- loss / accumulation
    count, gradients accumulated, on the window's last micro-step the total norm over the model's parameters, clip, plain SGD.  All dropout
    probabilities are 0 (the oracle is the eval-mode forward).  Differentiable torch on leaf tensors, any dtype / device.
  * head_reference: the formulas of csrc/pool_head.hip's header in fp64, forward and backward written out (no autograd), with a given keep mask.
  * head_autograd: the same quantities from autograd through oracle.multimodal.additive_attention + classifier + cross-entropy.  That function
    pools the tensor it scores; the two roles are separated by feeding it x = [ph | h] (2H channels) with P = [I 0] (so P x = ph), a classifier
    that reads only the h half, and Q's bias as the leaf behind qq: d(ph), d(h) and d(qq) then fall out of one backward unmixed."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.multimodal import additive_attention, meld_utt_logits

from tests.support_step_oracle import _clip_and_sgd, grad_stats, leaves, total_norm, trainable      # noqa: F401  (re-exported for the tests)


def step_loss(sd, cfg, feature, mask, labels):
    """one micro-step's loss, train.py:255-257"""
    return F.cross_entropy(meld_utt_logits(sd, cfg, feature, mask), labels) / cfg.trg_accumulation_steps


def run(sd, cfg, micro_batches, lr, keep_grads=False, keep_params=False):
    """The loop UnimodalStep.__call__ performs, from train.py:245-273; updates sd's leaves in place.
    Returns {"micro": [{loss, logits, grads?, unused}], "steps": [{norm, grads?, params?}], "pending_grads"}."""
    lv = trainable(sd)
    acc = {k: None for k in lv}
    out = {"micro": [], "steps": []}
    for i, (feature, mask, labels) in enumerate(micro_batches):
        logits = meld_utt_logits(sd, cfg, feature, mask)
        loss = F.cross_entropy(logits, labels) / cfg.trg_accumulation_steps
        got = dict(zip(lv, torch.autograd.grad(loss, list(lv.values()), allow_unused=True)))
        out["micro"].append({"loss": float(loss.detach()), "logits": logits.detach().clone(), "grads": got if keep_grads else None,
                             "unused": [k for k in lv if got[k] is None]})
        for k in lv:
            if got[k] is not None:
                acc[k] = got[k] if acc[k] is None else acc[k] + got[k]
        if (i + 1) % cfg.trg_accumulation_steps == 0:
            step = {"grads": dict(acc) if keep_grads else None}
            step["norm"] = _clip_and_sgd(lv, acc, cfg.clip, lr)
            step["params"] = {k: v.detach().clone() for k, v in lv.items()} if keep_params else None
            out["steps"].append(step)
            acc = {k: None for k in lv}
    out["pending_grads"] = acc
    return out


def head_reference(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, keep, dloss=1.0):
    """fp64, by hand: score_t = v . tanh(ph_t + qq) + v_b (-inf where mask == 0); alpha = softmax_t; pooled = sum_t alpha_t h_t;
    logits = W (keep * pooled) + b; loss = mean_b(logsumexp - logits[label]); and the backward of csrc/pool_head.hip's header:
    d(logits) = dloss / B (softmax - onehot); d(pooled) = keep * W^T d(logits); d(score_t) = alpha_t (d(pooled) . h_t - d(pooled) . pooled);
    dh_t = alpha_t d(pooled); dph_t = d(score_t) v (1 - tanh^2); dqq = sum dph; dv = sum d(score_t) tanh; dv_b = sum d(score_t)."""
    dd = torch.float64
    h, ph, qq, v, vb, mask, W, b, keep = (t.detach().to(dd) for t in (h, ph, qq.reshape(-1), value_w.reshape(-1), value_b.reshape(-1), mask, cls_w, cls_b, keep))
    B = h.shape[0]
    th = torch.tanh(ph + qq)
    score = th @ v + vb
    score = torch.where(mask == 0, torch.full_like(score, float("-inf")), score)
    m = score.max(dim=1, keepdim=True).values
    e = torch.exp(score - m)
    alpha = e / e.sum(dim=1, keepdim=True)
    pooled = torch.einsum("bt,bth->bh", alpha, h)
    pd = pooled * keep
    logits = pd @ W.t() + b
    mx = logits.max(dim=1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(logits - mx).sum(dim=1, keepdim=True))).squeeze(1)
    onehot = torch.zeros_like(logits)
    onehot[torch.arange(B), labels] = 1.0
    loss = (lse - (logits * onehot).sum(1)).sum() / B
    dlogits = float(dloss) / B * (torch.exp(logits - lse[:, None]) - onehot)
    dpooled = keep * (dlogits @ W)
    dscore = alpha * (torch.einsum("bh,bth->bt", dpooled, h) - (dpooled * pooled).sum(1, keepdim=True))
    dh = alpha[:, :, None] * dpooled[:, None, :]
    dph = dscore[:, :, None] * v * (1.0 - th * th)
    return dict(loss=loss, logits=logits, alpha=alpha, pooled=pooled, dh=dh, dph=dph, dqq=dph.sum((0, 1)), dv=torch.einsum("bt,bth->h", dscore, th),
                dvb=dscore.sum().reshape(1), dW=dlogits.t() @ pd, db=dlogits.sum(0), dscore=dscore)


def head_autograd(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, keep, dloss=1.0):
    """the same dictionary (without pooled / dscore) from autograd through oracle.multimodal.additive_attention (module docstring)"""
    dd = torch.float64
    H = h.shape[-1]
    lv = dict(h=h, u=ph, qb=qq.reshape(-1), v=value_w.reshape(1, H), vb=value_b.reshape(1), W=cls_w, b=cls_b)
    lv = {k: t.detach().to(dd).clone().requires_grad_(True) for k, t in lv.items()}
    sd = {"a.P.weight": torch.cat((torch.eye(H, dtype=dd), torch.zeros(H, H, dtype=dd)), dim=1), "a.P.bias": torch.zeros(H, dtype=dd),
          "a.Q.weight": torch.zeros(H, 2 * H, dtype=dd), "a.Q.bias": lv["qb"], "a.query_vector": torch.zeros(2 * H, dtype=dd),
          "a.value.weight": lv["v"], "a.value.bias": lv["vb"]}
    x = torch.cat((lv["u"], lv["h"]), dim=-1)
    mask = mask.detach().to(dd)
    pooled = additive_attention(sd, "a.", x, mask)[:, H:]
    logits = (pooled * keep.detach().to(dd)) @ lv["W"].t() + lv["b"]
    loss = F.cross_entropy(logits, labels)
    g = dict(zip(lv, torch.autograd.grad(loss * float(dloss), list(lv.values()))))
    with torch.no_grad():
        sc = (torch.tanh(lv["u"] + lv["qb"]) @ lv["v"].reshape(-1) + lv["vb"]).masked_fill(mask == 0., float("-inf"))
        alpha = torch.softmax(sc, -1)
    return dict(loss=loss.detach(), logits=logits.detach(), alpha=alpha, dh=g["h"], dph=g["u"], dqq=g["qb"], dv=g["v"].reshape(-1), dvb=g["vb"],
                dW=g["W"], db=g["b"])


def head_inputs(B, L, H, NL, seed, lengths=None):
    """hash-seeded inputs of the head at one shape, fp32 on the CPU: ragged masks (row 0 fully valid, the last row exactly one valid token when
    B > 1, the others in between), labels covering all classes when B allows.  ph is drawn at tanh's working range."""
    from facialmmt_amd import synth
    h = synth.tensor("ph_h", (B, L, H), seed=seed)
    ph = synth.tensor("ph_ph", (B, L, H), seed=seed + 1, lo=-1.5, hi=1.5)
    qq = synth.tensor("ph_qq", (H,), seed=seed + 2, lo=-0.5, hi=0.5)
    vw = synth.tensor("ph_v", (H,), seed=seed + 3, lo=-0.2, hi=0.2)
    vb = synth.tensor("ph_vb", (1,), seed=seed + 4)
    W = synth.tensor("ph_W", (NL, H), seed=seed + 5, lo=-0.1, hi=0.1)
    b = synth.tensor("ph_b", (NL,), seed=seed + 6, lo=-0.1, hi=0.1)
    if lengths is None:
        lengths = [L] + [max(1, (L * (3 + 5 * i)) // (5 * B + 3)) for i in range(1, B)]
        if B > 1:
            lengths[-1] = 1
    mask = torch.zeros(B, L)
    for i, n in enumerate(lengths):
        mask[i, :n] = 1
    labels = (torch.arange(B) * 3 + seed) % NL
    return dict(h=h, ph=ph, qq=qq, value_w=vw, value_b=vb, mask=mask, cls_w=W, cls_b=b, labels=labels), lengths
