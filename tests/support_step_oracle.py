"""A training step assembled from oracle/ only: the independent side of tests/test_gpu_step_oracle.py.

Nothing of facialmmt_amd's arithmetic is imported here (the tests hand over state dicts, settings from config.default_args and
synth inputs): Swin in train mode with explicit DropPath multipliers (oracle.swin), softmax((logits + G) / tau) with the Gumbel
noise G as an argument, the literal frame-filter loop of train.py:75-114 (oracle.train_glue), the multimodal model with its
literal token-slicing loop (oracle.multimodal), cross-entropy, and the loops of train.py:15-41 (auxiliary) and :46-143 (target)
written out: accumulation, total norm, clip, plain SGD.  Everything is differentiable torch on leaf tensors, any dtype / device
(fp64 on the CPU is the reference; the same functions under bf16 autocast on the GPU are the "stock" yardstick).

Memory: the multimodal leaves are ~0.1 G values; `run` keeps gradients / parameter snapshots per step only when asked."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import swin as OS
from oracle.multimodal import multimodal_logits
from oracle.train_glue import select_frames_loop

BN_PRE = "swin.output_layer.3."


def leaves(module, dtype, device="cpu"):
    """state dict -> {name: tensor} in `dtype` (floating entries; the others as they are): parameters that require a gradient
    become leaves with requires_grad, buffers and frozen parameters do not"""
    trainable = {k for k, p in module.named_parameters() if p.requires_grad}
    out = {}
    for k, v in module.state_dict().items():
        t = v.detach().to(device)
        if t.is_floating_point():
            t = t.to(dtype).clone()
            if k in trainable:
                t.requires_grad_(True)
        else:
            t = t.clone()
        out[k] = t
    return out


def trainable(sd):
    return {k: v for k, v in sd.items() if v.requires_grad}


def standin_plm(mm_sd, key="roberta.emb.weight"):
    """synth.make_standin_plm restated on the leaf table (read at call time: an update of the table is seen): the embedding rows,
    zeroed where the attention mask is 0; a tuple like the Hugging Face encoders"""
    def plm(ids, attention_mask=None):
        h = mm_sd[key][ids]
        if attention_mask is not None:
            h = h * attention_mask.unsqueeze(-1).to(h.dtype)
        return (h,)
    return plm


def gumbel_softmax_given_noise(logits, gumbel, tau):
    """F.gumbel_softmax(logits, tau) (soft, last dim) with the noise handed in instead of drawn"""
    return torch.softmax((logits + gumbel) / tau, dim=-1)


def swin_preds(swin_sd, frames, gumbel, tau, drop_path_scales=None):
    """SwinForAffwildClassification.forward(is_trg_task=True), train mode (src/models.py:27-33)"""
    logits = OS.swin_affwild_logits(swin_sd, frames, training=True, drop_path_scales=drop_path_scales)
    return gumbel_softmax_given_noise(logits, gumbel, tau)


def loss_from_preds(preds, mm_sd, plm, cfg, batch):
    """train.py:75-131 behind Swin: importance filter + emotion concat, multimodal model, cross-entropy / accumulation count.
    Returns (loss, new vision mask, per-frame importance sum(p^2))."""
    (ids, attn_mask, sep_mask, audio, audio_mask, vision, vision_mask, labels, _frames, num_imgs, utt_idx) = batch
    importance = (preds * preds).sum(dim=1)
    vis, new_mask = select_frames_loop(preds, vision, vision_mask, [int(n) for n in num_imgs], cfg.FacialEmoImpor_threshold, cfg.num_labels)
    roberta = cfg.pretrainedtextmodel_path.split("/")[-1] == "roberta-large"
    logits = multimodal_logits(mm_sd, plm, cfg, ids, attn_mask, sep_mask, audio, audio_mask, vis, new_mask, utt_idx, roberta=roberta)
    loss = F.cross_entropy(logits, labels) / cfg.trg_accumulation_steps
    return loss, new_mask, importance


def target_step_loss(swin_sd, mm_sd, plm, cfg, batch, gumbel, drop_path_scales=None):
    """One target-task micro-step's loss.  Returns (loss, new vision mask, importance (sum F,), Gumbel-softmax output (sum F, 7))."""
    preds = swin_preds(swin_sd, batch[8], gumbel, cfg.tau, drop_path_scales)
    loss, new_mask, importance = loss_from_preds(preds, mm_sd, plm, cfg, batch)
    return loss, new_mask, importance, preds


def aux_step_loss(swin_sd, frames, labels, drop_path_scales=None, return_bn_stats=False):
    """train.py:15-41: Swin (train mode) -> logits, no Gumbel noise -> cross-entropy.  With return_bn_stats also the batch mean
    and the UNBIASED batch variance of the head's BatchNorm1d input (what nn.BatchNorm1d folds into its running statistics)."""
    logits = OS.swin_affwild_logits(swin_sd, frames, training=True, drop_path_scales=drop_path_scales)
    loss = F.cross_entropy(logits, labels)
    if not return_bn_stats:
        return loss
    with torch.no_grad():
        sd = {k[len("swin."):]: v for k, v in swin_sd.items() if k.startswith("swin.")}
        _, stages = OS.swin_forward_features(sd, frames, training=True, drop_path_scales=drop_path_scales, return_stages=True)
        x = OS.layer_norm(stages[-1], sd["output_layer.0.weight"], sd["output_layer.0.bias"])
        x = x.reshape(x.shape[0], -1) @ sd["output_layer.2.weight"].t() + sd["output_layer.2.bias"]
    return loss, (x.mean(0), x.var(0, unbiased=True))


def total_norm(grads):
    """clip_grad_norm_'s norm: the L2 norm of all gradients taken together"""
    return torch.sqrt(sum((g.detach() ** 2).sum() for g in grads))


def _clip_and_sgd(params, grads, clip, lr):
    """train.py:140-143 / :30-33 with plain SGD: total norm, scale by clip / (norm + 1e-6) when that is below 1, p -= lr g"""
    norm = total_norm([g for g in grads.values() if g is not None])
    coef = min(1.0, float(clip) / (float(norm) + 1e-6))
    with torch.no_grad():
        for k, g in grads.items():
            if g is not None:
                params[k].sub_(g * coef, alpha=lr)
    return float(norm)


def run(swin_sd, mm_sd, cfg, micro_batches, gumbels, drop_path_scales, lr, swin_grads=False, keep_grads=False, keep_params=False):
    """The loop TargetStep.__call__ performs, from train.py:46-143: one entry of micro_batches / gumbels / drop_path_scales per
    micro-step; gradients accumulate over cfg.trg_accumulation_steps micro-steps; on the last one the total norm over the
    MULTIMODAL parameters only, clip at cfg.clip, SGD with `lr`, gradients cleared.  Swin is never updated; its gradients are
    computed (and returned per micro-step) only with swin_grads.  Updates mm_sd's leaves in place.

    Returns {"micro": [{loss, mask, importance, preds, swin_grads?, unused, unused_swin}], "steps": [{norm, grads?, params?}]}."""
    plm = standin_plm(mm_sd)
    mm_leaves = trainable(mm_sd)
    sw_leaves = trainable(swin_sd) if swin_grads else {}
    acc = {k: None for k in mm_leaves}
    out = {"micro": [], "steps": []}
    for i, (batch, g, dps) in enumerate(zip(micro_batches, gumbels, drop_path_scales)):
        if swin_grads:
            loss, mask, imp, preds = target_step_loss(swin_sd, mm_sd, plm, cfg, batch, g, dps)
        else:                                               # nothing reads Swin's target-step gradients (train.py:20,33,140-143)
            with torch.no_grad():
                preds = swin_preds(swin_sd, batch[8], g, cfg.tau, dps)
            loss, mask, imp = loss_from_preds(preds, mm_sd, plm, cfg, batch)
        flat = torch.autograd.grad(loss, list(mm_leaves.values()) + list(sw_leaves.values()), allow_unused=True)
        got = dict(zip(mm_leaves, flat[:len(mm_leaves)]))               # (the two models share key names: classifier.weight)
        got_swin = dict(zip(sw_leaves, flat[len(mm_leaves):]))
        rec = {"loss": float(loss.detach()), "mask": mask.detach().clone(), "importance": imp.detach().clone(), "preds": preds.detach().clone(),
               "unused": [k for k in mm_leaves if got[k] is None], "unused_swin": [k for k in sw_leaves if got_swin[k] is None]}
        if swin_grads:
            rec["swin_grads"] = got_swin
        out["micro"].append(rec)
        for k in mm_leaves:
            if got[k] is not None:
                acc[k] = got[k] if acc[k] is None else acc[k] + got[k]
        if (i + 1) % cfg.trg_accumulation_steps == 0:
            step = {"grads": dict(acc) if keep_grads else None}
            step["norm"] = _clip_and_sgd(mm_leaves, acc, cfg.clip, lr)
            step["params"] = {k: v.detach().clone() for k, v in mm_leaves.items()} if keep_params else None
            out["steps"].append(step)
            acc = {k: None for k in mm_leaves}
    out["pending_grads"] = acc                              # an unfinished accumulation window (what .grad still holds)
    return out


def run_aux(swin_sd, cfg, micro_batches, drop_path_scales, lr, keep_grads=False, momentum=0.1):
    """The loop AuxStep.__call__ performs, from train.py:15-41: loss / cfg.aux_accumulation_steps, accumulate, on the last micro-step
    the total norm over the Swin model's parameters, clip at cfg.clip, SGD.  BatchNorm1d's running statistics are advanced per
    forward as nn.BatchNorm1d does (momentum 0.1, unbiased variance, num_batches_tracked + 1).  Updates swin_sd in place."""
    lv = trainable(swin_sd)
    acc = {k: None for k in lv}
    out = {"micro": [], "steps": []}
    for i, ((frames, labels), dps) in enumerate(zip(micro_batches, drop_path_scales)):
        loss, (mean, var) = aux_step_loss(swin_sd, frames, labels, dps, return_bn_stats=True)
        loss = loss / cfg.aux_accumulation_steps
        got = dict(zip(lv, torch.autograd.grad(loss, list(lv.values()), allow_unused=True)))
        with torch.no_grad():
            swin_sd[BN_PRE + "running_mean"].mul_(1.0 - momentum).add_(mean, alpha=momentum)
            swin_sd[BN_PRE + "running_var"].mul_(1.0 - momentum).add_(var, alpha=momentum)
            swin_sd[BN_PRE + "num_batches_tracked"] += 1
        out["micro"].append({"loss": float(loss.detach()), "unused": [k for k in lv if got[k] is None]})
        for k in lv:
            if got[k] is not None:
                acc[k] = got[k] if acc[k] is None else acc[k] + got[k]
        if (i + 1) % cfg.aux_accumulation_steps == 0:
            step = {"grads": dict(acc) if keep_grads else None}
            step["norm"] = _clip_and_sgd(lv, acc, cfg.clip, lr)
            out["steps"].append(step)
            acc = {k: None for k in lv}
    return out


def to_reference(batch, dtype=torch.float64, device="cpu"):
    """a device batch (bench.synth_batch's tuple) for the reference: floating entries in `dtype`, the rest unchanged, on `device`"""
    return tuple((t.detach().to(device).to(dtype) if t.is_floating_point() else t.detach().to(device)) if torch.is_tensor(t) else t for t in batch)


def grad_stats(g, r):
    """(max|g - r| / max|r|, relative L2, cosine) of a gradient against the reference's, in fp64 on the CPU"""
    g, r = g.detach().cpu().double().reshape(-1), r.detach().cpu().double().reshape(-1)
    rn = float(r.norm())
    return (float((g - r).abs().max() / r.abs().max()), float((g - r).norm() / rn), float((g @ r) / (g.norm() * rn + 1e-300)))
