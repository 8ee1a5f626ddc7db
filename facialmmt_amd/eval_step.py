"""Evaluation on the HIP path: the reference's `multimodal_evaluate` / `unimodal_evaluate` (train.py:154-243, 275-292) and `eval_meld`
(utils/eval_metrics.py:16-28) without their per-batch host synchronisations.

One evaluation batch is: Swin features -> target-task head + Gumbel-softmax + importance (ONE launch, ops.emotion_head) -> frame filter (one
launch, train_step.select_frames) -> multimodal forward -> loss / argmax / confusion matrix accumulated ON THE DEVICE (one launch,
ops.eval_accumulate).  `EvalStep` issues that launch by launch; `GraphedEvalStep` captures it once as a single HIP graph (text encoder as the one
fork branch) and replays it per batch.  `MeldMetrics` owns the accumulators; the only device-to-host copy of a split is `MeldMetrics.result()`.

Departures from the reference, on purpose:
  * the loss is `sum of row losses / rows`, exact for any batch sizes; the reference multiplies each batch MEAN by args.trg_batch_size and divides
    by the split size, which is the same number when every batch is full and over-weights a short last batch otherwise;
  * `f1_per_class` always has num_labels entries (0 for a class that occurs neither as label nor as prediction); scikit-learn's
    `f1_score(average=None)` without `labels=`, as the reference calls it, returns fewer values when a class is absent from both vectors;
  * `gumbel="off"` (not the default) evaluates without the Gumbel noise: the reference keeps F.gumbel_softmax in evaluation too, so its score is a
    random variable of the generator state; "off" is the deterministic variant."""
from __future__ import annotations

import contextlib
import types

import numpy as np
import torch

from . import ops
from .train_step import _KEEP_GRAPHS, _ops_pinned_scope, _pin_shadows, capture_window, distinct_stream, fused_inference, select_frames

EMOTIONS = ("Neutral", "Surprise", "Fear", "Sadness", "Joy", "Disgust", "Anger")      # class order of eval_meld (utils/eval_metrics.py:27)


# ------------------------------------------------------------------------------------------------ host formulas
def confusion_matrix(pred, truth, num_labels: int) -> np.ndarray:
    """[label][prediction] counts (int64) of two integer vectors; labels outside [0, num_labels) are ignored"""
    pred, truth = np.asarray(pred).astype(np.int64).ravel(), np.asarray(truth).astype(np.int64).ravel()
    ok = (truth >= 0) & (truth < num_labels)
    conf = np.zeros((num_labels, num_labels), dtype=np.int64)
    np.add.at(conf, (truth[ok], pred[ok]), 1)
    return conf


def f1_from_confusion(conf):
    """(weighted F1, per-class F1) of a [label][prediction] count matrix: f1_c = 2 tp_c / (support_c + predicted_c), 0 where the denominator
    is 0; weighted by support.  Equal to sklearn.metrics.f1_score(average='weighted') and (average=None, labels=range(NL))."""
    conf = np.asarray(conf, dtype=np.float64)
    tp = np.diag(conf)
    support, predicted = conf.sum(axis=1), conf.sum(axis=0)
    den = support + predicted
    f1 = np.divide(2.0 * tp, den, out=np.zeros_like(tp), where=den > 0)
    total = support.sum()
    weighted = float((f1 * support).sum() / total) if total > 0 else 0.0
    return weighted, f1


def eval_meld(results, truths, test=False):
    """utils/eval_metrics.py:16-28 with the reference's signature: weighted F1 of argmax(results) against truths; `test=True` also prints the
    per-class scores.  Through the confusion-matrix formulas above: no scikit-learn needed.  The printed vector has one entry per column of
    `results` (see the module docstring)."""
    r = results.detach().float().cpu().numpy() if torch.is_tensor(results) else np.asarray(results)
    t = truths.detach().cpu().numpy() if torch.is_tensor(truths) else np.asarray(truths)
    weighted, f1 = f1_from_confusion(confusion_matrix(np.argmax(r, axis=1), t, r.shape[1]))
    if test:
        print('**TEST** | f1 on each class (Neutral, Surprise, Fear, Sadness, Joy, Disgust, Anger): \n', f1)
    return weighted


class MeldMetrics:
    """Loss sum, row count and confusion matrix of a split, accumulated on the device: `update` is one launch and no synchronisation,
    `result()` one device-to-host copy of 2 + num_labels^2 numbers (51 for MELD's 7 classes)."""

    def __init__(self, num_labels: int = 7, device="cuda"):
        if not 1 <= num_labels <= 8:
            raise ValueError("MeldMetrics: 1..8 classes (fmmt_eval_accumulate)")
        self.num_labels = num_labels
        self.acc = torch.zeros(2 + num_labels * num_labels, dtype=torch.int64, device=device)

    def reset(self):
        self.acc.zero_()                                      # in place: a captured graph keeps writing to this tensor

    def update(self, logits, labels, logits_out=None, out_offset=0, pred=False):
        """logits (B, num_labels), labels (B,) with negative = ignored (rows a caller padded); B <= 1024"""
        return ops.eval_accumulate(logits, labels, self.acc, logits_out, out_offset, pred=pred)

    @staticmethod
    def summarise(host: np.ndarray, num_labels: int):
        """the host half of result(): `host` = the 2 + NL^2 int64 words as copied from the device"""
        host = np.ascontiguousarray(host, dtype=np.int64)
        loss_sum = float(host[:1].view(np.float64)[0])
        count = int(host[1])
        conf = host[2:].reshape(num_labels, num_labels).copy()
        weighted, f1 = f1_from_confusion(conf)
        return types.SimpleNamespace(avg_loss=loss_sum / count if count else float("nan"), weighted_f1=weighted, f1_per_class=f1, confusion=conf,
                                     count=count, loss_sum=loss_sum)

    def result(self):
        """avg_loss (= loss sum / rows), weighted_f1, f1_per_class (always num_labels values, order EMOTIONS), confusion [label][prediction], count"""
        return self.summarise(self.acc.cpu().numpy(), self.num_labels)


# ------------------------------------------------------------------------------------------------ one batch
class _eval_mode:
    """both models in eval() for the length of the block; every module gets the mode it had back"""

    def __init__(self, *models):
        self.models = models

    def __enter__(self):
        self.was = [(m, m.training) for model in self.models for m in model.modules() if m.training]
        for m, _ in self.was:
            m.training = False
        return self

    def __exit__(self, *exc):
        for m, t in self.was:
            m.training = t
        return False


def _autocast(dtype):
    return torch.autocast("cuda", dtype=dtype) if dtype is not None else contextlib.nullcontext()


def _forward_batch(swin, mm, args, batch, metrics, autocast_dtype, sample, text_stream=None, shadows=None):
    """the launches of one evaluation batch on the current stream (text encoder on `text_stream`, forked and joined, when given)"""
    (ids, attn_mask, sep_mask, audio, audio_mask, vision_inputs, vision_mask, labels, frames, num_imgs, utt_idx) = batch
    dev = frames.device
    main = torch.cuda.current_stream()
    if shadows is not None:
        shadows.refresh()
    utt = torch.as_tensor(utt_idx, device=dev)

    def text():
        with _autocast(autocast_dtype):
            return mm.text_branch(ids, attn_mask, sep_mask, utt)
    if text_stream is not None:
        ev = torch.cuda.Event()
        ev.record(main)
        text_stream.wait_event(ev)
        with torch.cuda.stream(text_stream):
            text_feat, text_mask = text()
    else:
        text_feat, text_mask = text()
    feats = swin.swin(frames)
    noise = ops.gumbel_noise(feats.shape[0], swin.num_labels, dev) if sample else None
    preds, importance = ops.emotion_head(feats, swin.linear, swin.classifier, swin.tau, noise)
    vis_concat, new_mask = select_frames(preds, vision_inputs, vision_mask, torch.as_tensor(num_imgs, device=dev), args.FacialEmoImpor_threshold)
    if text_stream is not None:
        main.wait_stream(text_stream)
        text_feat.record_stream(main)
        text_mask.record_stream(main)
    with _autocast(autocast_dtype):
        logits = mm.fusion_branch(text_feat, text_mask, audio, audio_mask, vis_concat, new_mask)
    metrics.update(logits, torch.as_tensor(labels, device=dev))
    return logits, new_mask, importance


def _check_gumbel(gumbel):
    if gumbel not in ("sample", "off"):
        raise ValueError("gumbel: 'sample' (the reference: noise in evaluation too) or 'off' (deterministic)")
    return gumbel == "sample"


class EvalStep:
    """One batch of multimodal_evaluate (train.py:154-243), launch by launch, under no_grad with both models in eval(): Swin features ->
    ops.emotion_head -> select_frames -> multimodal forward -> MeldMetrics.update.  Same batch tuple as train_step.TargetStep.  Returns
    (logits, kept-frame mask); the models are back in their previous train / eval mode afterwards.  Inside the step the fused forwards of
    train_step.fuse_text_encoder run (train_step.fused_inference)."""

    def __init__(self, swin_model, multimodal_model, args, autocast_dtype=None, gumbel="sample", metrics=None):
        self.sample = _check_gumbel(gumbel)
        self.swin, self.mm, self.args, self.autocast_dtype = swin_model, multimodal_model, args, autocast_dtype
        self.metrics = metrics if metrics is not None else MeldMetrics(swin_model.num_labels, next(multimodal_model.parameters()).device)
        self.importance = None

    def __call__(self, batch):
        with torch.no_grad(), _eval_mode(self.swin, self.mm), fused_inference():
            logits, new_mask, self.importance = _forward_batch(self.swin, self.mm, self.args, batch, self.metrics, self.autocast_dtype, self.sample)
        return logits, new_mask


class GraphedEvalStep:
    """EvalStep's launches captured ONCE as a single HIP graph for the sample batch's shapes -- the text encoder as the one fork branch, the
    layout of GraphedTargetStep's graph A -- and replayed per batch: inputs are copied into static buffers, the metric update is inside the
    graph.  A batch of other shapes (the short last batch of a split) runs through an EvalStep on the same MeldMetrics; rows a caller padded
    carry a negative label.  The graph has a memory pool of its own and writes nothing the training graphs read except the bf16 weight
    shadows, which it rebuilds from the current parameters at its head exactly as they do.  The returned logits / mask are the graph's static
    outputs: clone what must survive the next call."""

    def __init__(self, swin_model, multimodal_model, args, batch, autocast_dtype=None, gumbel="sample", metrics=None, overlap_text=True, warmup_iters=2):
        import os
        if os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "") != "0":
            raise RuntimeError("GraphedEvalStep: DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 must be in the environment before the HIP runtime "
                               "initialises (see facialmmt_amd/__init__.py)")
        self.sample = _check_gumbel(gumbel)
        self.swin, self.mm, self.args, self.autocast_dtype = swin_model, multimodal_model, args, autocast_dtype
        dev = batch[8].device
        self.metrics = metrics if metrics is not None else MeldMetrics(swin_model.num_labels, dev)
        self.eager = EvalStep(swin_model, multimodal_model, args, autocast_dtype, gumbel, self.metrics)
        self.static = [t.clone() if torch.is_tensor(t) else torch.as_tensor(t, device=dev) for t in batch]
        cap = distinct_stream(dev)
        self.text_stream = distinct_stream(dev, (cap,)) if overlap_text else None
        scratch = MeldMetrics(self.metrics.num_labels, dev)                    # the warm-up passes count into this one
        rng = torch.cuda.get_rng_state(dev)
        with torch.no_grad(), _eval_mode(self.swin, self.mm), fused_inference():
            cap.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cap):
                for _ in range(max(1, warmup_iters)):                          # lazy initialisations, the shadow cache the pins are made from
                    _forward_batch(self.swin, self.mm, args, self.static, scratch, autocast_dtype, self.sample)
            torch.cuda.current_stream().wait_stream(cap)
            torch.cuda.synchronize(dev)
            torch.cuda.set_rng_state(rng, dev)
            self.shadows = _pin_shadows([self.swin, self.mm])
            self.graph = torch.cuda.CUDAGraph()
            with capture_window(), _ops_pinned_scope(self.shadows):
                with torch.cuda.graph(self.graph, stream=cap):
                    self.logits, self.new_mask, self.importance = _forward_batch(self.swin, self.mm, args, self.static, self.metrics, autocast_dtype,
                                                                                 self.sample, self.text_stream, self.shadows)
        _KEEP_GRAPHS.append((self.graph,))

    def __call__(self, batch):
        if len(batch) != len(self.static):
            raise ValueError(f"GraphedEvalStep: batch of {len(batch)} entries, captured with {len(self.static)}")
        srcs = [s if torch.is_tensor(s) else torch.as_tensor(s) for s in batch]
        if any(tuple(s.shape) != tuple(d.shape) for s, d in zip(srcs, self.static)):
            return self.eager(batch)
        with torch.no_grad():
            for dst, src in zip(self.static, srcs):
                if dst is not src:
                    dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self.logits, self.new_mask


class UnimodalEvalStep:
    """One batch of unimodal_evaluate (train.py:275-292, choice_modality 'V'): meld_utt_transformer forward -> MeldMetrics.update.
    batch = (modality_feature, utterance_mask, labels); returns the logits."""

    def __init__(self, model, args, metrics=None):
        self.model, self.args = model, args
        self.metrics = metrics if metrics is not None else MeldMetrics(args.num_labels, next(model.parameters()).device)

    def __call__(self, batch):
        feature, mask, labels = batch
        with torch.no_grad(), _eval_mode(self.model):
            logits = self.model(feature, mask)
            self.metrics.update(logits, torch.as_tensor(labels, device=logits.device))
        return logits


def evaluate(step, loader):
    """A whole split through `step` (EvalStep / GraphedEvalStep / UnimodalEvalStep): (avg_loss, results, truths) as multimodal_evaluate /
    unimodal_evaluate return them -- results = the concatenated logits, truths = the concatenated labels, both left on the device.  The one
    host synchronisation is the final copy of the accumulators; step.metrics.result() afterwards has the F1 scores of the same split.
    avg_loss = loss sum / rows (module docstring)."""
    step.metrics.reset()
    results, truths = [], []
    for batch in loader:
        out = step(batch)
        logits = out[0] if isinstance(out, tuple) else out
        labels = batch[2] if len(batch) == 3 else batch[7]
        results.append(logits.detach().float().clone())       # a graphed step hands out its static buffer
        truths.append(torch.as_tensor(labels, device=logits.device).clone())
    r = step.metrics.result()
    return r.avg_loss, torch.cat(results), torch.cat(truths)
