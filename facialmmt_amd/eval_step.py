"""Evaluation on the HIP path: the reference's `multimodal_evaluate` / `unimodal_evaluate` (train.py:154-243, 275-292) and `eval_meld`
(utils/eval_metrics.py:16-28) without their per-batch host synchronisations.

One evaluation batch is: Swin features -> target-task head + Gumbel-softmax + importance (ONE launch, ops.emotion_head) -> frame filter (one
launch, train_step.select_frames) -> multimodal forward -> loss / argmax / confusion matrix accumulated ON THE DEVICE (one launch,
ops.eval_accumulate).  `EvalStep` issues that launch by launch; `GraphedEvalStep` captures it once as a single HIP graph (text encoder as the one
fork branch) and replays it per batch.  `MeldMetrics` owns the accumulators; the only device-to-host copy of a split is `MeldMetrics.result()`.

Real MELD batches are ragged: the loader pads the frames to (B, Lv, ...) and says how many are real (utils/dataset.py:275-292), and the compact
tensor the reference concatenates (train.py:167-178) has another first dimension in almost every batch.  `frame_capacity` on either step takes the
padded batch instead: ops.pack_frames moves the real frames to the front of a fixed number of rows on the device, Swin and the head run on all of
them, and the frame filter is told how many are real.  `GraphedEvalStep` captures one graph per capacity ("bucket") and replays the smallest that
holds the batch; `MeldMetrics(collect_rows=...)` keeps the split's logits and labels at a device-held row index (ops.eval_accumulate_at), so
`evaluate` clones nothing per batch.

Departures from the reference, on purpose:
  * the loss is `sum of row losses / rows`, exact for any batch sizes; the reference multiplies each batch MEAN by args.trg_batch_size and divides
    by the split size, which is the same number when every batch is full and over-weights a short last batch otherwise;
  * `f1_per_class` always has num_labels entries (0 for a class that occurs neither as label nor as prediction); scikit-learn's
    `f1_score(average=None)` without `labels=`, as the reference calls it, returns fewer values when a class is absent from both vectors;
  * `gumbel="off"` (not the default) evaluates without the Gumbel noise: the reference keeps F.gumbel_softmax in evaluation too, so its score is a
    random variable of the generator state; "off" is the deterministic variant.  With `frame_capacity` the noise is drawn for every row of the
    capacity, so under "sample" the numbers a given seed hands to a given frame -- and with them the score -- also depend on the capacity, i.e.
    on which bucket a batch was replayed in: one more way in which that score is a draw, not a constant.  "off" does not depend on the bucket.
    The same holds for a split SHARDED over ranks (`evaluate(sharded=True)`, parallel.eval_shard): every rank draws from its own generator, so the
    sharded score under "sample" is another draw than the single-rank one; under "off" it does not depend on the number of ranks.

A short last batch (MELD's validation and test splits both end short at 4 per batch, and of a sharded split the last non-empty rank always does):
`GraphedEvalStep(pad_rows=True)` pads it to the captured rows (train_step.pad_target_batch) and replays it; a device word tells the collecting metric
update how many rows exist (ops.eval_accumulate_rows).  Several ranks: each evaluates a contiguous block of whole batches, `MeldMetrics.gather_merge`
all-gathers accumulators and rows and ops.eval_merge makes the one split of them on the device, in dataset order, the same on every rank."""
from __future__ import annotations

import types

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .graph_capture import _KEEP_GRAPHS, _autocast, capture_window, check_static_shapes, copy_into_static, distinct_stream, require_packet_capture_off, warmup_undone
from .train_step import _clamp_counts, _pin_shadows, check_frame_total, frame_buckets, fused_inference, pad_target_batch, pick_bucket, select_frames  # noqa: F401

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
    `result()` one device-to-host copy of 2 + num_labels^2 numbers (51 for MELD's 7 classes).

    `collect_rows` (None: nothing below exists): the metrics also COLLECT the split -- `results` (collect_rows, num_labels) fp32, `truths`
    (collect_rows,) int64 and `cursor`, one int64 device word -- through ops.eval_accumulate_at: every update stores its rows at the cursor and
    advances it on the device, so the update inside a captured graph fills the buffers front to back.  Rows behind collect_rows are counted and
    not kept; `collected()` then raises.  The cursor lives behind the accumulators in one allocation: one copy brings both to the host.

    `gather_merge()` (collecting metrics only) makes the whole split of the shards W ranks evaluated: `merged`, a MeldMetrics(collect_rows =
    W * collect_rows) built on first use, whose result() / collected() are the split's; this object stays the rank's own."""

    def __init__(self, num_labels: int = 7, device="cuda", collect_rows=None):
        if not 1 <= num_labels <= 8:
            raise ValueError("MeldMetrics: 1..8 classes (fmmt_eval_accumulate)")
        self.num_labels = num_labels
        self.collect_rows = None if collect_rows is None else int(collect_rows)
        n = 2 + num_labels * num_labels
        if self.collect_rows is None:
            self.acc = torch.zeros(n, dtype=torch.int64, device=device)
            return
        if self.collect_rows < 0:
            raise ValueError("MeldMetrics: collect_rows is a number of rows")
        self.words = torch.zeros(n + 1, dtype=torch.int64, device=device)          # accumulators | cursor
        self.acc, self.cursor = self.words[:n], self.words[n:]
        self.results = torch.zeros(self.collect_rows, num_labels, dtype=torch.float32, device=device)
        self.truths = torch.zeros(self.collect_rows, dtype=torch.int64, device=device)
        self.merged = None

    def reset(self):
        (self.acc if self.collect_rows is None else self.words).zero_()          # in place: a captured graph keeps writing to this tensor

    def update(self, logits, labels, logits_out=None, out_offset=0, pred=False, n_rows=None):
        """logits (B, num_labels), labels (B,) with negative = ignored (rows a caller padded); B <= 1024.  `n_rows` (a batch padded to B rows): one
        int32 device word, the rows that exist -- collecting metrics store and count those alone (ops.eval_accumulate_rows); metrics that do not
        collect need no word, the padded rows' negative labels keep them out of every sum."""
        if self.collect_rows is None:
            return ops.eval_accumulate(logits, labels, self.acc, logits_out, out_offset, pred=pred)
        if logits_out is not None or pred:
            raise ValueError("MeldMetrics(collect_rows=...): the rows go to `results` / `truths` at the cursor; logits_out / pred are the other mode")
        if n_rows is not None:
            return ops.eval_accumulate_rows(logits, labels, self.acc, self.cursor, n_rows, self.results, self.truths)
        return ops.eval_accumulate_at(logits, labels, self.acc, self.cursor, self.results, self.truths)

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

    @staticmethod
    def collected_count(host: np.ndarray, collect_rows: int) -> int:
        """the host half of collected(): `host` = the 2 + NL^2 + 1 int64 words as copied from the device, the cursor last.  The rows kept, or
        ValueError when more rows went through update() than the buffers hold"""
        cursor = int(np.asarray(host).ravel()[-1])
        if cursor > collect_rows:
            raise ValueError(f"MeldMetrics: {cursor} rows went through update(), the buffers were built for collect_rows={collect_rows}: "
                             f"the rows behind it were counted and not kept")
        return max(cursor, 0)

    def _host(self):
        return (self.acc if self.collect_rows is None else self.words).cpu().numpy()

    def result(self):
        """avg_loss (= loss sum / rows), weighted_f1, f1_per_class (always num_labels values, order EMOTIONS), confusion [label][prediction], count"""
        return self.summarise(self._host()[:2 + self.num_labels ** 2], self.num_labels)

    def collected(self, host=None):
        """(results[:n], truths[:n]), n = the rows updated since reset(): views of the buffers, valid until the next reset() / update().  `host`:
        the words a caller already copied (evaluate() reads cursor and accumulators in one copy)"""
        if self.collect_rows is None:
            raise ValueError("MeldMetrics was built without collect_rows: nothing is collected")
        n = self.collected_count(self._host() if host is None else host, self.collect_rows)
        return self.results[:n], self.truths[:n]

    def gather_merge(self, process_group=None):
        """The shards of all ranks -> `self.merged`, the whole split, the same on every rank; returns it.  Every rank evaluated a contiguous block
        of the dataset (parallel.eval_shard) into metrics of the same collect_rows (parallel.eval_collect_rows).  First one small all-gather of
        `words` with collect_rows behind them: a rank built with another collect_rows raises ValueError on EVERY rank, before the large gather.
        Then `results` and `truths` are gathered and ops.eval_merge (one launch) lays rank r's first cursor_r rows behind those of the ranks in
        front of it and adds the accumulators, the loss sums in rank order.  gloo gathers host tensors, RCCL device tensors
        (parallel.replicas_agree); nothing is copied to the host on RCCL, and nothing synchronises there.  World size 1, or no process group: no
        collective, `merged` is filled by the same kernel with W = 1.  A shard that overflowed its buffers makes merged.collected() raise."""
        if self.collect_rows is None:
            raise ValueError("MeldMetrics.gather_merge: collecting metrics only (collect_rows=...): the merged split is made of the ranks' rows")
        dev, nl, cap = self.words.device, self.num_labels, self.collect_rows
        world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        if world > 64:
            raise ValueError("MeldMetrics.gather_merge: at most 64 ranks (fmmt_eval_merge)")
        if world == 1:
            words, results, truths = self.words[None], self.results[None], self.truths[None]
        else:
            on_host = dist.get_backend(process_group) != "nccl"                # gloo gathers host tensors only; RCCL device tensors only

            def gather(t):                                                     # (world,) + t.shape, rank order
                t = t.cpu() if on_host else t
                got = [torch.empty_like(t) for _ in range(world)]
                dist.all_gather(got, t, group=process_group)
                return torch.stack(got)
            heads = gather(torch.cat((self.words, torch.tensor([cap], dtype=torch.int64, device=dev))))
            caps = heads[:, -1].tolist()                                       # on RCCL a host read of W words: the check comes before the large gather
            if any(c != caps[0] for c in caps):
                raise ValueError(f"MeldMetrics.gather_merge: every rank builds its metrics with the same collect_rows (parallel.eval_collect_rows), "
                                 f"the ranks hold {caps}")
            words = heads[:, :-1].contiguous().to(dev)
            results, truths = gather(self.results).to(dev), gather(self.truths).to(dev)
        if self.merged is None or self.merged.collect_rows != world * cap:
            self.merged = MeldMetrics(nl, dev, collect_rows=world * cap)
        ops.eval_merge(words, results, truths, self.merged.words, self.merged.results, self.merged.truths)
        return self.merged


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


def _check_padded_frames(frames, vision_inputs):
    if frames.dim() < 3 or tuple(frames.shape[:2]) != tuple(vision_inputs.shape[:2]):
        raise ValueError(f"frame_capacity: `frames` as the loader pads them, (B, Lv, ...) = {tuple(vision_inputs.shape[:2])} + the frame's shape, "
                         f"got {tuple(frames.shape)} (the compact (sum num_imgs, ...) tensor belongs to a step without frame_capacity)")


def _forward_batch(swin, mm, args, batch, metrics, autocast_dtype, sample, text_stream=None, shadows=None, frame_capacity=None, n_rows=None):
    """the launches of one evaluation batch on the current stream (text encoder on `text_stream`, forked and joined, when given).  With a
    `frame_capacity` the batch's frames are the padded (B, Lv, ...) tensor: checked on the host where num_imgs lives there, packed on the device,
    and everything up to the frame filter runs on `frame_capacity` rows.  `n_rows`: the device word of a batch padded in its rows, handed to the
    metric update.  Returns (logits, kept-frame mask, importance, frame counts or None)."""
    (ids, attn_mask, sep_mask, audio, audio_mask, vision_inputs, vision_mask, labels, frames, num_imgs, utt_idx) = batch
    dev = frames.device
    counts = None
    if frame_capacity is not None:                           # both checks read host values only and come before the first launch
        _check_padded_frames(frames, vision_inputs)
        check_frame_total(num_imgs, frames.shape[1], frame_capacity)
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
    n_imgs = torch.as_tensor(num_imgs, device=dev)
    if frame_capacity is not None:
        # in eval() the embedding head's BatchNorm normalises with its running statistics, row by row: Swin needs no row count, the filter does
        frames, counts = ops.pack_frames(frames, n_imgs, frame_capacity)
    feats = swin.swin(frames)
    noise = ops.gumbel_noise(feats.shape[0], swin.num_labels, dev) if sample else None
    preds, importance = ops.emotion_head(feats, swin.linear, swin.classifier, swin.tau, noise)
    vis_concat, new_mask = select_frames(preds, vision_inputs, vision_mask, n_imgs, args.FacialEmoImpor_threshold, n_valid=counts)
    if text_stream is not None:
        main.wait_stream(text_stream)
        text_feat.record_stream(main)
        text_mask.record_stream(main)
    with _autocast(autocast_dtype):
        logits = mm.fusion_branch(text_feat, text_mask, audio, audio_mask, vis_concat, new_mask)
    if n_rows is None:
        metrics.update(logits, torch.as_tensor(labels, device=dev))
    else:
        metrics.update(logits, torch.as_tensor(labels, device=dev), n_rows=n_rows)
    return logits, new_mask, importance, counts


def _check_gumbel(gumbel):
    if gumbel not in ("sample", "off"):
        raise ValueError("gumbel: 'sample' (the reference: noise in evaluation too) or 'off' (deterministic)")
    return gumbel == "sample"


class EvalStep:
    """One batch of multimodal_evaluate (train.py:154-243), launch by launch, under no_grad with both models in eval(): Swin features ->
    ops.emotion_head -> select_frames -> multimodal forward -> MeldMetrics.update.  Same batch tuple as train_step.TargetStep.  Returns
    (logits, kept-frame mask); the models are back in their previous train / eval mode afterwards.  Inside the step the fused forwards of
    train_step.fuse_text_encoder run (train_step.fused_inference).

    `frame_capacity` (None: `frames` is the compact (sum num_imgs, ...) tensor): the meaning it has on train_step.TargetStep.  The batch carries
    `frames` as the loader pads them, (B, Lv, ...), and num_imgs the real counts; the step packs them into `frame_capacity` rows on the device
    (ops.pack_frames), runs Swin, the noise and the head on all of them and hands the row count to the frame filter.  num_imgs as a list or CPU
    tensor is checked on the host (ValueError before anything is launched); with a device tensor `frame_counts` -- the (2,) int32 device tensor
    [rows packed, frames in the batch] of the last batch -- tells afterwards ([1] > frame_capacity: frames were dropped).  `importance` then has
    `frame_capacity` rows, of which the first frame_counts[0] mean something: the others are the head's answer to an all-zero frame."""

    def __init__(self, swin_model, multimodal_model, args, autocast_dtype=None, gumbel="sample", metrics=None, frame_capacity=None):
        self.sample = _check_gumbel(gumbel)
        self.frame_capacity = None if frame_capacity is None else int(frame_capacity)
        if self.frame_capacity is not None and self.frame_capacity < 1:
            raise ValueError("frame_capacity: a positive number of frames")
        self.frame_counts = None
        self.swin, self.mm, self.args, self.autocast_dtype = swin_model, multimodal_model, args, autocast_dtype
        self.metrics = metrics if metrics is not None else MeldMetrics(swin_model.num_labels, next(multimodal_model.parameters()).device)
        self.importance = None

    def __call__(self, batch):
        with torch.no_grad(), _eval_mode(self.swin, self.mm), fused_inference():
            logits, new_mask, self.importance, self.frame_counts = _forward_batch(self.swin, self.mm, self.args, batch, self.metrics, self.autocast_dtype,
                                                                                  self.sample, frame_capacity=self.frame_capacity)
        return logits, new_mask


class GraphedEvalStep:
    """EvalStep's launches captured ONCE as a single HIP graph for the sample batch's shapes -- the text encoder as the one fork branch, the
    layout of GraphedTargetStep's graph A -- and replayed per batch: inputs are copied into static buffers, the metric update is inside the
    graph.  A batch of other shapes (the short last batch of a split) runs through an EvalStep on the same MeldMetrics; rows a caller padded
    carry a negative label.  The graph has a memory pool of its own and writes nothing the training graphs read except the bf16 weight
    shadows, which it rebuilds from the current parameters at its head exactly as they do.  The returned logits / mask are the graph's static
    outputs: clone what must survive the next call.

    `frame_capacity` (None: the above, and a batch whose compact frame tensor has another number of rows is "another shape"): an int, or an
    ascending tuple of ints ("buckets"), makes the step evaluate RAGGED batches by replay.  The sample `batch` and every later one carry
    `frames` as the loader pads them, (B, Lv, ...), with num_imgs the real counts (EvalStep's docstring).  One graph is captured per capacity;
    they share the static input buffers and the MeldMetrics, and no captured shape depends on the counts (a bucket below the sample batch's
    total is warmed up and captured with the sample's counts cut down to fit).  Per batch: num_imgs on the host picks the smallest bucket that
    holds the batch (`pick_bucket`; a total above the largest is a ValueError before anything is copied or launched); a device tensor takes the
    largest, without a synchronisation.  A batch whose other shapes differ runs through EvalStep(frame_capacity=largest).  `replays` and
    `fallbacks` count the two paths on the host; `capacity` is the bucket of the last call, `frame_counts` / `importance` its outputs
    (`importance` has `capacity` rows, the first frame_counts[0] of them real).  Under gumbel="sample" the noise tensor has the bucket's
    shape: see the module docstring.

    `pad_rows` (default False: everything above, bit for bit; needs `frame_capacity`, ValueError otherwise, as on GraphedTargetStep): a batch
    with 1 <= b <= B utterances whose other dimensions match is padded to the captured B by train_step.pad_target_batch (PAD_NOTE there: copies
    of row 0, zero frames with num_imgs = 0, label -100) and REPLAYED in the bucket its real frames pick; no eager step, no second warm-up.  The
    real row count goes into a static device word in front of the replay (a device fill, no synchronisation), and the captured metric update is
    ops.eval_accumulate_rows when the metrics collect: the padded rows are neither stored nor counted and the cursor advances by b.  Metrics
    that do not collect keep ops.eval_accumulate, which ignores the negative labels.  The step returns logits[:b], new_mask[:b].  `rows`: the
    real rows of the last call; `padded_calls`: the calls that padded; `fallbacks` stays 0 for such a batch."""

    def __init__(self, swin_model, multimodal_model, args, batch, autocast_dtype=None, gumbel="sample", metrics=None, overlap_text=True, warmup_iters=2,
                 frame_capacity=None, pad_rows: bool = False):
        require_packet_capture_off("GraphedEvalStep")
        self.sample = _check_gumbel(gumbel)
        self.pad_rows, self.rows, self.padded_calls = bool(pad_rows), None, 0
        if self.pad_rows and frame_capacity is None:
            raise ValueError("pad_rows: only with frame_capacity (compact frames change their shape with the batch's rows)")
        self.swin, self.mm, self.args, self.autocast_dtype = swin_model, multimodal_model, args, autocast_dtype
        self.buckets = frame_buckets(frame_capacity)
        if self.buckets is not None:
            _check_padded_frames(batch[8], batch[5])
            check_frame_total(batch[9], batch[8].shape[1], self.buckets[-1])
        self.replays = self.fallbacks = 0
        self.capacity = self.frame_counts = None
        dev = batch[8].device
        self.metrics = metrics if metrics is not None else MeldMetrics(swin_model.num_labels, dev)
        self.eager = EvalStep(swin_model, multimodal_model, args, autocast_dtype, gumbel, self.metrics, frame_capacity=self.buckets[-1] if self.buckets else None)
        self.static = [t.clone() if torch.is_tensor(t) else torch.as_tensor(t, device=dev) for t in batch]
        # the rows of the batch that exist, re-read by the captured metric update on every replay; without pad_rows no such word and no such kernel
        self.n_rows = torch.full((1,), len(batch[7]), dtype=torch.int32, device=dev) if self.pad_rows else None
        cap = distinct_stream(dev)
        self.text_stream = distinct_stream(dev, (cap,)) if overlap_text else None
        collect = getattr(self.metrics, "collect_rows", None)                  # the warm-up passes count into this one, through the same kernel
        scratch = MeldMetrics(self.metrics.num_labels, dev, collect_rows=None if collect is None else len(batch[7]))
        self.graphs = {}
        with torch.no_grad(), _eval_mode(self.swin, self.mm), fused_inference():
            for c in self.buckets or (None,):
                if c is not None:
                    self.static[9].copy_(torch.as_tensor(_clamp_counts(batch[9], batch[8].shape[1], c)))
                with warmup_undone([], dev, cap):                              # an evaluation pass moves nothing but the generator
                    for _ in range(max(1, warmup_iters)):                      # lazy initialisations, the shadow cache the pins are made from
                        scratch.reset()
                        _forward_batch(self.swin, self.mm, args, self.static, scratch, autocast_dtype, self.sample, frame_capacity=c, n_rows=self.n_rows)
                if not self.graphs:
                    self.shadows = _pin_shadows([self.swin, self.mm])
                graph = torch.cuda.CUDAGraph()
                with capture_window(), ops.pinned_scope(self.shadows):
                    with torch.cuda.graph(graph, stream=cap):
                        outs = _forward_batch(self.swin, self.mm, args, self.static, self.metrics, autocast_dtype, self.sample, self.text_stream,
                                              self.shadows, frame_capacity=c, n_rows=self.n_rows)
                self.graphs[c] = (graph, outs)
                _KEEP_GRAPHS.append((graph,))
            if self.buckets:
                self.static[9].copy_(torch.as_tensor(batch[9]))
        self.graph, (self.logits, self.new_mask, self.importance, _) = self.graphs[self.buckets[-1] if self.buckets else None]

    def __call__(self, batch):
        rows = self.static[7].shape[0]
        b, given = rows, batch
        if self.pad_rows and len(batch) == len(self.static) and 1 <= len(batch[7]) < rows:
            b, batch = len(batch[7]), pad_target_batch(batch, rows)
        try:
            check_static_shapes(self.static, batch, "GraphedEvalStep")
        except ValueError:
            if len(batch) != len(self.static):
                raise
            b, batch = rows, given                                 # not a short batch of the captured shapes: the launch-by-launch step, unpadded
            if self.buckets:
                _check_padded_frames(torch.as_tensor(batch[8]), torch.as_tensor(batch[5]))     # the compact tensor is an error, not "another shape"
            out = self.eager(batch)
            self.fallbacks += 1
            if self.buckets:
                self.capacity, self.frame_counts, self.importance = self.buckets[-1], self.eager.frame_counts, self.eager.importance
            return out
        c = pick_bucket(batch[9], self.static[8].shape[1], self.buckets) if self.buckets else None
        copy_into_static(self.static, batch, "GraphedEvalStep")
        self.graph, (self.logits, self.new_mask, self.importance, self.frame_counts) = self.graphs[c]
        self.capacity = c
        if self.pad_rows:
            self.n_rows.fill_(b)                                   # a device fill: no host synchronisation
        self.graph.replay()
        self.replays += 1
        self.rows = b
        self.padded_calls += int(b != rows)
        if b != rows:
            return self.logits[:b], self.new_mask[:b]
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


def evaluate(step, loader, sharded=False, process_group=None):
    """A whole split through `step` (EvalStep / GraphedEvalStep / UnimodalEvalStep): (avg_loss, results, truths) as multimodal_evaluate /
    unimodal_evaluate return them -- results = the concatenated logits, truths = the concatenated labels, both left on the device.  The one
    host synchronisation is the final copy of the accumulators; step.metrics.result() afterwards has the F1 scores of the same split.
    avg_loss = loss sum / rows (module docstring).

    When step.metrics collects (MeldMetrics(collect_rows=...)), nothing is cloned per batch: the metric update inside the step has stored every
    row, and results / truths are `collected()` -- views of the metrics' buffers, valid until its next reset() or update(); ValueError when the
    split had more rows than collect_rows.  Cursor and accumulators come to the host in the same single copy.

    `sharded=True` (collecting metrics only, ValueError otherwise): `loader` is this rank's shard of the split -- the rows parallel.eval_shard gives
    it, in batches the single-rank loader would have formed; an empty one for a rank without rows -- and step.metrics was built with
    collect_rows = parallel.eval_collect_rows(...).  The batches run with no collective between them, so ranks may run different numbers of them;
    then MeldMetrics.gather_merge(process_group) makes the whole split on every rank and (avg_loss, results, truths) are the WHOLE split's, from
    step.metrics.merged, the same values on every rank, in dataset order.  step.metrics.result() stays the rank's own, step.metrics.merged.result()
    is the split's.  Still one device-to-host copy per split on RCCL behind the W words gather_merge reads."""
    step.metrics.reset()
    if sharded:
        if getattr(step.metrics, "collect_rows", None) is None:
            raise ValueError("evaluate(sharded=True): the step's metrics collect the split (MeldMetrics(collect_rows=parallel.eval_collect_rows(...)))")
        for batch in loader:
            step(batch)
        merged = step.metrics.gather_merge(process_group)
        host = merged._host()
        nl = merged.num_labels
        return (merged.summarise(host[:2 + nl * nl], nl).avg_loss,) + merged.collected(host)
    if getattr(step.metrics, "collect_rows", None) is not None:
        for batch in loader:
            step(batch)
        host = step.metrics._host()
        nl = step.metrics.num_labels
        return (step.metrics.summarise(host[:2 + nl * nl], nl).avg_loss,) + step.metrics.collected(host)
    results, truths = [], []
    for batch in loader:
        out = step(batch)
        logits = out[0] if isinstance(out, tuple) else out
        labels = batch[2] if len(batch) == 3 else batch[7]
        results.append(logits.detach().float().clone())       # a graphed step hands out its static buffer
        truths.append(torch.as_tensor(labels, device=logits.device).clone())
    r = step.metrics.result()
    return r.avg_loss, torch.cat(results), torch.cat(truths)
