"""One target-task training step (forward + backward + optimizer) of FacialMMT on the HIP path.

Restates the body of the reference's `multimodal_train` loop (train.py:54-143) without its host
synchronisations: the per-face importance filter and the emotion-concat (train.py:75-114) are
cumsum / searchsorted / index_put on the device (parity pinned against the literal
loop restatement in oracle/train_glue.py, reference quirk included)."""
from __future__ import annotations

import types

import torch
import torch.nn.functional as F

from .graph_capture import (_KEEP_GRAPHS, _autocast, _bump_versions, _reset_optimizer_state, capture_window, copy_into_static,  # noqa: F401
                            distinct_stream, pick_concurrent_stream, replay_update, require_packet_capture_off, warmup_undone)
from . import step_state
from .step_state import StepState


SELECT_FRAMES_KERNEL = True      # module constant (tests patch it): False = the torch restatement below (~55 launches)


def select_frames(preds, vision_inputs, vision_mask, num_imgs, threshold, n_valid=None):
    """Device-side, sync-free version of train.py:75-114.

    preds (sumF, 7): per-face emotion distribution (Gumbel-softmax of the Swin logits), differentiable;
    vision_inputs (B, Lv, D); vision_mask (B, Lv); num_imgs (B,) int tensor of real frames per utterance.
    Faces with sum(p^2) > threshold are kept; each utterance packs its kept faces to the front
    (new mask = count of kept faces) together with the matching rows of vision_inputs; if no face at all
    passes, every real frame is kept.  Returns (vision_inputs_concat (B,Lv,D+7), new_vision_mask (B,Lv)).

    n_valid (a 1-element integer tensor on preds' device, ops.pack_frames' counts; None: every row is a face): preds holds a fixed
    capacity of rows of which the first n_valid are faces.  "No face at all passes" (train.py:80,84) is then decided over those rows
    only; ownership needs nothing (an owned face lies below the largest boundary max_u (sum_{i<=u} num_imgs_i - u) <= sum(num_imgs) = n_valid)."""
    B, Lv, D = vision_inputs.shape
    dev = preds.device
    nF = preds.shape[0]
    if SELECT_FRAMES_KERNEL and torch.is_tensor(num_imgs):
        from . import ops
        if ops.select_frames_fusable(preds, vision_inputs, vision_mask):
            return ops.select_frames(preds, vision_inputs, vision_mask, num_imgs, threshold, n_valid)      # one launch (csrc/frame_filter.hip): same index arithmetic
    n = torch.as_tensor(num_imgs).to(dev).long()
    importance = (preds * preds).sum(dim=1)                       # == diag(P P^T)
    sel = importance > threshold                                   # (nF,)
    g = torch.arange(nF, device=dev)
    # utterance boundaries with the reference's (n - 1) margin: b_u = sum_{i<=u} n_i - u; the loop hands the faces out in order, so an utterance
    # takes what lies between the largest boundary so far and its own -- the running maximum, which IS b_u while every n_i >= 1 and leaves an
    # utterance without frames (a padded row of a short batch, pad_target_batch) owning nothing
    csum = torch.cumsum(n, 0)
    raw = csum - torch.arange(B, device=dev)
    upper = torch.cummax(raw, 0).values                            # exclusive upper bound of utterance u (raw[0] = n_0 >= 0: never negative)
    margin = raw - n                                               # sum_{i<u}(n_i - 1)
    u = torch.searchsorted(upper, g, right=True)                   # owning utterance (== B: dropped tail)
    owned = sel & (u < B)
    uc = u.clamp(max=B - 1)
    # rank of each selected face inside its utterance
    sel_cum = torch.cumsum(owned.long(), 0)
    first_of_utt = torch.cat((torch.zeros(1, dtype=torch.long, device=dev), upper[:-1])).clamp(max=nF)   # start index of utt u
    before = torch.where(first_of_utt > 0, sel_cum[(first_of_utt - 1).clamp(min=0)], torch.zeros_like(first_of_utt))
    k = (sel_cum - 1 - before[uc]).clamp(min=0, max=Lv - 1)
    w = owned.to(preds.dtype).unsqueeze(1)
    emo_sel = torch.zeros(B, Lv, preds.shape[1], dtype=preds.dtype, device=dev).index_put((uc, k), preds * w, accumulate=True)
    src = vision_inputs[uc, (g - margin[uc]).clamp(min=0, max=Lv - 1)]                                   # (nF, D)
    inp_sel = torch.zeros_like(vision_inputs).index_put((uc, k), src * owned.to(vision_inputs.dtype).unsqueeze(1), accumulate=True)
    cnt = torch.zeros(B, dtype=torch.long, device=dev).index_put((uc,), owned.long(), accumulate=True)
    mask_sel = (torch.arange(Lv, device=dev).view(1, Lv) < cnt.view(B, 1)).to(vision_mask.dtype)
    # fallback branch (no face passes): sequential fill over the real frames, masks unchanged
    real = torch.cumsum(vision_mask, dim=1) == torch.arange(1, Lv + 1, device=dev).view(1, Lv)          # leading run of ones
    real_cnt = real.long().sum(1)
    offs = torch.cumsum(real_cnt, 0) - real_cnt
    idx_all = (offs.view(B, 1) + torch.arange(Lv, device=dev).view(1, Lv)).clamp(max=nF - 1)
    emo_all = preds[idx_all] * real.unsqueeze(-1).to(preds.dtype)
    any_sel = sel.any() if n_valid is None else (sel & (g < n_valid.reshape(-1)[0])).any()
    emo = torch.where(any_sel, emo_sel, emo_all)
    inputs = torch.where(any_sel, inp_sel, vision_inputs)
    mask = torch.where(any_sel, mask_sel, vision_mask)
    return torch.cat((inputs, emo.to(inputs.dtype)), dim=-1), mask


def pick_bucket(num_imgs, Lv, buckets):
    """The capacity a ragged batch runs in (a training step packs into it, a graphed step replays its capture): the smallest of the ascending
    `buckets` that holds its sum(clamp(num_imgs, 0, Lv)) real frames when num_imgs is on the host (a list or CPU tensor, as the reference's
    collate yields it); the LARGEST for a device tensor, which is not read here (that would be a host synchronisation).  A host total above the
    largest bucket: ValueError, before anything is launched."""
    if torch.is_tensor(num_imgs):
        if num_imgs.is_cuda:
            return buckets[-1]
        num_imgs = num_imgs.tolist()
    total = sum(min(max(int(n), 0), int(Lv)) for n in num_imgs)
    for c in buckets:
        if total <= c:
            return c
    raise ValueError(f"the batch holds {total} face frames, the step was built for frame_capacity={buckets[-1]}")


frame_bucket = pick_bucket                                  # the name the training steps call it by: one rule, not a second statement of it


def check_frame_total(num_imgs, Lv, capacity):
    """Host-side guard of a packed step (frame_capacity): pick_bucket with the one capacity the step was built for -- with num_imgs as the
    reference's collate yields it the real frames must fit it; ValueError otherwise, before anything is launched.  A device tensor is not read:
    the step's `frame_counts` then tells (counts[1] > capacity)."""
    pick_bucket(num_imgs, Lv, (capacity,))


def _clamp_counts(num_imgs, Lv, capacity):
    """the sample batch's counts cut down, utterance by utterance, until their total fits `capacity`: what a bucket below the sample's total is captured on"""
    out, room = [], int(capacity)
    for n in (num_imgs.tolist() if torch.is_tensor(num_imgs) else num_imgs):
        k = min(max(int(n), 0), int(Lv), room)
        out.append(k)
        room -= k
    return out


def frame_buckets(frame_capacity):
    """`frame_capacity` as the steps take it -> the ascending tuple of capacities ("buckets"), or None.  None -> None; an integer c -> (c,); a
    tuple or list must be non-empty, positive, ascending and free of duplicates.  Anything else: ValueError.  Pure host code."""
    if frame_capacity is None:
        return None
    caps = tuple(int(c) for c in frame_capacity) if isinstance(frame_capacity, (tuple, list)) else (int(frame_capacity),)
    if not caps or caps[0] < 1 or any(a >= b for a, b in zip(caps, caps[1:])):
        raise ValueError(f"frame_capacity: a positive number of frames, or an ascending tuple of them without duplicates, got {frame_capacity!r}")
    return caps


# ------------------------------------------------------------------------------------------------
# The text encoder on real tokens only (token_capacity on the target steps; _SeedBox PACK_NOTE): what the host decides per call.
# ------------------------------------------------------------------------------------------------
# Capacities are whole multiples of this many rows: the default capacity is the construction batch's token count rounded up to it.  Measured at
# the benchmark shape (4 x 512 tokens, 1600 real; NOTES.md R13): 64 and 128 rows are 0.1 ms apart (inside the spread), 256 is 0.3 ms behind; 64 leaves the benchmark no filler row.
TOKEN_GRANULE = 64

_TOKEN_COUNTS = {}                                           # device masks: id(tensor) -> (weak reference to it, its version, (total, prefix))


def count_tokens(mask):
    """(real tokens, every row a prefix of ones) of a (B, T) padding mask, on the host.  A host tensor (or nested list) is read directly; a device
    tensor costs ONE synchronisation per (tensor object, version), so a loop that hands over the same unmodified tensor every step never waits.  (The
    object, held weakly, and not its address: the caching allocator gives a new mask the address of a freed one.)"""
    m = torch.as_tensor(mask)
    if m.dim() != 2:
        raise ValueError(f"the text padding mask must be (B, T), got {tuple(m.shape)}")
    key = None
    if m.is_cuda:
        key = id(m)
        hit = _TOKEN_COUNTS.get(key)
        if hit is not None and hit[0]() is m and hit[1] == m._version:
            return hit[2]
    real = m != 0
    lens = real.sum(1)
    prefix = (real == (torch.arange(m.shape[1], device=m.device)[None, :] < lens[:, None])).all()
    total, ok = torch.stack([lens.sum(), prefix.to(lens.dtype)]).tolist()
    out = (int(total), bool(ok))
    if key is not None:
        if len(_TOKEN_COUNTS) > 64:
            _TOKEN_COUNTS.clear()
        import weakref
        _TOKEN_COUNTS[key] = (weakref.ref(m), m._version, out)
    return out


def default_token_capacity(mask, granule=None):
    """the capacity a step derives from its construction batch: the real tokens rounded up to TOKEN_GRANULE; 0 (= the padded path) for a mask with
    a hole, without a real token, or whose rounded count reaches B * T"""
    total, prefix = count_tokens(mask)
    g = int(granule or TOKEN_GRANULE)
    cap = (total + g - 1) // g * g
    B, T = torch.as_tensor(mask).shape
    return cap if prefix and 0 < total and cap < B * T else 0


def token_box(mm):
    """the _SeedBox of the multimodal model's text encoder when that encoder can run on packed rows (fuse_text_encoder packed every attention
    module of a bf16 encoder stack), else None"""
    plm = getattr(mm, "roberta", None) if getattr(mm, "text_pretrained_model", "") == "roberta" else getattr(mm, "bert", None)
    box = getattr(plm, "_fmmt_box", None)
    if box is None or not box.all_attention_fused or not PLM_FUSE_ATTN or next(plm.parameters()).dtype != torch.bfloat16:
        return None
    return box


class _text_rows:
    """`mm.text_token_capacity = rows` for the length of ONE forward of the model, 0 behind it whatever happens inside: whoever else calls the model
    (an evaluation step, whose masks nobody checks on the host) sees the padded layout"""

    def __init__(self, mm, rows):
        self.mm, self.rows = mm, int(rows or 0)

    def __enter__(self):
        self.mm.text_token_capacity = self.rows

    def __exit__(self, *exc):
        self.mm.text_token_capacity = 0
        return False


def token_fit(mask, capacity):
    """Does this batch run on packed rows?  False: token packing is off (capacity 0) or the mask is not a prefix of ones per row (the padded path
    computes such a mask correctly).  A prefix mask with more real tokens than `capacity`: ValueError, as check_frame_total for frames -- before
    anything is launched."""
    if not capacity:
        return False
    total, prefix = count_tokens(mask)
    if not prefix:
        return False
    if total > capacity:
        raise ValueError(f"the batch holds {total} text tokens, the step was built for token_capacity={capacity}")
    return True


# ------------------------------------------------------------------------------------------------
# A short last batch of an epoch behind a captured batch shape (pad_rows=True on the graphed steps).  PAD_NOTE: the rule for what a padded row
# holds, stated once.  Every padded row is a computation that can occur for a real utterance -- no kernel meets a degenerate case (a row whose
# masks are all zero gives NaN in the pooling head's softmax and in the text encoder's attention) -- and its label is -100, F.cross_entropy's
# default ignore_index: the loss is the mean over the real rows, and a padded row's gradient is zero from the loss on down.
# ------------------------------------------------------------------------------------------------
IGNORE_LABEL = -100


def _pad_count(b, rows, what):
    if b < 1 or b > rows:
        raise ValueError(f"{what}: a batch of {b} rows cannot be padded to {rows} rows (1 <= rows of the batch <= {rows})")
    return rows - b


def _pad_like_row0(t, extra):
    return torch.cat((t, t[:1].expand(extra, *t.shape[1:])), dim=0)


def _pad_const(t, extra, value=0):
    return torch.cat((t, t.new_full((extra, *t.shape[1:]), value)), dim=0)


def pad_target_batch(batch, rows):
    """The T+A+V batch (ids, attn_mask, sep_mask, audio, audio_mask, vision_inputs, vision_mask, labels, frames, num_imgs, utt_idx) with
    1 <= b <= rows utterances -> the same batch with `rows` utterances (b == rows: the entries as they are); ValueError otherwise.  A padded row:
      * ids, attn_mask, sep_mask, audio, audio_mask, utt_idx: COPIES OF ROW 0 -- a valid text and audio row (an all-zero attention mask would be a
        softmax over nothing);
      * vision_inputs, vision_mask, frames: ZEROS, num_imgs = 0.  The mask is zero and not copied: the reference's keep-everything branch
        (train.py:122-130) walks the vision_mask == 1 slots and takes Swin's rows in order, so a copied mask would run past the real frames; zero
        frames keep the BatchNorm statistics and the "any face passed" count over the real frames (the n_valid path of frame_capacity), and in the
        selection branch an utterance without frames owns nothing (select_frames: the boundaries as a running maximum);
      * labels = -100.
    `frames` is the loader's (b, Lv, ...) tensor; num_imgs and utt_idx may be lists (the reference's collate) or tensors and keep their kind.
    Works on CPU or device tensors; nothing is launched in-tree."""
    if len(batch) != 11:
        raise ValueError(f"pad_target_batch: a batch of 11 entries, got {len(batch)}")
    extra = _pad_count(len(batch[7]), rows, "pad_target_batch")
    if extra == 0:
        return tuple(batch)
    out = list(batch)
    for i in (0, 1, 2, 3, 4):
        out[i] = _pad_like_row0(batch[i], extra)
    for i in (5, 6, 8):
        out[i] = _pad_const(batch[i], extra)
    out[7] = _pad_const(torch.as_tensor(batch[7]), extra, IGNORE_LABEL)
    out[9] = _pad_const(batch[9], extra) if torch.is_tensor(batch[9]) else list(batch[9]) + [0] * extra
    out[10] = _pad_like_row0(batch[10], extra) if torch.is_tensor(batch[10]) else list(batch[10]) + [batch[10][0]] * extra
    return tuple(out)


def pad_unimodal_batch(batch, rows):
    """The V-only batch (feature, mask, labels) with 1 <= b <= rows rows -> `rows` rows: feature and mask of a padded row are copies of row 0 (a row
    the model already computes: finite everywhere), its label is -100.  b == rows: the entries as they are; b == 0 or b > rows: ValueError."""
    feature, mask, labels = batch
    extra = _pad_count(feature.shape[0], rows, "pad_unimodal_batch")
    if extra == 0:
        return feature, mask, labels
    return _pad_like_row0(feature, extra), _pad_like_row0(mask, extra), _pad_const(torch.as_tensor(labels), extra, IGNORE_LABEL)


def pad_aux_batch(images, labels, rows):
    """The auxiliary batch (images, labels) with 1 <= b <= rows images -> `rows` images: a padded image is zeros, its label -100.  The step passes b
    as the head BatchNorm's n_valid, so the padded rows take no part in the batch statistics and get no gradient."""
    extra = _pad_count(images.shape[0], rows, "pad_aux_batch")
    if extra == 0:
        return images, labels
    return _pad_const(images, extra), _pad_const(torch.as_tensor(labels), extra, IGNORE_LABEL)


def row_weight(b, world, global_rows, captured_rows=None):
    """The factor a rank multiplies its mean loss over `b` real rows with so that the all-reduce's mean over `world` ranks is the mean over the
    `global_rows` real rows all ranks hold together: b * world / global_rows (sum_r (w_r / world) * mean_r = sum_r b_r mean_r / global_rows).
    global_rows None -- every rank holds the same number of real rows, DistributedSampler's contract -- gives 1.0.  ValueError unless 1 <= b and
    b + (world - 1) <= global_rows <= world * captured_rows (every other rank holds at least one and at most the captured number of rows;
    `captured_rows` None: no upper bound is known).  Pure host code.  A rank without any real row is not covered: the padding refuses b == 0."""
    b, world = int(b), int(world)
    if b < 1 or world < 1:
        raise ValueError(f"row_weight: a rank holds at least one real row and the world at least one rank, got b={b}, world={world}")
    if global_rows is None:
        return 1.0
    g = int(global_rows)
    if g < b + (world - 1) or (captured_rows is not None and g > world * int(captured_rows)):
        raise ValueError(f"row_weight: global_rows={g} is impossible for a rank with {b} real rows among {world} ranks"
                         + (f" of at most {int(captured_rows)} rows each" if captured_rows is not None else "")
                         + f" ({b + world - 1} <= global_rows" + (f" <= {world * int(captured_rows)})" if captured_rows is not None else ")"))
    return b * world / g


class Criterion:
    """The loss a run chooses, torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps, reduction='mean') -- the value the reference sets once and
    hands every loop (train.py:295 -> :26,135,256) -- as a construction argument of the six training steps (CRITERION_NOTE at GraphedTargetStep.__init__).
    `weight` (None: every class counts 1): NL finite numbers >= 0, kept as ONE fp32 tensor on `device` (default: the current GPU, the CPU without
    one) that every captured launch addresses: `step.criterion.weight.copy_(new)` between steps is seen by the next replay, nothing is rebound.
    `label_smoothing`: eps in [0, 1), a host float the launches carry.  ValueError for anything else.
    Calling it, criterion(logits, labels) with logits (B, NL) and labels (B,) (a label outside [0, NL) is ignored: -100, a padded row), gives the
    mean loss: on the GPU ops.ce_loss (csrc/ce_loss.hip, one launch per direction, bf16 / fp32 logits read as they are), on the CPU `reference`.
    DEPARTURE from torch (include/fmmt_loss.h): a batch whose labelled rows weigh 0 together gives loss 0 and a zero gradient, not NaN.
    Not part of any state_dict(): like the betas it is given again when a run is resumed."""

    def __init__(self, weight=None, label_smoothing=0.0, device=None):
        eps = float(label_smoothing)
        if not 0.0 <= eps < 1.0:                             # NaN fails both comparisons
            raise ValueError(f"Criterion: label_smoothing must lie in [0, 1), got {label_smoothing}")
        self.label_smoothing = eps
        if device is None:
            device = weight.device if torch.is_tensor(weight) and weight.is_cuda else ("cuda" if torch.cuda.is_available() else "cpu")
        self.weight = None
        if weight is not None:
            w = torch.as_tensor(weight).detach().to(dtype=torch.float32)
            if w.dim() != 1 or not 1 <= w.numel() <= 8:
                raise ValueError(f"Criterion: weight must hold one number per class, 1 <= NL <= 8, got shape {tuple(w.shape)}")
            if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                raise ValueError("Criterion: the class weights must be finite and >= 0")
            self.weight = w.to(device).contiguous().clone()

    @property
    def num_labels(self):
        """NL the weights were given for; None without weights (any NL)"""
        return None if self.weight is None else self.weight.numel()

    def check_labels(self, num_labels):
        """ValueError unless the weights, when there are any, count `num_labels` classes"""
        if self.weight is not None and self.weight.numel() != int(num_labels):
            raise ValueError(f"Criterion: {self.weight.numel()} class weights for {int(num_labels)} classes")

    def __call__(self, logits, labels):
        if not logits.is_cuda:
            return self.reference(logits, labels)
        from . import ops
        self.check_labels(logits.shape[-1])
        lg = logits if logits.dtype in (torch.float32, torch.bfloat16) else logits.float()
        return ops.ce_loss(lg, labels, self.weight, self.label_smoothing)

    def reference(self, logits, labels):
        """The pure-torch statement of the formulas of include/fmmt_loss.h, in the dtype and on the device of `logits` (fp64 logits: the fp64
        reference the tests hold the kernels to), differentiable by autograd.  den == 0: loss 0, gradient 0."""
        x = logits
        NL = x.shape[-1]
        self.check_labels(NL)
        eps = self.label_smoothing
        lab = torch.as_tensor(labels).to(device=x.device, dtype=torch.int64)
        valid = (lab >= 0) & (lab < NL)
        y = lab.clamp(0, NL - 1)
        w = torch.ones(NL, dtype=x.dtype, device=x.device) if self.weight is None else self.weight.to(device=x.device, dtype=x.dtype)
        onehot = F.one_hot(y, NL).to(x.dtype)
        t = valid.to(x.dtype).unsqueeze(1) * ((1.0 - eps) * w[y].unsqueeze(1) * onehot + (eps / NL) * w.unsqueeze(0))
        num = -(t * torch.log_softmax(x, dim=-1)).sum()
        den = (valid.to(x.dtype) * w[y]).sum()
        some = den > 0
        return torch.where(some, num / torch.where(some, den, torch.ones_like(den)), torch.zeros_like(num))


def _check_criterion(criterion, num_labels=None):
    """the steps' `criterion` argument: None (F.cross_entropy and the plain head, every launch as before) or a Criterion"""
    if criterion is not None and not isinstance(criterion, Criterion):
        raise ValueError("criterion: None (plain cross-entropy) or a train_step.Criterion")
    if criterion is not None and num_labels is not None:
        criterion.check_labels(num_labels)
    return criterion


def _loss_of(criterion, logits, labels):
    """the mean loss of a step's (B, NL) logits: F.cross_entropy over the fp32 logits without a criterion -- the launches of before --, else the
    criterion's one launch (the logits are read in their own dtype, which is what the cast in front of F.cross_entropy computes)"""
    if criterion is None:
        return F.cross_entropy(logits.float(), labels)
    return criterion(logits, labels)


def check_criterion_rows(who, criterion, global_rows):
    """CRITERION_NOTE (at GraphedTargetStep.__init__), several ranks.  The ranks' weighted means are averaged by the exchange, which is what DDP over
    nn.CrossEntropyLoss(weight=...) gives.  `global_rows` corrects the mean of means to the mean over all real rows by the ROW count; under class
    weights the exact correction needs every rank's den (sum of w[label]), which the sampler does not know: ValueError.  With smoothing alone den
    IS the row count and global_rows works as without a criterion.  Pure host code."""
    if global_rows is not None and criterion is not None and criterion.weight is not None:
        raise ValueError(f"{who}: global_rows together with class weights: the correction needs the ranks' weight sums, which no row count gives")


def _check_global_rows(who, global_rows, weight_word, b, world, captured_rows):
    """the graphed steps' __call__: the weight this micro-step's loss is differentiated with (row_weight), or ValueError -- before any copy or launch"""
    if global_rows is not None and weight_word is None:
        raise ValueError(f"{who}: global_rows needs pad_rows=True and an active gradient exchange (without them every rank's mean counts alike)")
    return row_weight(b, world, global_rows, captured_rows)


class _Branch(torch.nn.Module):
    """One branch of the multimodal forward as a module of its own, so that torch.cuda.make_graphed_callables sees
    exactly the parameters it uses.  Shares the owner's sub-modules (same Parameter objects); never registered on the
    owner, so state_dict keys are untouched."""

    def __init__(self, owner, fn_name, submodules):
        super().__init__()
        self._fn = getattr(owner, fn_name)
        for i, m in enumerate(submodules):
            self.add_module(f"m{i}", m)

    def forward(self, *args):
        return self._fn(*args)


def graph_multimodal(mm, sample_args, autocast_dtype=None, overlap_text=True, parallel_fusion=False):
    """Capture forward and backward of the multimodal model as HIP graphs (torch.cuda.make_graphed_callables):
    its ~4000 small launches per step (24 PLM layers, 7 self-attention layers, 8 cross-modal layer calls) are
    host-bound when issued one by one (measured: 112 ms of host time per step against 105 ms of GPU work).
    Everything on that path is capture-safe: no host synchronisation, dropout seeds drawn on the device,
    bf16 weight shadows re-cast inside the graph.  Shapes are static (fixed synthetic batch).

    Two graphs are captured: the text branch (PLM -> text_linear -> slicing) and the fusion branch.  With
    `overlap_text` the text branch replays on a second HIP stream (`mm.text_stream`): it does not depend on the
    visual path, and its small launches fill the CUs that Swin's large launches leave idle between waves
    (measured on an MI355X: text encoder 28.4 ms + Swin 52.9 ms = 82.8 ms back to back, 66.9 ms concurrently).
    Returns the module (its forward now replays the graphs)."""
    require_packet_capture_off("graph_multimodal")
    ids, attn_mask, sep_mask, audio, audio_mask, vision, vision_mask, utt_idx = sample_args
    utt_idx = torch.as_tensor(utt_idx, device=ids.device)
    plm = mm.roberta if mm.text_pretrained_model == 'roberta' else mm.bert
    text = _Branch(mm, "text_branch", [plm, mm.text_linear])
    fusion = _Branch(mm, "fusion_branch", [mm.audio_linear, mm.audio_utt_transformer, mm.vision_linear, mm.vision_utt_transformer,
                                           mm.attention, mm.CrossModalTrans_TA, mm.CrossModalTrans_TA_V, mm.dropout, mm.classifier])
    B = ids.shape[0]
    act = autocast_dtype if autocast_dtype is not None else torch.float32
    text_feat = torch.zeros(B, mm.get_text_utt_max_lens, mm.hidden_size, device=ids.device, dtype=act, requires_grad=True)
    text_mask = torch.ones(B, mm.get_text_utt_max_lens, device=ids.device)
    side = None
    if overlap_text:
        # The gradient accumulators of the text branch's parameters must live on the text stream too: autograd runs
        # AccumulateGrad on the stream that was current when the node was created, and a node created on the main
        # stream would make the main stream wait for the whole text backward before Swin's backward could start.
        # Create them now, under the text stream, and keep them alive (DDP, wrapped later, finds these same nodes).
        side, ratio = pick_concurrent_stream(ids.device)
        mm.text_stream_concurrency = ratio                 # ~1.0: truly concurrent with the main stream; ~2.0: serialised
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mm._text_grad_accumulators = [p.expand_as(p).grad_fn.next_functions[0][0] for p in text.parameters() if p.requires_grad]
        torch.cuda.current_stream().wait_stream(side)
    # independent halves of the fusion stack (audio / vision encoder, the two directions of each cross-modal encoder) are
    # captured as parallel branches of the fusion graphs: models._pair
    mm.pair_stream = distinct_stream(ids.device, (side,)) if parallel_fusion else None
    with _autocast(autocast_dtype, cache_enabled=False), capture_window():
        gtext, gfusion = torch.cuda.make_graphed_callables(
            (text, fusion),
            ((ids, attn_mask, sep_mask, utt_idx), (text_feat, text_mask, audio, audio_mask, vision, vision_mask)),
            num_warmup_iters=3)
    # plain attributes, NOT child modules: the branch wrappers must not show up in mm.state_dict() / named_parameters()
    mm.pair_stream = None                                     # eager calls of the branches stay single-stream
    object.__setattr__(mm, "_text_call", gtext)
    object.__setattr__(mm, "_fusion_call", gfusion)
    _KEEP_GRAPHS.append((gtext, gfusion))
    mm.text_stream = side
    return mm


# The reference back-propagates the target-task loss through Swin (the emotion features are written into the vision tensor by a
# differentiable copy, train.py:101-104,121), but nothing ever reads those gradients: the target step clips and steps the multimodal
# model only (train.py:140-143), and Swin's optimizer zeroes them before its next use (train.py:20,33).  With "skip" the Swin forward
# of the target step runs without autograd (its fused kernels then also skip the saved-activation stores) and no Swin backward runs:
# the parameters, BatchNorm statistics and losses of every later step are the same to fp32 rounding (tests/test_gpu_train_step.py: the
# inference form of a few forward launches differs in the last bit), at 60 % of the step time (40.5 against 66.1 ms).  It is an OPTION: the default executes what the reference executes, and bench.py's `value` is measured with it.
SKIP_NOTE = "Swin's target-step gradients are never read (train.py:20,33,140-143): 'skip' does not compute them"


def _check_color_jitter(color_jitter):
    from .augment import ColorJitter
    if color_jitter is not None and not isinstance(color_jitter, ColorJitter):
        raise TypeError(f"color_jitter: an augment.ColorJitter or None, got {type(color_jitter).__name__}")
    return color_jitter


def _need_u8_frames(frames):
    if frames.dtype != torch.uint8:
        raise ValueError(f"color_jitter works on the uint8 crops the pre-step resizes (frames (.., S, S, 3) uint8), got {frames.dtype} frames")


def _check_augment(augment):
    from .augment import AffWildAugment
    if augment is not None and not isinstance(augment, AffWildAugment):
        raise TypeError(f"augment: an augment.AffWildAugment or None, got {type(augment).__name__}")
    return augment


def _need_u8_images(images):
    if images.dtype != torch.uint8:
        raise ValueError(f"augment works on the uint8 crops the pre-step resizes (images (B, S, S, 3) uint8), got {images.dtype} images")


class TargetStep(StepState):
    """Swin (train mode, Gumbel-softmax head) -> frame filter -> multimodal model -> CE -> backward ->
    (every `accumulation_steps`) clip + AdamW + schedule, as train.py:46-143.  Only the multimodal
    optimizer steps here; Swin receives gradients through the emotion features and is updated by the
    auxiliary task's optimizer (train.py:31), so its gradients are dropped after each step."""
    STATE_KIND, STATE_MODELS, STATE_WINDOW = "target", ("swin", "mm"), "trg_accumulation_steps"

    def __init__(self, swin_model, multimodal_model, optimizer, scheduler, args, autocast_dtype=None, ddp_model=None, averager=None,
                 discarded_swin_gradients="compute", frame_capacity=None, color_jitter=None, token_capacity=None, criterion=None):
        """`criterion` (None: F.cross_entropy, the launches of before): a Criterion -- CRITERION_NOTE at GraphedTargetStep.
        Data parallel: pass `averager` (parallel.GradientAverager over the multimodal parameters) or, alternatively,
        `ddp_model` (the module wrapped by torch's DistributedDataParallel).
        `color_jitter` (an augment.ColorJitter; None: no augmentation): the MELD train transform (utils/dataset.py:35-39,62-63) on the uint8 frames,
        inside the pre-step -- every call draws a table from the device generator for the frames Swin runs on and keeps it in `last_jitter`.
        `discarded_swin_gradients`: "compute" (default, what the reference executes) or "skip" -- see SKIP_NOTE.
        `frame_capacity` (None: `frames` is the compact (sum num_imgs, ...) tensor): the batch carries `frames` as the loader pads them,
        (B, Lv, ...), and the step packs them on the device into `frame_capacity` rows (ops.pack_frames), runs Swin on all of them with the
        head's BatchNorm over the real ones and filters with the same row count -- GraphedTargetStep(frame_capacity=...) launch by launch.  An
        ascending tuple of capacities: every batch is packed into the smallest that holds it (`frame_bucket`: num_imgs as a list or CPU tensor; a
        device tensor takes the largest); `capacity` is the one the last call ran in, `replays` counts the calls per capacity.
        `token_capacity` (PACK_NOTE): the text encoder's layers run on the real tokens packed into that many rows.  None (default): every call takes
        its own batch's count rounded up to TOKEN_GRANULE (nothing here has a captured shape); an integer: that many rows, more real tokens raise
        ValueError; 0: the padded layout.  A mask with a hole takes the padded layout.  `token_rows`: what the last call ran with (0: padded).
        Not under `ddp_model` (torch's DDP calls the module through its own forward: the padded layout)."""
        self.criterion = _check_criterion(criterion, getattr(args, "num_labels", None))
        self.token_capacity = None if token_capacity is None else int(token_capacity)
        if self.token_capacity is not None and self.token_capacity < 0:
            raise ValueError("token_capacity: a number of rows, 0 (padded layout) or None (per batch)")
        self.token_rows = 0
        self.capacities = frame_buckets(frame_capacity)
        self.frame_capacity = None if self.capacities is None else self.capacities[-1]
        self.capacity, self.replays = None, {c: 0 for c in self.capacities or ()}
        self.frame_counts = None                             # packed path: ops.pack_frames' counts of the last step (device, int32 [n_valid, total])
        if discarded_swin_gradients not in ("compute", "skip"):
            raise ValueError("discarded_swin_gradients: 'compute' or 'skip'")
        self.skip_swin_bwd = discarded_swin_gradients == "skip"
        self.swin = swin_model
        self.mm = multimodal_model
        self.mm_call = ddp_model if ddp_model is not None else multimodal_model
        self.exchange = averager if averager is not None else ddp_model
        self.opt = optimizer
        self.sched = scheduler
        self.args = args
        self.autocast_dtype = autocast_dtype
        self.i_batch = 0
        self.host_ms = {}          # cumulative host-side enqueue time per phase (no device sync)
        self.color_jitter = _check_color_jitter(color_jitter)
        self.last_jitter = None                              # color_jitter: the table of the last call (device, int32 (frames, 8))

    def start_epoch(self):
        """As the reference at the top of each epoch (train.py:52,54): gradients zeroed, micro-batch count restarted, so a
        partial accumulation window at the end of an epoch (len(loader) % trg_accumulation_steps != 0) is dropped, not
        carried into the next epoch."""
        self.i_batch = 0
        averager = self.exchange if hasattr(self.exchange, "zero_grad") and not isinstance(self.exchange, torch.nn.Module) else None
        if averager is not None:
            averager.zero_grad()
        else:
            self.opt.zero_grad(set_to_none=True)
        self.swin.zero_grad(set_to_none=True)

    def __call__(self, batch):
        (ids, attn_mask, sep_mask, audio, audio_mask, vision_inputs, vision_mask, labels, frames, num_imgs, utt_idx) = batch
        import time
        args = self.args
        t = [time.perf_counter()]

        evs = getattr(self, "gpu_events", None)          # optional: list collecting (phase, event) on the main stream

        def mark(name):
            t.append(time.perf_counter())
            self.host_ms[name] = self.host_ms.get(name, 0.0) + (t[-1] - t[-2]) * 1e3
            if evs is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                evs.append((name, e))
        if evs is not None:
            mark("start")
        from .parallel import GradientAverager, accumulate
        if self.color_jitter is not None:
            _need_u8_frames(frames)                          # ValueError before anything is launched
        if self.mm_call is not self.mm or token_box(self.mm) is None:
            if self.token_capacity:
                raise ValueError("token_capacity: needs the fused bf16 text encoder, called without torch's DistributedDataParallel")
            rows = 0
        elif self.token_capacity is None:
            rows = default_token_capacity(attn_mask)
        else:
            rows = self.token_capacity if token_fit(attn_mask, self.token_capacity) else 0      # ValueError before anything is launched
        self.token_rows = rows
        n_valid, swin_kw = None, {}
        if self.capacities is not None:
            cap = frame_bucket(num_imgs, frames.shape[1], self.capacities)     # ValueError before anything is launched
            from . import ops
            num_imgs = torch.as_tensor(num_imgs).to(frames.device)
            frames, n_valid = ops.pack_frames(frames, num_imgs, cap)
            self.frame_counts, swin_kw = n_valid, {"n_valid": n_valid}
            self.capacity = cap
            self.replays[cap] += 1
        self.i_batch += 1
        last = self.i_batch % args.trg_accumulation_steps == 0
        if getattr(self.mm, "text_stream", None) is not None:
            # start the text branch on its own stream before the Swin forward is enqueued (models.launch_text)
            with _text_rows(self.mm, rows), _autocast(self.autocast_dtype):
                self.mm.launch_text(ids, attn_mask, sep_mask, utt_idx)
        if self.color_jitter is not None:                   # one record per frame Swin runs on (packed: per slot of the capacity), drawn just ahead of Swin
            self.last_jitter = swin_kw["jitter"] = self.color_jitter.draw(frames.shape[0], frames.device)
        if self.skip_swin_bwd:
            with torch.no_grad():
                preds = self.swin(frames, is_trg_task=True, **swin_kw)
        else:
            preds = self.swin(frames, is_trg_task=True, **swin_kw)                   # (sumF, 7), Gumbel-softmax
        mark("swin_fwd")
        vis_concat, new_mask = select_frames(preds.float(), vision_inputs, vision_mask, num_imgs, args.FacialEmoImpor_threshold, n_valid)
        mark("frame_filter")
        # gradient exchange only on the last micro-step of the window; torch's DDP decides in its FORWARD whether the
        # coming backward synchronises, so the no_sync context has to cover the forward as well
        with accumulate(self.exchange, last):
            with _text_rows(self.mm, rows), _autocast(self.autocast_dtype):
                logits = self.mm_call(ids, attn_mask, sep_mask, audio, audio_mask, vis_concat, new_mask, utt_idx)
            mark("multimodal_fwd")
            loss = _loss_of(self.criterion, logits, labels) / args.trg_accumulation_steps
            loss.backward()
        mark("backward")
        if last:
            averager = self.exchange if isinstance(self.exchange, GradientAverager) else None
            if averager is not None:
                averager.finish()
            torch.nn.utils.clip_grad_norm_(self.mm.parameters(), args.clip)
            mark("clip")
            self.opt.step()
            if self.sched is not None:
                self.sched.step()
            if averager is not None:
                averager.zero_grad()                         # the .grad views into the flat buckets must survive
            else:
                self.opt.zero_grad(set_to_none=True)
            mark("optimizer")
        self.swin.zero_grad(set_to_none=True)
        return loss.detach(), new_mask


class VendorLinear(torch.nn.Linear):
    """nn.Linear of a low-precision text encoder with ops.VendorLinearFn behind it (same parameters, same state_dict keys)"""

    def forward(self, x):
        if self.bias is None or not x.is_cuda or x.dtype != self.weight.dtype or x.dtype not in (torch.bfloat16, torch.float32) \
                or self.weight.shape[0] % 8 or not torch.is_grad_enabled():
            return super().forward(x)
        from . import ops
        return ops.VendorLinearFn.apply(x, self.weight, self.bias)


class VendorLayerNorm(torch.nn.LayerNorm):
    """nn.LayerNorm of a bf16 text encoder: torch's forward, fmmt_layernorm_bwd_bf16 backward (ops.PlmLayerNormFn)"""

    def forward(self, x):
        if (self.weight is None or self.bias is None or not x.is_cuda or x.dtype != torch.bfloat16 or self.weight.dtype != torch.bfloat16
                or len(self.normalized_shape) != 1 or x.shape[-1] % 8 or x.shape[-1] > 2048 or not torch.is_grad_enabled()):
            return super().forward(x)
        from . import ops
        return ops.PlmLayerNormFn.apply(x, self.weight, self.bias, self.eps)


# Module constants (the probes patch them), not environment switches: each is the off-switch of one fused launch family
PLM_COLSUM, PLM_LN, FUSED_ADAMW, PIN_SHADOWS, FUSED_HANDOVER = True, True, True, True, True
PLM_FUSE_EMBED = True                                       # nn.Embedding tables: the weight gradient by fmmt_embedding_bwd (False: torch's embedding backward)
PLM_FUSE_FFN = True                                         # intermediate + output of a layer as one autograd node (ops.PlmFfnFn); False: the two modules
PLM_FUSE_ATTN = True                                        # a packed *SelfAttention runs its attention core on fmmt_mha_fwd / _bwd (False: the stock attention interface)
PLM_FUSE_TAILS, PLM_FUSE_QKV = True, True                  # fuse_text_encoder: sublayer tails as one launch per direction / packed query-key-value GEMM


class fused_inference:
    """`with fused_inference():` -- inside it the fused forwards of fuse_text_encoder (sublayer tails, the feed-forward node, the packed
    query / key / value projection with the in-tree attention core) also run when autograd is off, with p = 0 and nothing kept for a backward.
    Outside it a `no_grad` caller gets the stock modules, as before: the evaluation steps (eval_step.py) opt in, nobody else is changed."""
    depth = 0

    def __enter__(self):
        fused_inference.depth += 1
        return self

    def __exit__(self, *exc):
        fused_inference.depth -= 1
        return False


def _fusable_now():
    """autograd on (training: the fused nodes carry their own backward) or an evaluation step opted in (fused_inference)"""
    return torch.is_grad_enabled() or fused_inference.depth > 0


def use_colsum_bias_gradients(module):
    """Re-class every nn.Linear of `module` (a Hugging Face text encoder) as VendorLinear: the bias gradients of its ~146 Linear
    layers then cost one 4 us launch each instead of a memset + a multi-block reduction (measured: 3.2 + 0.8 ms per step).
    PLM_COLSUM = False (module constant) leaves the module alone.  Returns the number of layers changed."""
    if not PLM_COLSUM:
        return 0
    n = 0
    ln = PLM_LN
    for m in module.modules():
        if type(m) is torch.nn.Linear and m.bias is not None:
            m.__class__ = VendorLinear
            n += 1
        elif ln and type(m) is torch.nn.LayerNorm and m.elementwise_affine and m.bias is not None:
            m.__class__ = VendorLayerNorm                    # two backward launches instead of three (fmmt_layernorm_bwd_bf16)
    return n


class _SeedBox:
    """one device int64 word per forward of the text encoder, drawn inside the step (graph-replay safe: torch's captured generator) by a forward
    pre-hook; every fused sublayer reads it and adds its own salt"""

    def __init__(self):
        self.t = None
        self.all_attention_fused = False
        self.words = 1            # word 0: the sublayer tails (each adds its salt); word 1 + i: attention module i (its kernels take no salt)
        # the attention mask the caller handed the encoder, recorded by its pre-hook for the length of one forward: (mask: None or (batch, keys)
        # padding mask, its per-key logit bias once _fused_attention made it), or None = no forward of the encoder in progress or a mask of another
        # form (per query, causal, packed sequences ...): the layers' 4-d mask cannot tell a padding mask from those, so only this record decides.
        # A layer forward re-run after the model's forward returned (activation-checkpoint recomputation in the backward) finds no record and
        # would take the stock attention where the original forward took the fused one: a model with gradient checkpointing on records nothing
        self.mask = None
        # PACK_NOTE.  Running the layers on real tokens only.  `capacity` (0: off; set by the caller for the forwards it wants packed, e.g.
        # MultiModalTransformerForClassification.text_branch from `text_token_capacity`): with a (batch, keys) padding mask whose rows are prefixes of
        # ones, the hook in front of the encoder stack (encoder_pre_hook) packs the embedding output's real rows into (1, capacity, E) -- the
        # embeddings themselves and their dropout stream stay on the padded layout --, records the ops.TokenLayout in `packed` for the length of the
        # forward and drops the mask; attention then runs the kernels' ragged mode, the tails and the feed-forward node draw the padded call's dropout
        # mask through the layout's row map, and the model hands back (1, capacity, E): rows of the real tokens, sequence by sequence, zeros (and
        # zero gradients) behind.  `layout_out` keeps the layout of the last packed forward for the caller's ops.unpack_rows (take_layout).  The
        # CALLER vouches for the mask: a hole or more tokens than the capacity is not detected here (the steps check on the host, train_step.token_fit;
        # on the device the lengths are cut to the capacity, so nothing is read or written out of bounds -- the result is then simply wrong).
        self.capacity = 0
        self.packed = None
        self.layout_out = None
        self.packed_forwards = 0                            # forwards that ran packed: a step that asked for packing checks that it happened

    def take_layout(self):
        """the layout of the forward that just returned if it ran packed (once), else None"""
        lay, self.layout_out = self.layout_out, None
        return lay

    def encoder_pre_hook(self, mod, args, kwargs):
        """forward pre-hook of the encoder STACK (plm.encoder): PACK_NOTE.  Packs only inside a forward of the model that recorded a 2-d padding mask."""
        self.packed = None
        rec, cap = self.mask, int(self.capacity or 0)
        if cap <= 0 or rec is None or rec[0] is None or not args or not torch.is_tensor(args[0]) or not self.all_attention_fused:
            return None
        x = args[0]
        B, T = rec[0].shape
        if x.dim() != 3 or tuple(x.shape[:2]) != (B, T) or not x.is_cuda or x.dtype != torch.bfloat16 or not PLM_FUSE_ATTN or not _fusable_now():
            return None
        if cap > B * T or (x.shape[-1] * x.element_size()) % 16:
            return None
        from . import ops
        lay = ops.token_layout_raw(rec[0], cap)
        self.packed = self.layout_out = lay
        self.packed_forwards += 1
        kwargs = dict(kwargs)
        rest = list(args[1:])
        if "attention_mask" in kwargs:
            kwargs["attention_mask"] = None                 # a sequence's keys end where it ends: the ragged kernels need no bias
        elif rest:
            rest[0] = None
        return (ops.pack_rows(x, lay)[None],) + tuple(rest), kwargs

    def draw(self, device):
        self.t = torch.randint(0, 2 ** 62, (self.words,), dtype=torch.int64, device=device)

    def pre_hook(self, mod, args, kwargs):
        """forward pre-hook of the encoder: the seed word draw (training) and the record of the caller's attention mask (keyword or second positional)"""
        if mod.training:
            self.draw(next(mod.parameters()).device)
        mask = kwargs["attention_mask"] if "attention_mask" in kwargs else (args[1] if len(args) > 1 else None)
        self.packed = self.layout_out = None
        if getattr(mod, "is_gradient_checkpointing", False):
            self.mask = None
        else:
            self.mask = [None, None] if mask is None else ([mask, None] if torch.is_tensor(mask) and mask.dim() == 2 else None)

    def post_hook(self, mod, args, kwargs, out):
        self.mask = None
        self.packed = None


def _row_map(box, x):
    """PACK_NOTE: the row map of the packed forward in progress when x is its (1, capacity, E) rows, else None"""
    lay = box.packed
    return lay.row_map if lay is not None and x.dim() == 3 and x.shape[0] == 1 and x.shape[1] == lay.cap else None


def _sublayer_tail_forward(self, hidden_states, input_tensor):
    """forward of a re-classed transformers *SelfOutput / *Output: dense + dropout + residual + LayerNorm = the vendor GEMM + one launch"""
    d, ln = self.dense, self.LayerNorm
    p = float(self.dropout.p) if self.training else 0.0
    box = self._fmmt_seed
    if (not hidden_states.is_cuda or hidden_states.dtype != torch.bfloat16 or d.weight.dtype != torch.bfloat16 or ln.weight.dtype != torch.bfloat16
            or d.bias is None or ln.bias is None or d.weight.shape[0] % 8 or d.weight.shape[0] > 2048 or not _fusable_now()
            or (p > 0.0 and box.t is None)):
        return self._fmmt_stock_forward(hidden_states, input_tensor)
    from . import ops
    return ops.PlmSublayerTailFn.apply(hidden_states, input_tensor, d.weight, d.bias, ln.weight, ln.bias, ln.eps, p,
                                       box.t if p > 0.0 else 0, self._fmmt_salt, _row_map(box, hidden_states))


def _fused_ffn_chunk(self, attention_output):
    """feed_forward_chunk of a re-classed transformers *Layer: intermediate + output as one autograd node (ops.PlmFfnFn), or the stock pair of modules.
    A layer whose feed-forward runs in sequence chunks (config.chunk_size_feed_forward) takes the stock modules' own forwards: the fused dropout stream
    counts rows from 0 in every call with the module's one salt, so every chunk would draw the same mask."""
    inter, out = self.intermediate, self.output
    if getattr(self, "chunk_size_feed_forward", 0):
        return out._fmmt_stock_forward(inter(attention_output), attention_output)
    d1, d2, ln = inter.dense, out.dense, out.LayerNorm
    p = float(out.dropout.p) if self.training else 0.0
    box = out._fmmt_seed
    x = attention_output
    if (not PLM_FUSE_FFN or not x.is_cuda or x.dtype != torch.bfloat16 or not _fusable_now() or d1.bias is None or d2.bias is None or ln.bias is None
            or any(t.dtype != torch.bfloat16 for t in (d1.weight, d2.weight, ln.weight)) or d2.weight.shape[0] % 8 or d2.weight.shape[0] > 2048
            or d1.weight.shape[0] % 8 or d1.weight.shape[0] > 8192 or d1.weight.shape[1] != d2.weight.shape[0] or (p > 0.0 and box.t is None)):
        return self._fmmt_stock_ffn(attention_output)
    from . import ops
    return ops.PlmFfnFn.apply(x, d1.weight, d1.bias, d2.weight, d2.bias, ln.weight, ln.bias, ln.eps, p, box.t if p > 0.0 else 0, out._fmmt_salt,
                              _row_map(box, x))


def _fused_embedding_forward(self, input):
    """forward of a re-classed nn.Embedding of the text encoder: the stock lookup, the weight gradient by fmmt_embedding_bwd (ops.PlmEmbeddingFn)"""
    w = self.weight
    if (not PLM_FUSE_EMBED or not input.is_cuda or w.dtype != torch.bfloat16 or not torch.is_grad_enabled() or not w.requires_grad or self.max_norm is not None
            or self.scale_grad_by_freq or self.sparse or w.shape[1] % 8 or w.shape[1] > 2048 or input.numel() > 32768 or input.numel() == 0
            or input.dtype not in (torch.int64, torch.int32)):
        return self._fmmt_stock_forward(input)
    from . import ops
    return ops.PlmEmbeddingFn.apply(input, w, self.padding_idx)


def _is_exact_gelu(fn):
    """transformers' ACT2FN["gelu"] (GELUActivation over torch's erf gelu) or torch.nn.functional.gelu / nn.GELU() itself"""
    if fn is torch.nn.functional.gelu:
        return True
    if isinstance(fn, torch.nn.GELU):
        return fn.approximate == "none"
    return type(fn).__name__ == "GELUActivation" and getattr(fn, "act", None) is torch.nn.functional.gelu


def _packed_qkv_forward(self, hidden_states, *args, **kwargs):
    """forward of a re-classed transformers *SelfAttention: query / key / value as one GEMM over the packed weight they are slices of; everything
    behind the projections (head split, the attention interface, dropout) is the stock method's, fed through three pass-through Linear stand-ins"""
    w, b = self._fmmt_qkv
    q, k, v = self.query, self.key, self.value
    ok = (hidden_states.is_cuda and hidden_states.dtype == w.dtype and _fusable_now() and q.weight.data_ptr() == w.data_ptr()
          and k.weight.data_ptr() == w.data_ptr() + w[0].numel() * w.shape[0] // 3 * w.element_size()
          and v.weight.data_ptr() == w.data_ptr() + 2 * w[0].numel() * w.shape[0] // 3 * w.element_size() and q.bias.data_ptr() == b.data_ptr())
    # key / value from another tensor (cross-attention) or a cache: the packed projection of hidden_states would silently be the wrong one
    # (round-5 ADVICE).  transformers passes these by keyword or as the positional slots behind attention_mask / head_mask
    cross = (getattr(self, "is_cross_attention", False) or any(kwargs.get(k) is not None for k in ("encoder_hidden_states", "past_key_value", "past_key_values"))
             or any(torch.is_tensor(a) and a.dim() == 3 and a.shape[-1] == hidden_states.shape[-1] for a in args[2:]))
    packed = getattr(self._fmmt_seed, "packed", None) is not None
    if not ok or cross:
        if packed:
            raise RuntimeError("text encoder on packed rows (PACK_NOTE): this attention module cannot take the fused path, and the stock attention "
                               "would mix the sequences; build the step with token_capacity=0")
        return self._fmmt_stock_forward(hidden_states, *args, **kwargs)
    from . import ops
    fused = _fused_attention(self, hidden_states, args, kwargs, w, b)
    if fused is not None:
        return fused
    if packed:
        raise RuntimeError("text encoder on packed rows (PACK_NOTE): the in-tree attention kernels do not apply to this module, and the stock "
                           "attention would mix the sequences; build the step with token_capacity=0")
    yq, yk, yv = ops.PlmQkvFn.apply(hidden_states, q.weight, k.weight, v.weight, q.bias, k.bias, v.bias, w, b)
    saved = (self.query, self.key, self.value)
    try:                                                     # the stock forward calls self.query(x) ...: hand it the projections already made
        self.__dict__["_modules"] = dict(self._modules, query=_Fixed(yq), key=_Fixed(yk), value=_Fixed(yv))
        return self._fmmt_stock_forward(hidden_states, *args, **kwargs)
    finally:
        self.__dict__["_modules"] = dict(self._modules, query=saved[0], key=saved[1], value=saved[2])


def _fused_attention(self, hidden_states, args, kwargs, w, b):
    """the attention core of a packed *SelfAttention on the in-tree kernels (ops.PlmSelfAttnFn), or None where they do not apply (then: the stock attention
    interface behind the packed projection).  Encoder self-attention only: bf16, head_dim 64, no cache, no head mask, no attention weights asked for, and
    only inside a forward of the encoder whose caller passed no mask or a (batch, keys) padding mask (_SeedBox.pre_hook): that mask becomes the kernels'
    per-key logit bias.  transformers hands the layers the 4-d form of any mask, and a padding mask's is contiguous (B, 1, S, S) like a per-query one's
    (sequence packing, causal): a 4-d mask from the caller takes the stock interface."""
    if not PLM_FUSE_ATTN or hidden_states.dim() != 3 or hidden_states.dtype != torch.bfloat16:
        return None
    nH = int(getattr(self, "num_attention_heads", 0))
    E = w.shape[1]
    if nH <= 0 or E % nH or E // nH != 64 or getattr(self, "is_decoder", False) or getattr(self, "is_causal", False):
        return None
    if getattr(self, "position_embedding_type", "absolute") not in (None, "absolute"):
        return None                                         # relative-position variants add a term to the scores
    if kwargs.get("output_attentions") or kwargs.get("head_mask") is not None or any(a is not None for a in args[1:]):
        return None
    mask = args[0] if args else kwargs.get("attention_mask")
    B, S, _ = hidden_states.shape
    box = getattr(self, "_fmmt_seed", None)
    rec = box.mask if box is not None else None
    if rec is None:
        return None
    if mask is not None and (not torch.is_tensor(mask) or mask.dim() != 4 or mask.shape[0] != B or mask.shape[1] != 1 or mask.shape[-1] != S
                             or mask.shape[2] not in (1, S)):
        return None
    key_bias = None
    lay = box.packed
    if lay is not None:                                     # PACK_NOTE: (1, capacity, E) rows, the mask dropped by encoder_pre_hook
        if mask is not None or B != 1 or S != lay.cap:
            return None
    elif rec[0] is not None:
        if rec[0].shape != (B, S):
            return None
        if rec[1] is None:                                  # once per forward of the encoder, not once per layer
            m2 = rec[0] if rec[0].dtype == torch.bool else rec[0] != 0
            rec[1] = torch.where(m2, 0.0, -30000.0).to(torch.float32).contiguous()     # the kernels read it row-major: a transposed mask keeps its strides
        key_bias = rec[1]
    p = float(self.dropout.p) if self.training else 0.0
    if p > 0.0 and (box is None or box.t is None or box.t.numel() <= self._fmmt_attn_word):
        return None
    seed = box.t[self._fmmt_attn_word:self._fmmt_attn_word + 1] if p > 0.0 else 0
    scale = float(getattr(self, "scaling", 64 ** -0.5))
    from . import ops
    q, k, v = self.query, self.key, self.value
    out = ops.PlmSelfAttnFn.apply(hidden_states, q.weight, k.weight, v.weight, q.bias, k.bias, v.bias, w, b, nH, scale, p, seed, key_bias, lay)
    return out, None


class _Fixed(torch.nn.Module):
    def __init__(self, y):
        super().__init__()
        self.y = y

    def forward(self, x):
        return self.y


def fuse_text_encoder(plm, tails: bool = True, qkv: bool = True):
    """Launch diet for a bf16 Hugging Face BERT / RoBERTa encoder (src/models.py:75-91), call it AFTER the module has its final dtype / device
    (MasterWeights): (a) every *SelfOutput / *Output runs dense + dropout + residual + LayerNorm as the vendor GEMM + one fused launch, backward one
    launch + a reduction + the two GEMMs (ops.PlmSublayerTailFn); (b) every *SelfAttention computes query / key / value with ONE GEMM over a packed
    (3E, E) weight of which the three nn.Linear parameters become row slices (same Parameter objects, same names, same state_dict; the optimizer's
    views keep working) and, where the in-tree attention kernels apply (_fused_attention: bf16, head_dim 64, encoder self-attention), its attention core
    with them on the packed projection (PLM_FUSE_ATTN); (c) where a layer's *Output took (a) and its *Intermediate is dense -> exact GELU, the two run as one
    autograd node (ops.PlmFfnFn, PLM_FUSE_FFN; the count is left in plm._fmmt_fused_ffn); (d) the nn.Embedding tables keep their forward and take
    fmmt_embedding_bwd for the weight gradient (ops.PlmEmbeddingFn, PLM_FUSE_EMBED).  Returns (tails changed, attentions packed).  Numerics: (a) rounds like the bf16 module op by op,
    with its own dropout stream (counter-based, replayed in the backward instead of a stored mask); (b) is the same arithmetic as three GEMMs; the
    attention core is a flash-style online softmax in fp32 with bf16 probabilities, like the library kernel it replaces, and its own dropout stream."""
    box = _SeedBox()
    n_tail = n_qkv = 0
    salt = 0
    for name, m in plm.named_modules():
        cls = type(m).__name__
        if tails and cls.endswith(("SelfOutput", "Output")) and isinstance(getattr(m, "dense", None), torch.nn.Linear) \
                and isinstance(getattr(m, "LayerNorm", None), torch.nn.LayerNorm) and isinstance(getattr(m, "dropout", None), torch.nn.Dropout) \
                and not hasattr(m, "_fmmt_stock_forward"):
            m._fmmt_stock_forward = m.forward
            m._fmmt_seed = box
            salt += 1
            m._fmmt_salt = salt << 40                       # 2^40 elements per call site
            m.forward = types.MethodType(_sublayer_tail_forward, m)
            n_tail += 1
        elif qkv and cls.endswith("SelfAttention") and all(hasattr(m, a) for a in ("query", "key", "value")) and not hasattr(m, "_fmmt_stock_forward"):
            q, k, v = m.query, m.key, m.value
            if not all(isinstance(l, torch.nn.Linear) for l in (q, k, v)) or getattr(m, "is_cross_attention", False):
                continue
            if not (q.weight.shape == k.weight.shape == v.weight.shape and q.bias is not None and k.bias is not None and v.bias is not None
                    and q.weight.dtype == k.weight.dtype == v.weight.dtype):
                continue
            with torch.no_grad():
                w = torch.cat([q.weight.data, k.weight.data, v.weight.data], dim=0).contiguous()
                b = torch.cat([q.bias.data, k.bias.data, v.bias.data], dim=0).contiguous()
                E = q.weight.shape[0]
                for i, lin in enumerate((q, k, v)):
                    lin.weight.data = w[i * E:(i + 1) * E]
                    lin.bias.data = b[i * E:(i + 1) * E]
            m._fmmt_qkv = (w, b)
            m._fmmt_stock_forward = m.forward
            m._fmmt_seed = box
            m._fmmt_attn_word = box.words                   # its own word of the step's seed draw
            box.words += 1
            m.forward = types.MethodType(_packed_qkv_forward, m)
            n_qkv += 1
    # (c) the feed-forward half as one node: only where its output module took the fused tail (its seed box and salt are the node's)
    n_ffn = 0
    for name, m in plm.named_modules():
        inter, out = getattr(m, "intermediate", None), getattr(m, "output", None)
        if (tails and inter is not None and out is not None and hasattr(m, "feed_forward_chunk") and hasattr(out, "_fmmt_salt") and not hasattr(m, "_fmmt_stock_ffn")
                and isinstance(getattr(inter, "dense", None), torch.nn.Linear) and _is_exact_gelu(getattr(inter, "intermediate_act_fn", None))
                and type(inter).forward.__code__.co_names[:2] == ("dense", "intermediate_act_fn")):
            m._fmmt_stock_ffn = m.feed_forward_chunk
            m.feed_forward_chunk = types.MethodType(_fused_ffn_chunk, m)
            n_ffn += 1
    plm._fmmt_fused_ffn = n_ffn
    # (d) the embedding tables' weight gradients (the stock forward; the tables stay nn.Embedding modules)
    for name, m in plm.named_modules():
        if tails and type(m) is torch.nn.Embedding and not hasattr(m, "_fmmt_stock_forward"):
            m._fmmt_stock_forward = m.forward
            m.forward = types.MethodType(_fused_embedding_forward, m)
    if n_tail or n_qkv:
        plm.register_forward_pre_hook(box.pre_hook, with_kwargs=True)
        plm.register_forward_hook(box.post_hook, with_kwargs=True, always_call=True)
        # PACK_NOTE: the pack sits in front of the encoder stack, and only a stack whose every attention module was packed above may run on packed rows
        stack = getattr(plm, "encoder", None)
        n_attn = sum(1 for _, m in plm.named_modules() if type(m).__name__.endswith("SelfAttention"))
        box.all_attention_fused = bool(n_qkv) and n_qkv == n_attn
        if isinstance(stack, torch.nn.Module) and stack is not plm:
            stack.register_forward_pre_hook(box.encoder_pre_hook, with_kwargs=True)
        plm._fmmt_box = box
    return n_tail, n_qkv


class MasterWeights:
    """fp32 master copies of a sub-module that runs in a low-precision parameter dtype (the text encoder in bf16).

    Under autocast an fp32 text encoder re-casts every weight to bf16 in every step and casts every weight gradient
    back (about 1050 small launches and 2.5 GB of traffic per step for RoBERTa-large: measured 650 fp32->bf16 and 403
    bf16->fp32 copy kernels per step), and its LayerNorms run with fp32 I/O.  With bf16 parameters the module needs no
    autocast; the optimizer steps fp32 masters (`self.masters`, nn.Parameters that are views of one flat buffer) and
    `sync_low()` rounds them back into the module with one multi-tensor copy.  The masters start as exact copies of the
    fp32 parameters, so the trajectory is that of mixed-precision training with fp32 master weights."""

    def __init__(self, module: torch.nn.Module, dtype=torch.bfloat16):
        low = [p for p in module.parameters() if p.requires_grad]
        if any(p.dtype != torch.float32 for p in low):
            raise TypeError("MasterWeights: the module must still be in fp32 when the masters are taken")
        offs, n = [], 0
        for p in low:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        flat = torch.empty(n, dtype=torch.float32, device=low[0].device)
        self.masters = []
        for p, o in zip(low, offs):
            v = flat[o:o + p.numel()].view_as(p)
            v.copy_(p.detach())
            self.masters.append(torch.nn.Parameter(v))
        # what has no master -- frozen parameters (the unused pooler) and floating-point buffers -- keeps its fp32 values here: the
        # reference leaves them untouched, a checkpoint must not hold their bf16 roundings
        trainable = set(map(id, low))
        self.frozen_fp32 = {k: t.detach().clone() for k, t in list(module.named_parameters()) + list(module.named_buffers())
                            if id(t) not in trainable and t.is_floating_point() and t.dtype == torch.float32}
        module.to(dtype)                                    # in place: the Parameter objects survive, their data becomes bf16
        self.colsum_layers = use_colsum_bias_gradients(module)
        self.fused_layers = fuse_text_encoder(module, tails=PLM_FUSE_TAILS, qkv=PLM_FUSE_QKV)
        self.low = low
        self.flat = flat
        self.module = module

    def pairs(self):
        return list(zip(self.low, self.masters))

    @torch.no_grad()
    def sync_low(self):
        torch._foreach_copy_(self.low, self.masters)

    def fp32_items(self):
        """[(key of the module's state_dict, the LIVE fp32 tensor that holds its value)]: the master of every stepped parameter, the kept fp32
        copy of everything else that was rounded -- the one statement of which keys a checkpoint takes from where (state_dict_fp32, step_state)"""
        keys = set(self.module.state_dict().keys())
        by_id = {id(p): m for p, m in zip(self.low, self.masters)}
        out = [(k, by_id[id(p)]) for k, p in self.module.named_parameters() if id(p) in by_id and k in keys]
        return out + [(k, t) for k, t in self.frozen_fp32.items() if k in keys]

    def state_dict_fp32(self):
        """the module's state_dict with the master values in place of the rounded ones (what a checkpoint should hold)"""
        sd = {k: v.detach().clone() for k, v in self.module.state_dict().items()}
        sd.update({k: t.detach().clone() for k, t in self.fp32_items()})
        return sd


def _hand_over_gradients(pairs, flat_view_of, accumulate: bool):
    """After a backward: move the fresh gradients (p.grad of the model parameters) into the static flat fp32 buffers the
    optimizer and the all-reduce work on, with a handful of multi-tensor launches instead of one AccumulateGrad add per
    parameter (measured: 768 elementwise adds per step).  `accumulate=False` overwrites (one micro-step per update: no
    zeroing needed), True adds (gradient accumulation).  Leaves p.grad = None on the model parameters."""
    same_src, same_dst, cast_src, cast_dst = [], [], [], []
    for p, master in pairs:
        g = p.grad
        if g is None:
            continue
        p.grad = None
        dst = flat_view_of[master]
        if g.dtype == dst.dtype:
            same_src.append(g)
            same_dst.append(dst)
        else:
            cast_src.append(g)
            cast_dst.append(dst)
    with torch.no_grad():
        if accumulate:
            if same_src:
                torch._foreach_add_(same_dst, same_src)
            if cast_src:                                     # bf16 gradients into fp32 buffers: multi-tensor cast, then add
                tmp = [torch.empty_like(d) for d in cast_dst]
                torch._foreach_copy_(tmp, cast_src)
                torch._foreach_add_(cast_dst, tmp)
        else:
            if same_src:
                torch._foreach_copy_(same_dst, same_src)
            if cast_src:
                torch._foreach_copy_(cast_dst, cast_src)


def step_parameters(mm, masters=None):
    """the parameters the target step's optimizer updates: the multimodal model's, with the text encoder's replaced by
    their fp32 masters when it runs in bf16 (MasterWeights)"""
    if masters is None:
        return [p for p in mm.parameters() if p.requires_grad]
    master_of = {id(l): m for l, m in masters.pairs()}
    return [master_of.get(id(p), p) for p in mm.parameters() if p.requires_grad]


def named_step_parameters(mm, masters=None):
    """(name, parameter) for every parameter of step_parameters(mm, masters), in its order: the name is mm.named_parameters()'s, the parameter
    the one the optimizer steps (the fp32 master of a bf16 text-encoder weight) -- what parameter groups are built from by name:
        decay = [p for n, p in named_step_parameters(mm, masters) if not ("bias" in n or "LayerNorm" in n)]"""
    master_of = {id(l): m for l, m in masters.pairs()} if masters is not None else {}
    for name, p in mm.named_parameters():
        if p.requires_grad:
            yield name, master_of.get(id(p), p)


_GROUPS_AGREE_ON = (("correct_bias", True), ("amsgrad", False), ("maximize", False))


def group_plan(opt, params):
    """The host half of the grouped fused update, pure (CPU tensors do): which group of `opt` steps each parameter of `params`, and with what.
    Returns a namespace: `group_of`, one index into opt.param_groups per parameter, in `params`' order (the order of FusedClipAdamW's descriptor
    table); `groups`, one dict per group of the optimizer with its `lr` (as the group holds it: a tensor or a float), `betas`, `eps` and
    `weight_decay`.  A parameter of the optimizer that is not in `params` is ignored (the eager optimizer skips a parameter without a gradient);
    ValueError for a parameter of `params` that no group holds, and for groups that disagree on correct_bias, amsgrad or maximize (one launch
    has one hf_semantics and one formula)."""
    if not opt.param_groups:
        raise ValueError("group_plan: the optimizer has no parameter group")
    for key, default in _GROUPS_AGREE_ON:
        seen = [bool(g.get(key, default)) for g in opt.param_groups]
        if len(set(seen)) > 1:
            raise ValueError(f"group_plan: the parameter groups disagree on `{key}` ({seen}); the fused update takes one value for all groups")
    at = {id(p): j for j, g in enumerate(opt.param_groups) for p in g["params"]}
    group_of = []
    for i, p in enumerate(params):
        if id(p) not in at:
            raise ValueError(f"group_plan: parameter {i} of `params` (shape {tuple(p.shape)}) is in no parameter group of the optimizer")
        group_of.append(at[id(p)])
    groups = [{"lr": g["lr"], "betas": tuple(float(b) for b in g["betas"]), "eps": float(g["eps"]), "weight_decay": float(g["weight_decay"])}
              for g in opt.param_groups]
    return types.SimpleNamespace(group_of=group_of, groups=groups)


def group_tables(plan, dev):
    """the device half of group_plan: (`group_of` as int32, the group table of include/fmmt_groups.h as uint8) for ops.adamw_groups; every group's
    `lr` must be an fp32 tensor on `dev` -- the table holds its ADDRESS, so a scheduler that fills the tensor in place reaches the kernel"""
    import numpy as np
    from . import _lib
    tab = np.zeros(len(plan.groups), dtype=np.dtype(_lib.ADAMW_GROUP_FIELDS))
    assert tab.itemsize == _lib.ADAMW_GROUP_BYTES
    for j, h in enumerate(plan.groups):
        if not (torch.is_tensor(h["lr"]) and h["lr"].dtype == torch.float32 and h["lr"].numel() == 1 and h["lr"].device == dev):
            raise ValueError(f"group_tables: the learning rate of group {j} is not one fp32 word on {dev}")
        tab[j] = (h["lr"].data_ptr(), h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], 0)
    if any(not 0 <= j < len(plan.groups) for j in plan.group_of):
        raise ValueError("group_tables: a group index outside the group table")
    return torch.tensor(plan.group_of, dtype=torch.int32).to(dev), torch.from_numpy(tab.view(np.uint8).copy()).to(dev)


class HFAdamW(torch.optim.Optimizer):
    """`transformers.AdamW` restated (the optimizer class the reference constructs, train.py:307,333; transformers 4.24
    optimization.py, not vendored under the reference tree): defaults betas (0.9, 0.999), **eps 1e-6, weight_decay 0.0**,
    correct_bias True; per step
        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps);  p += p * (-lr wd)
    i.e. eps is added BEFORE the bias correction and the decoupled decay is applied AFTER the update -- both differ from
    torch.optim.AdamW (whose defaults are also eps 1e-8, weight_decay 0.01).  `lr` may be a 0-dim device tensor and the step
    counter is a device tensor, so the eager step is capture-safe; the graphed steps hand the same hyper-parameters to
    fmmt_adamw_batch(hf_semantics=1) through FusedClipAdamW (several parameter groups: fmmt_adamw_groups).  Every group has its own counter here."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for g in self.param_groups:
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            grads = [p.grad for p in ps]
            for p in ps:
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
            # the group's step counter is a device scalar kept IN the param group (capture-safe; transformers.AdamW keeps an int per
            # parameter: `hf_state_dict()` below writes that layout for exchange with the reference class)
            if not torch.is_tensor(g.get("step")):
                g["step"] = torch.zeros((), dtype=torch.float32, device=ps[0].device)
            t = g["step"]
            t.add_(1.0)
            b1, b2 = g["betas"]
            m = [self.state[p]["exp_avg"] for p in ps]
            v = [self.state[p]["exp_avg_sq"] for p in ps]
            torch._foreach_mul_(m, b1)
            torch._foreach_add_(m, grads, alpha=1.0 - b1)
            torch._foreach_mul_(v, b2)
            torch._foreach_addcmul_(v, grads, grads, value=1.0 - b2)
            den = torch._foreach_sqrt(v)
            torch._foreach_add_(den, g["eps"])
            lr = g["lr"] if torch.is_tensor(g["lr"]) else torch.tensor(float(g["lr"]), dtype=torch.float32, device=ps[0].device)
            step_size = lr * torch.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) if g["correct_bias"] else lr
            upd = torch._foreach_div(m, den)
            torch._foreach_mul_(upd, step_size)
            torch._foreach_sub_(ps, upd)
            if g["weight_decay"] > 0.0:
                dec = torch._foreach_mul(ps, lr * (-g["weight_decay"]))
                torch._foreach_add_(ps, dec)
        return loss

    def load_hf_state_dict(self, sd):
        """load a `transformers.AdamW` state dict (the reference's checkpoints, train.py:316-331: an int `step` per parameter, none in the
        groups): the per-parameter counters must agree within a group and become the group's device counter, so that the next step()
        continues the bias correction at t + 1 instead of restarting it with non-zero moments"""
        sd = {"state": {k: dict(v) for k, v in sd["state"].items()}, "param_groups": [dict(g) for g in sd["param_groups"]]}
        steps = []
        for g in sd["param_groups"]:
            ns = {int(sd["state"][i].pop("step")) for i in g["params"] if i in sd["state"] and "step" in sd["state"][i]}
            if len(ns) > 1:
                raise ValueError(f"per-parameter step counters of one group disagree: {sorted(ns)}")
            steps.append(ns.pop() if ns else None)
        # Optimizer.load_state_dict REPLACES each group with the checkpoint's values: the reference stores `lr` as a Python float, and the
        # graphed steps (FusedClipAdamW, a captured graph) address the group's 0-dim DEVICE lr tensor the scheduler writes into -- keep that
        # tensor object and fill it with the saved value; keys the checkpoint does not carry (`step`, anything added here later) stay
        live = [dict(g) for g in self.param_groups]
        self.load_state_dict(sd)
        for g, old, n in zip(self.param_groups, live, steps):
            if torch.is_tensor(old.get("lr")):
                saved = g["lr"]
                g["lr"] = old["lr"]
                with torch.no_grad():
                    g["lr"].fill_(float(saved))
            for k, v in old.items():
                if k not in g:
                    g[k] = v
            if n is not None:
                if torch.is_tensor(old.get("step")):
                    g["step"] = old["step"]
                    with torch.no_grad():
                        g["step"].fill_(float(n))
                else:
                    g["step"] = torch.full((), float(n), dtype=torch.float32, device=g["params"][0].device)

    def hf_state_dict(self):
        """`state_dict()` in transformers.AdamW's layout: an int `step` per parameter beside exp_avg / exp_avg_sq, none in the groups"""
        sd = self.state_dict()
        for g in sd["param_groups"]:
            t = g.pop("step", None)
            n = int(t.item()) if torch.is_tensor(t) else int(t or 0)
            for i in g["params"]:
                if i in sd["state"]:
                    sd["state"][i] = dict(sd["state"][i], step=n)
        return sd


class FusedHandOver:
    """_hand_over_gradients + the clip norm as ONE pass (fmmt_grad_handover): every fresh gradient is written (accumulation: added) into its
    slot of the flat fp32 buffers and the L2 norm of what the slots then hold lands in `norm_out` -- instead of a multi-tensor copy and a
    multi-tensor norm over the same 435 M values (23 + 30 launches, 1.3 ms of kernel time in the step's serial tail).  Returns False --
    nothing touched -- when a parameter has no gradient (its slot would keep a stale value the norm must still see) or a gradient is not a
    contiguous fp32 / bf16 tensor: the caller then takes the two-pass path.  The tables are built from the gradients' addresses on every call
    (warm-up passes, then once under capture: a captured step replays the copy of the one pinned table made then)."""

    def __init__(self, n_records: int, captures: int = 4):
        # pinned host tables, allocated HERE (a host allocation is illegal while a stream captures): two, used alternately -- an eager
        # (warm-up) call waits for the stream before it rewrites one, the call under capture leaves its table untouched for the replays
        self.hosts = [torch.empty(32 * max(1, n_records), dtype=torch.uint8).pin_memory() for _ in range(2)]
        # a call UNDER CAPTURE gets a table of its own that no later call rewrites (the captured copy node re-reads it on every replay: an
        # eager call after the capture -- a re-capture, a debugging pass -- must not land in it); `captures` (four) captures per object, then it raises.
        # A step with several frame capacities captures its forward/backward once per capacity: one table each, the records' destinations the same
        self.capture_hosts = [torch.empty(32 * max(1, n_records), dtype=torch.uint8).pin_memory() for _ in range(max(1, int(captures)))]
        self.captures = 0
        self.calls = 0
        self.keep = []                                       # (device table, partial sums): alive as long as the graphs

    @torch.no_grad()
    def __call__(self, pairs, flat_view_of, accumulate: bool, norm_out) -> bool:
        import numpy as np
        from . import ops
        grads = []
        for p, master in pairs:
            g = p.grad
            if g is None or not g.is_cuda or not g.is_contiguous() or g.dtype not in (torch.float32, torch.bfloat16) or g.numel() != flat_view_of[master].numel():
                return False
            grads.append(g)
        if not grads:
            return False
        dev = grads[0].device
        arr = np.zeros(len(grads), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("n", "<i8"), ("bb", "<i4"), ("flags", "<i4")]))
        blocks = 0
        for i, (g, (p, master)) in enumerate(zip(grads, pairs)):
            arr[i] = (g.data_ptr(), flat_view_of[master].data_ptr(), g.numel(), blocks, (1 if g.dtype == torch.bfloat16 else 0) | (2 if accumulate else 0))
            blocks += (g.numel() + 4095) // 4096
        raw = torch.from_numpy(arr.view(np.uint8))
        if raw.numel() > self.hosts[0].numel():
            return False
        if torch.cuda.is_current_stream_capturing():
            if self.captures >= len(self.capture_hosts):
                raise RuntimeError("FusedHandOver: more captures than pinned capture tables")
            host = self.capture_hosts[self.captures][:raw.numel()]
            self.captures += 1
        else:
            torch.cuda.current_stream(dev).synchronize()     # an earlier eager call's copy has read its table
            host = self.hosts[self.calls % 2][:raw.numel()]
            self.calls += 1
        host.copy_(raw)
        table = torch.empty(raw.numel(), dtype=torch.uint8, device=dev)
        table.copy_(host, non_blocking=True)
        partial = torch.empty(blocks, dtype=torch.float32, device=dev)
        ops.grad_handover_raw(len(grads), blocks, table, partial, norm_out)
        self.keep = self.keep[-3:] + [(table, partial)]
        for p, _ in pairs:
            p.grad = None
        return True


# GUARD_NOTE.  `skip_nonfinite=True` on a graphed training step (default False: nothing changes): the step builds a TrainMonitor (`step.monitor`), counts
# every micro-step's loss in it behind the loss inside the captured forward/backward, and SKIPS an update whose gradient norm is NaN or infinite --
# parameters, moments, bf16 twins and the update count keep their bits, the flat buffers are zeroed as after any update, `monitor.read().skipped`
# counts it (FusedClipAdamW, FlatGradientTail; ValueError with an optimizer the fused update does not take).  The learning-rate schedule advances on a
# skipped update too: that is what the reference does under GradScaler (train.py:139-143), and the host cannot know otherwise.  A non-finite FORWARD
# is not undone (BatchNorm's running statistics in the auxiliary step): `monitor.read().nonfinite_losses` reports it.  The counters are diagnostics,
# not part of state_dict(): they start at zero after a resume.
class TrainMonitor:
    """What a captured training run reports without a host synchronisation per step: six int64 words on the device (include/fmmt_guard.h,
    _lib.GUARD_*) that ops.monitor_loss (once per micro-step, behind the loss) and ops.guard_commit (once per update) write.  `read()` is one
    device-to-host copy; `reset()` zeroes in place (the captured graphs keep writing to this tensor).  The counters are diagnostics: they are
    not part of a step's state_dict() and start at zero after a resume."""

    def __init__(self, device="cuda"):
        from . import _lib
        self.words = torch.zeros(_lib.GUARD_WORDS, dtype=torch.int64, device=device)

    def reset(self):
        self.words.zero_()

    @staticmethod
    def summarise(host_words):
        """the host half of read(): `host_words` = the six int64 words as copied from the device.  avg_loss: the mean of the finite micro-step
        losses, undivided by the accumulation factor (what the reference logs, train.py:144-150), NaN while there is none; last_norm: the
        gradient norm the last update saw, NaN or inf when it was skipped for it"""
        import numpy as np
        from . import _lib
        host = np.ascontiguousarray(host_words, dtype=np.int64)
        if host.shape != (_lib.GUARD_WORDS,):
            raise ValueError(f"TrainMonitor.summarise: {_lib.GUARD_WORDS} int64 words")
        loss_sum = float(host[_lib.GUARD_LOSS_SUM:_lib.GUARD_LOSS_SUM + 1].view(np.float64)[0])
        micro = int(host[_lib.GUARD_MICRO_STEPS])
        last_norm = float(host[_lib.GUARD_LAST_NORM:_lib.GUARD_LAST_NORM + 1].astype(np.uint32).view(np.float32)[0])
        return types.SimpleNamespace(avg_loss=loss_sum / micro if micro else float("nan"), loss_sum=loss_sum, micro_steps=micro,
                                     nonfinite_losses=int(host[_lib.GUARD_NONFINITE_LOSSES]), applied=int(host[_lib.GUARD_APPLIED]),
                                     skipped=int(host[_lib.GUARD_SKIPPED]), last_norm=last_norm)

    def read(self):
        return self.summarise(self.words.cpu().numpy())

    def loss(self, loss, scale):
        """count one micro-step's loss (fp32 device scalar, already divided by `scale`): one launch, capture-safe"""
        from . import ops
        ops.monitor_loss(loss if loss.dtype == torch.float32 else loss.float(), scale, self.words)


# REPORT_NOTE.  `grad_report=True` on a graphed training step (default False: no buffer, no launch, every bit as before): the step builds a GradReport
# (`step.grad_report`) over the fused update's descriptor table, and every update runs ops.table_stats over the flat gradient buffers between the
# clip norm and the update launch -- the values the update sees, before they are zeroed (train.py:135-143: the moment p.grad can be inspected in
# the reference).  `step.grad_report.read()` gives each parameter's gradient norm, largest magnitude and NaN / inf count of the last update by
# name; an update whose norm was NaN or infinite leaves a snapshot behind (`last_bad`, `last_bad.first`) that later clean updates do not touch.
# With or without skip_nonfinite: without the guard the parameters still go NaN, but the snapshot names the cause.  Only with the fused update
# (ValueError otherwise, as skip_nonfinite); a diagnostic, not part of state_dict().
class GradReport:
    """Per-parameter statistics of what the fused update reads, kept on the device: `stats` (one record of _lib.STATS_FIELDS per record of
    FusedClipAdamW's descriptor table, written by every captured update), `bad_stats` / `bad_words` (the copy a non-finite norm leaves, its count
    and the first offending record) and `partial` (the per-block scratch) -- include/fmmt_stats.h.  `read()` is one device-to-host copy;
    `reset()` zeroes in place (the captured graphs keep these addresses); `state(which)` runs the kernel on demand over the parameters or a
    moment.  `named`: (name, parameter) pairs, matched by identity to the table's order when FusedClipAdamW binds the report to its table (bind():
    the buffers exist from then on); a parameter without a name is `param{i}`."""

    def __init__(self, named=()):
        self.named = [(name, p) for name, p in named]
        self.names, self.n, self.blocks = [], 0, 0
        self.desc = self.buf = self.stats = self.bad_stats = self.bad_words = self.partial = self._on_demand = None

    def bind(self, desc, n, blocks, params):
        """FusedClipAdamW's: the descriptor table this report is over (`n` records in `blocks` blocks, kept alive here too) and the parameters of its
        records, in order"""
        from . import _lib
        if self.desc is not None:
            raise RuntimeError("GradReport: already bound to an update's table; one report serves one FusedClipAdamW")
        if len(params) != n:
            raise ValueError(f"GradReport.bind: {len(params)} parameters for a table of {n} records")
        name_of = {}
        for name, p in self.named:
            name_of.setdefault(id(p), name)
        self.names = [name_of.get(id(p), f"param{i}") for i, p in enumerate(params)]
        self.desc, self.n, self.blocks = desc, int(n), int(blocks)
        # ONE allocation, so that read() is one copy: stats rows, bad_stats rows, then the two int64 words as one more 16-byte row
        self.buf = torch.zeros((2 * n + 1, 4), dtype=torch.int32, device=desc.device)
        self.stats, self.bad_stats = self.buf[:n], self.buf[n:2 * n]
        self.bad_words = self.buf[2 * n].view(torch.int64)
        assert self.bad_words.numel() == _lib.STATS_BAD_WORDS
        self.partial = torch.empty((self.blocks, 4), dtype=torch.int32, device=desc.device)

    def reset(self):
        if self.buf is not None:
            self.buf.zero_()

    def record(self, norm):
        """inside the update, behind the norm and in front of the update launch: two launches, capture-safe"""
        from . import _lib, ops
        ops.table_stats(_lib.STATS_G, self.n, self.blocks, self.desc, self.partial, self.stats, norm=norm, bad_stats=self.bad_stats, bad_words=self.bad_words)

    @staticmethod
    def _fields(rows, names):
        import numpy as np
        sumsq = rows["sumsq"].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            norm, total = np.sqrt(sumsq), float(np.sqrt(sumsq.astype(np.float64).sum()))
        ns = types.SimpleNamespace(names=list(names), norm=norm, sumsq=sumsq, max_abs=rows["max_abs"].copy(), nonfinite=rows["nonfinite"].copy(), total_norm=total)

        def worst(k):
            """the k names with the largest norm, largest first; a NaN norm counts as the largest of all"""
            key = np.where(np.isnan(ns.norm), np.inf, ns.norm)
            return [ns.names[i] for i in np.argsort(-key, kind="stable")[:max(int(k), 0)]]
        ns.worst = worst
        return ns

    @staticmethod
    def summarise(stats_host, bad_host, bad_words_host, names):
        """the host half of read(), pure: `stats_host` / `bad_host` = the records as copied from the device ((n, 4) int32 rows, or None for
        `bad_host` and `bad_words_host`: no snapshot fields), `bad_words_host` = the two int64 words.  Returns a namespace: names, norm (sqrt of
        sumsq), sumsq, max_abs, nonfinite (numpy, one entry per name), total_norm (sqrt of the fp64 sum of sumsq), worst(k); and with the
        snapshot: bad_updates, last_bad -- the same fields of the last update whose norm was not finite plus `first`, the name of the first
        tensor with a non-finite element or sum (None when no single tensor has one); last_bad is None while bad_updates == 0"""
        import numpy as np
        from . import _lib
        rec = np.dtype(_lib.STATS_FIELDS)
        names = list(names)

        def rows(host, what):
            a = np.ascontiguousarray(host, dtype=np.int32)
            if a.shape != (len(names), 4):
                raise ValueError(f"GradReport.summarise: {what} is {len(names)} rows of four int32 words")
            return a.view(rec).reshape(len(names))
        out = GradReport._fields(rows(stats_host, "stats_host"), names)
        if bad_words_host is None:
            return out
        words = np.ascontiguousarray(bad_words_host, dtype=np.int64)
        if words.shape != (_lib.STATS_BAD_WORDS,):
            raise ValueError(f"GradReport.summarise: {_lib.STATS_BAD_WORDS} int64 words")
        out.bad_updates, out.last_bad = int(words[0]), None
        if out.bad_updates:
            first = int(words[1])
            if not -1 <= first < len(names):
                raise ValueError(f"GradReport.summarise: the first bad record is {first}, the table has {len(names)}")
            out.last_bad = GradReport._fields(rows(bad_host, "bad_host"), names)
            out.last_bad.first = names[first] if first >= 0 else None
        return out

    def read(self):
        if self.desc is None:
            raise RuntimeError("GradReport.read: the report is not bound to an update's table yet (FusedClipAdamW(report=...))")
        host = self.buf.cpu().numpy()
        n = self.n
        return self.summarise(host[:n], host[n:2 * n], host[2 * n].view("<i8"), self.names)

    def worst(self, k):
        return self.read().worst(k)

    def state(self, which):
        """the same statistics of the parameters ("p"), first ("m") or second ("v") moments, now and not captured: after load_state_dict, or when
        parallel.replicas_agree raised, to name the tensor.  Its own result rows: the captured update's are not touched; the per-block scratch is
        shared with it, so call this on the stream the step is replayed on (the current one, as everything here), where the two are ordered"""
        from . import _lib, ops
        code = {"p": _lib.STATS_P, "m": _lib.STATS_M, "v": _lib.STATS_V}.get(which)
        if code is None:
            raise ValueError(f'GradReport.state: which is "p", "m" or "v", not {which!r}')
        if self.desc is None:
            raise RuntimeError("GradReport.state: the report is not bound to an update's table yet (FusedClipAdamW(report=...))")
        if self._on_demand is None:
            self._on_demand = torch.empty((self.n, 4), dtype=torch.int32, device=self.buf.device)
        ops.table_stats(code, self.n, self.blocks, self.desc, self.partial, self._on_demand)
        return self.summarise(self._on_demand.cpu().numpy(), None, None, self.names)


class FusedClipAdamW:
    """clip_grad_norm_ + AdamW.step() (torch.optim.AdamW, or HFAdamW = the reference's transformers.AdamW) (+ the bf16 re-rounding of parameters stepped through fp32 masters) as one
    multi-tensor norm and ONE kernel launch (fmmt_adamw_batch): the gradients are read once and not scaled in place, the fp32
    parameters are not read a second time for their bf16 twins.  Takes its hyper-parameters from an existing torch AdamW
    (tensor learning rate on the device as `capturable=True` keeps it, so a LambdaLR scheduler keeps
    working); keeps its own moments and step counter -- `optimizer.state` stays empty while this is in use.
    Parameter groups: with one group the launch is fmmt_adamw_batch and the group's betas / eps / weight decay are launch arguments; with several
    (no decay on biases and LayerNorm weights, a learning rate per sub-model, a group held still with lr = 0) it is fmmt_adamw_groups -- still ONE
    launch, which reads each record's learning rate word, betas, eps and weight decay from a group table built here once (group_plan).  One update
    count and one clip coefficient serve all groups, as clip_grad_norm_(model.parameters()) and a step() over all groups give.
    `monitor` (a TrainMonitor; None: the path above, unchanged): the update is SKIPPED when the gradient norm is NaN or infinite -- what GradScaler
    does for the reference under AMP (train.py:139-143) -- decided on the device: update() runs the norm, ops.adamw_batch_guarded (every block
    reads the norm first and leaves p, m, v and the bf16 twins alone when it is not finite) and ops.guard_commit (advances `step` only for an
    applied update, counts applied / skipped in the monitor).  `step` stays the number of APPLIED updates, so export() / load_from() mean what
    they meant; with finite gradients every bit is the unguarded path's.
    `report` (a GradReport; None: no launch more): REPORT_NOTE -- update() runs ops.table_stats over the gradient field of the descriptor table behind
    the norm (ready from the hand-over, or taken here over the reduced buffers) and in front of whichever of the four update launches runs, so the
    report sees the values the update sees: on one rank or several, with or without accumulation, with one group or many."""

    plan = group_of = group_table = None                     # several parameter groups only: group_plan's result and its two device tables

    @staticmethod
    def eligible(opt, params):
        """any number of parameter groups (at least one) of torch.optim.AdamW / HFAdamW, each with one fp32 word on the device as its learning rate (one tensor
        may serve several groups), no amsgrad, no maximize, correct_bias; fp32 device parameters, each held by a group"""
        if not FUSED_ADAMW or type(opt) not in (torch.optim.AdamW, HFAdamW) or len(opt.param_groups) < 1:
            return False
        for g in opt.param_groups:
            if not (torch.is_tensor(g["lr"]) and g["lr"].is_cuda and g["lr"].numel() == 1 and g["lr"].dtype == torch.float32 and not g.get("amsgrad", False)
                    and not g.get("maximize", False) and g.get("correct_bias", True)):
                return False
        held = {id(p) for g in opt.param_groups for p in g["params"]} if len(opt.param_groups) > 1 else None
        return all(p.dtype == torch.float32 and p.is_cuda and (held is None or id(p) in held) for p in params)

    def __init__(self, opt, params, grad_of, low_of, max_norm, monitor=None, report=None):
        import numpy as np
        self.monitor = monitor
        self.report = report
        if len(opt.param_groups) == 1:                       # the hyper-parameters are launch arguments of fmmt_adamw_batch, as ever
            g = opt.param_groups[0]
            self.lr, (self.b1, self.b2), self.eps, self.wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        else:                                                # fmmt_adamw_groups reads them from two device tables, built below
            self.plan = group_plan(opt, params)
        self.hf = isinstance(opt, HFAdamW)                    # transformers.AdamW's update (the reference's class) vs torch.optim.AdamW's
        self.max_norm = float(max_norm)
        dev = params[0].device
        self.step = torch.zeros((), dtype=torch.float32, device=dev)
        self.grads = [grad_of[p] for p in params]
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.norm = torch.zeros((), dtype=torch.float32, device=dev)
        self.norm_ready = False                              # set by the caller when FusedHandOver already left the norm in self.norm
        # The norm alone as ONE launch: fmmt_grad_handover with every flat gradient buffer as its own source and destination (a copy onto itself
        # plus the partial sums of squares).  N > 1: the buffers change between the hand-over and the update (the exchange averages them), so the
        # hand-over's own norm is of the wrong values -- this second pass over the REDUCED buffers replaces the multi-tensor norm (30 launches).
        self.norm_table = self.norm_partial = None
        if FUSED_HANDOVER:
            tb = np.zeros(len(params), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("n", "<i8"), ("bb", "<i4"), ("flags", "<i4")]))
            nb = 0
            for i, g in enumerate(self.grads):
                tb[i] = (g.data_ptr(), g.data_ptr(), g.numel(), nb, 0)
                nb += (g.numel() + 4095) // 4096
            self.norm_table = torch.from_numpy(tb.view(np.uint8).copy()).to(dev)
            self.norm_partial = torch.empty(nb, dtype=torch.float32, device=dev)
            self.norm_blocks = nb
        recs, blocks = [], 0
        self.keep = (params, [low_of.get(id(p)) for p in params])
        for p, gr, m, v, low in zip(params, self.grads, self.m, self.v, self.keep[1]):
            assert gr.dtype == torch.float32 and gr.is_contiguous() and p.is_contiguous() and (low is None or (low.dtype == torch.bfloat16 and low.is_contiguous()))
            recs.append((p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), low.data_ptr() if low is not None else 0, p.numel(), blocks, 0))
            blocks += (p.numel() + 4095) // 4096
        arr = np.zeros(len(recs), dtype=np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("low", "<u8"), ("n", "<i8"), ("bb", "<i4"), ("pad", "<i4")]))
        for i, r in enumerate(recs):
            arr[i] = r
        self.desc = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
        self.n, self.blocks = len(recs), blocks
        self._digest_partial = None
        if report is not None:
            report.bind(self.desc, self.n, self.blocks, params)
        if self.plan is not None:                            # built once: the learning rates are addresses, the schedulers write through them
            self.group_of, self.group_table = group_tables(self.plan, dev)

    def digest(self, out=None):
        """the replica digest of what this object steps (ops.param_digest on its own descriptor table): six int64 words on the device -- (S1, S2)
        of the parameters, the first and the second moments -- that are equal on two ranks exactly when (up to a 2^-64 coincidence) the bits are;
        two launches, no host synchronisation; the scratch for the per-block words is allocated on the first call and kept"""
        from . import ops
        if self._digest_partial is None:
            self._digest_partial = torch.empty(6 * self.blocks, dtype=torch.int64, device=self.desc.device)
        return ops.param_digest(self.n, self.blocks, self.desc, out=out, partial=self._digest_partial)

    def reset(self):
        self.step.zero_()
        torch._foreach_zero_(self.m)
        torch._foreach_zero_(self.v)

    @torch.no_grad()
    def load_from(self, opt):
        """take moments and step counter from `opt` (after HFAdamW.load_hf_state_dict / Optimizer.load_state_dict of a checkpoint): this object
        keeps its own m, v and step -- the ones the captured update addresses -- so a loaded optimizer state must be copied IN, in place.
        Parameters the optimizer holds no state for keep zero moments.  Every loaded group's betas / eps / weight decay must be this object's
        for that group: the captured update holds them as launch arguments (several groups: in its group table), so others cannot take effect;
        and the groups must agree on the update count, for there is one counter -- ValueError naming the group and the field, nothing copied."""
        params = self.keep[0]
        plan = self.plan
        hyper = plan.groups if plan is not None else [{"betas": (self.b1, self.b2), "eps": self.eps, "weight_decay": self.wd}]
        group_of = plan.group_of if plan is not None else [0] * len(params)
        if len(opt.param_groups) != len(hyper):
            raise ValueError(f"FusedClipAdamW.load_from: {len(opt.param_groups)} parameter groups loaded, the update was built over {len(hyper)}")
        for j, (g, h) in enumerate(zip(opt.param_groups, hyper)):
            who = "FusedClipAdamW.load_from" if plan is None else f"FusedClipAdamW.load_from, group {j}"
            step_state.check_hyper(g, {k: h[k] for k in ("betas", "eps", "weight_decay")}, who)
        counts = {}                                           # group -> its update count: the group's own counter (HFAdamW), else its parameters'
        for j in sorted(set(group_of)):
            t = opt.param_groups[j].get("step")
            ts = {float(t)} if t is not None else {float(opt.state[p]["step"]) for p, k in zip(params, group_of)
                                                   if k == j and p in opt.state and "step" in opt.state[p]}
            if len(ts) > 1:
                raise ValueError(f"per-parameter step counters disagree: {sorted(ts)}")
            counts[j] = ts.pop() if ts else None
        seen = {t for t in counts.values() if t is not None}
        if len(seen) > 1:
            raise ValueError(f"FusedClipAdamW.load_from: the groups' step counters disagree ({counts}); the fused update keeps one counter for all groups")
        for p, m, v in zip(params, self.m, self.v):
            st = opt.state.get(p, {})
            if "exp_avg" in st:
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
            else:
                m.zero_()
                v.zero_()
        self.step.fill_(seen.pop() if seen else 0.0)

    @torch.no_grad()
    def export(self, params=None):
        """the inverse of load_from: (first moments, second moments, update count) on the HOST, one tensor per parameter of `params` (default:
        this object's own order), copied tensor by tensor -- no second device copy of the moments; nothing of this object or the optimizer changes"""
        at = {id(p): i for i, p in enumerate(self.keep[0])}
        order = [at[id(p)] for p in (self.keep[0] if params is None else params)]
        return [step_state.to_host(self.m[i]) for i in order], [step_state.to_host(self.v[i]) for i in order], int(self.step.item())

    @torch.no_grad()
    def update(self):
        from . import ops
        if self.monitor is None:
            self.step.add_(1.0)
        if not self.norm_ready:
            if self.norm_table is not None:
                ops.grad_handover_raw(len(self.grads), self.norm_blocks, self.norm_table, self.norm_partial, self.norm)
            else:
                self.norm.copy_(torch.nn.utils.get_total_norm(self.grads, 2.0, foreach=True))
        self.norm_ready = False
        if self.report is not None:                           # behind the norm, in front of the update: the values the update reads
            self.report.record(self.norm)
        if self.group_table is not None:                      # several groups: the same two launches, hyper-parameters from the group table
            n_groups = len(self.plan.groups)
            if self.monitor is not None:
                ops.adamw_groups_guarded(self.n, self.blocks, self.desc, n_groups, self.group_of, self.group_table, self.step, self.norm, self.max_norm, self.hf)
                ops.guard_commit(self.norm, self.step, self.monitor.words)
                return
            ops.adamw_groups(self.n, self.blocks, self.desc, n_groups, self.group_of, self.group_table, self.step, self.norm, self.max_norm, self.hf)
            return
        if self.monitor is not None:                          # `step` is the count before this update; the commit advances it when the update ran
            ops.adamw_batch_guarded(self.n, self.blocks, self.desc, self.lr, self.step, self.norm, self.b1, self.b2, self.eps, self.wd, self.max_norm, self.hf)
            ops.guard_commit(self.norm, self.step, self.monitor.words)
            return
        ops.adamw_batch(self.n, self.blocks, self.desc, self.lr, self.step, self.norm, self.b1, self.b2, self.eps, self.wd, self.max_norm, self.hf)


def _pin_shadows(modules):
    """ops.PinnedShadows over the parameters of `modules` (PIN_SHADOWS = False: per-weight casts inside the graph, as before)"""
    if not PIN_SHADOWS:
        return None
    from . import ops
    seen, params = set(), []
    for m in modules:
        for p in m.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                params.append(p)
    return ops.PinnedShadows(params)


class FlatGradientTail:
    """What every graphed training step does behind its backward, stated once: the static flat fp32 gradient buffers the optimizer and the
    all-reduce work on (parallel.GradientAverager's buckets, hooks off: inside a replay no autograd hook fires), the hand-over of the fresh
    gradients into them, and the update (clip + optimizer step).  The steps differ only in the forward/backward in front of it.
    `flat`: a GradientAverager(hooks=False), or the parameters to build one over; `masters`: MasterWeights of a sub-module that runs in bf16 --
    `flat` and the optimizer are then over the fp32 masters (step_parameters); `exchanging`: a gradient exchange runs between hand_over() and
    update() (the caller's statement, read once: bool(flat.active) where the step exchanges); `capture_tables`: FusedHandOver's `captures`;
    `monitor` (a TrainMonitor): the update is skipped on a non-finite gradient norm (FusedClipAdamW) -- only with the fused update: the stock
    clip_grad_norm_ + opt.step() path cannot decide without a host synchronisation, so an optimizer FusedClipAdamW.eligible rejects is a
    ValueError.  With accumulation a bad micro-step makes the window's buffers non-finite: the window's one update is skipped and update()
    zeroes the buffers as always, so nothing of it reaches the next window.
    `report` (a GradReport): REPORT_NOTE -- handed to FusedClipAdamW, whose table it reads; likewise a ValueError without the fused update."""

    def __init__(self, flat, opt, clip, accumulate, masters=None, exchanging=False, capture_tables=4, monitor=None, report=None):
        from .parallel import GradientAverager
        if not isinstance(flat, GradientAverager):
            flat = list(flat)
        if report is not None and not FusedClipAdamW.eligible(opt, flat.params if isinstance(flat, GradientAverager) else flat):
            raise ValueError("grad_report needs the fused update (FusedClipAdamW.eligible: torch.optim.AdamW / HFAdamW whose parameter groups all hold a "
                             "device learning rate, over fp32 device parameters): the report runs over its descriptor table")
        self.report = report
        if monitor is not None and not FusedClipAdamW.eligible(opt, flat.params if isinstance(flat, GradientAverager) else flat):
            raise ValueError("skip_nonfinite needs the fused update (FusedClipAdamW.eligible: torch.optim.AdamW / HFAdamW whose parameter groups all hold a "
                             "device learning rate, over fp32 device parameters): the stock optimizer path cannot skip an update without a host synchronisation")
        self.monitor = monitor
        self.opt, self.clip, self.accumulate, self.masters, self.exchanging = opt, clip, bool(accumulate), masters, bool(exchanging)
        self.flat = flat if isinstance(flat, GradientAverager) else GradientAverager(flat, hooks=False)
        self.flat_view_of = {p: p.grad for p in self.flat.params}          # the averager made every .grad a view of its bucket
        low_of = {id(m): l for l, m in (masters.pairs() if masters is not None else [])}
        self.pairs = [(low_of.get(id(p), p), p) for p in self.flat.params]     # (parameter the model differentiates, parameter the optimizer steps)
        for l, m in self.pairs:
            l.grad = None
        self.fused = None
        if FusedClipAdamW.eligible(opt, self.flat.params):
            self.fused = FusedClipAdamW(opt, self.flat.params, self.flat_view_of, low_of, clip, monitor=monitor, report=report)
        # hand-over and clip norm in one pass; with an exchange between the hand-over and the update (N > 1) the hand-over still runs as one pass, its norm is
        # discarded and FusedClipAdamW.update takes the norm of the REDUCED buffers in one more launch
        self.handover = FusedHandOver(len(self.pairs), captures=capture_tables) if (self.fused is not None and FUSED_HANDOVER) else None

    def hand_over(self):
        """after a backward: the leaves' fresh gradients into the flat buffers (accumulation: added), .grad = None on the leaves -- one pass with the
        clip norm where FusedHandOver applies, _hand_over_gradients otherwise"""
        ran = self.handover is not None and self.handover(self.pairs, self.flat_view_of, self.accumulate, self.fused.norm)
        if not ran:
            _hand_over_gradients(self.pairs, self.flat_view_of, self.accumulate)
        # THE RULE for fused.norm_ready: the norm the hand-over left is usable exactly when the fused hand-over ran and no exchange follows it.
        # With an exchange behind it the norm is of the LOCAL gradients: FusedClipAdamW.update takes it again, of the reduced buffers.
        if self.fused is not None:
            self.fused.norm_ready = ran and not self.exchanging

    def update(self):
        if self.fused is not None:                           # norm + one launch: clip, AdamW, bf16 twins (FusedClipAdamW)
            self.fused.update()
        else:
            for p in self.flat.params:                       # the optimizer reads the static flat buffers
                p.grad = self.flat_view_of[p]
            torch.nn.utils.clip_grad_norm_(self.flat.params, self.clip)
            self.opt.step()
            if self.masters is not None:
                self.masters.sync_low()
        if self.accumulate:
            self.flat.zero_grad()
        for l, _ in self.pairs:                              # the next backward must produce fresh gradient tensors
            l.grad = None

    def replica_digest(self):
        """FusedClipAdamW.digest() of the parameters and moments this tail steps (compare across ranks: parallel.replicas_agree); only with the
        fused update, which owns the descriptor table -- ValueError otherwise, as skip_nonfinite"""
        if self.fused is None:
            raise ValueError("replica_digest needs the fused update (FusedClipAdamW.eligible: torch.optim.AdamW / HFAdamW whose parameter groups all hold a "
                             "device learning rate, over fp32 device parameters): the digest runs over its descriptor table")
        return self.fused.digest()

    def undo_warmup(self):
        """what the warm-up passes in front of a capture left in the optimizer and the flat buffers (graph_capture.warmup_undone calls it)"""
        _reset_optimizer_state(self.opt)
        if self.fused is not None:
            self.fused.reset()
        self.flat.zero_grad()
        if self.monitor is not None:                         # the warm-up's losses and updates are not the run's
            self.monitor.reset()
        if self.report is not None:
            self.report.reset()

    # -- the graphed half of a step's state_dict() / load_state_dict() (step_state.py; the eager half: step_state.EagerTail)
    def require_single_rank(self, what):
        if self.flat.active:
            raise NotImplementedError(f"{what}: one rank only (not with an active gradient exchange: per-rank generator state is not saved)")

    def optimizer_state(self):
        """the optimizer's state in its class's own layout, on the host: from FusedClipAdamW where the fused update keeps it (`optimizer.state` stays
        empty), from the optimizer otherwise"""
        if self.fused is None:
            return step_state.stock_optimizer_state(self.opt)
        return step_state.optimizer_state(self.opt, *self.fused.export(step_state.optimizer_params(self.opt)))

    def window(self):
        """the gradients of an open accumulation window: the flat views, in the optimizer's order, as fp32 host tensors"""
        return [step_state.to_host(self.flat_view_of[p]) for p in step_state.optimizer_params(self.opt)]

    def check_window(self, who):
        if any(p not in self.flat_view_of for p in step_state.optimizer_params(self.opt)):
            raise RuntimeError(f"{who}: the optimizer steps a parameter the flat gradient buffers do not hold")

    @torch.no_grad()
    def load(self, optimizer, window):
        """a checked optimizer state and window (None: no window is open) into the tensors the captured graphs address, in place"""
        step_state.load_optimizer_state(optimizer, self.opt, self.fused)
        if window is None:
            self.flat.zero_grad()
        else:
            for p, src in zip(step_state.optimizer_params(self.opt), window):
                self.flat_view_of[p].copy_(src)
        for l, _ in self.pairs:
            l.grad = None


def _default_mode_only(argument):
    """what GraphedTargetStep answers to `argument` (token_capacity, pad_rows, frame_capacity) together with one of its three side modes"""
    raise NotImplementedError(f"{argument}: the default single-graph mode, or the two-piece mode of an active gradient exchange (not with "
                              "pipeline_swin / branch_graphs / fork_streams)")


class GraphedTargetStep(StepState):
    """The whole target-task step as HIP graphs, replayed per step with one host call each -- two graphs (A = A1 + A2 as one, then B) on
    a single GPU, three when a gradient exchange has to be hidden (N > 1):

      A1 text encoder (forked onto a second stream) || Swin forward -> frame filter -> fusion stack -> cross-entropy ->
         backward through the fusion stack, the text encoder and Swin's head / stages 3-1, down to the gradient of Swin's stage-0
         output (SWIN_CUT); the multimodal gradients land in static flat fp32 buffers (parallel.GradientAverager's buckets, hooks off);
      -- N > 1: one asynchronous all-reduce per flat bucket is ISSUED here (the only collective of the step): the
         collectives run on the backend's stream behind A1 and BESIDE A2 --
      A2 the rest of Swin's backward from that gradient (stage 0: ~10 ms); Swin's parameter gradients land in buffers nobody reads
         (Swin's target-step gradients are discarded, train.py:20,141, and therefore never exchanged);
      -- N > 1: the stream waits for the collectives --
      B  clip_grad_norm_ + optimizer.step() (capturable) + zeroing of the flat buffers.

    Why: issued launch by launch the step costs ~75 ms of host time (Swin's ~600 launches through Python autograd and
    ctypes, ~800 AccumulateGrad nodes, clip_grad_norm_ over ~800 tensors, the optimizer) against ~80 ms of GPU time, so
    any kernel speed-up would disappear behind the host; two graph launches cost a few milliseconds.  Everything inside is
    capture-safe: no host synchronisation, DropPath / Gumbel / dropout noise from device-side generators, bf16 weight
    shadows re-cast inside the graph.  Shapes are static: __call__ copies the batch into the captured input buffers.
    `accumulation_steps` > 1 replays A that many times per B (gradients accumulate in the flat buffers).
    Parity: tests/test_gpu_train_step.py walks this against the eager TargetStep (same losses, same parameters)."""

    STATE_KIND, STATE_MODELS, STATE_WINDOW = TargetStep.STATE_KIND, TargetStep.STATE_MODELS, TargetStep.STATE_WINDOW

    # where the text branch's launches enter the capture order: "start" (in front of Swin's forward), "pe" (behind PatchEmbed), "s<i>"
    # (behind Swin stage i).  A class constant the probes patch (PATCH="train_step.GraphedTargetStep.TEXT_FORK_AT='s0'" tools/probes/bench_patch.py),
    # not an environment switch; measured in NOTES.md R5.3.
    TEXT_FORK_AT = "start"

    def __init__(self, swin_model, multimodal_model, optimizer, scheduler, args, batch, autocast_dtype=None,
                 overlap_text=True, parallel_fusion=False, averager=None, warmup_iters=2, masters=None, discarded_swin_gradients="compute",
                 swin_cut: int = 0, pipeline_swin: bool = False, branch_graphs: bool = False, fork_streams: bool = False, frame_capacity=None,
                 pad_rows: bool = False, skip_nonfinite: bool = False, color_jitter=None, grad_report: bool = False, token_capacity=None,
                 criterion=None):
        """`criterion` (None: F.cross_entropy, every launch as before): a Criterion.  CRITERION_NOTE: the loss a run chooses -- class weights, label
        smoothing -- is a construction argument of all six training steps like the optimizer's betas.  A graphed step captures ops.ce_loss in the
        place of F.cross_entropy (one launch per direction; GraphedUnimodalStep: the pooling head's _crit pair) in EVERY capture it makes (single
        graph, branch_graphs, every capacity, the padded twin); the launches address `criterion.weight`, so weights copied into that tensor between
        calls hold from the next replay on.  Padded rows (label -100) drop out of numerator and denominator; accumulation, skip_nonfinite, grad_report,
        parameter groups, augmentation and resuming are untouched, and the criterion is in no state_dict().  Several ranks: the ranks' weighted means
        are averaged; `global_rows` with class weights is a ValueError (check_criterion_rows).  Evaluation keeps the plain cross-entropy.
        `averager`: GradientAverager(hooks=False) over the parameters the optimizer steps (default: the multimodal
        model's); `swin_cut`: with an exchange to hide (N > 1), the Swin stage behind which the backward graph is cut (0: the second
        piece is stage 0's backward, ~10 ms; 1: stages 1 + 0, ~17 ms) -- the caller picks it from a MEASURED exchange time
        (`pick_swin_cut`, bench.py), never from a nominal link rate; `masters`: optional MasterWeights of the text encoder -- then `averager` and the optimizer must have been
        built over `step_parameters(multimodal_model, masters)`; `discarded_swin_gradients`: "compute" (default) / "skip", SKIP_NOTE;
        `pipeline_swin` (one rank, no exchange): Swin's FORWARD becomes a graph of its own (S) over two alternating sets of saved activations, and
        `step(batch, next_batch=...)` replays S for the NEXT batch on a second stream beside this batch's graph A' (frame filter, text encoder,
        fusion stack, loss, every backward).  Valid because nothing steps Swin in a target step (train.py:20,141: its target-step gradients are
        discarded) -- the prefetched forward sees the weights the in-order forward would; a Swin parameter whose version moved since the prefetch
        (an auxiliary step ran in between) makes the step redo the forward in order.  Why: per step ~22 ms of the GPU's time are streams of small
        launches at low occupancy (text encoder forward and the tail of its backward, the fusion stack, the update) that a 14 ms block of
        chip-filling Swin kernels can run beside; every step still executes exactly one Swin forward.
        `frame_capacity` (None: `frames` is the compact (sum num_imgs, ...) tensor and every batch must have the captured number of frames): an
        integer F_cap makes the step train on RAGGED batches with one capture.  The sample `batch` and every later one carry `frames` as the
        loader pads them, (B, Lv, ...), with num_imgs the real counts; the capture holds ops.pack_frames (real frames to the front of F_cap rows,
        the count in a device word) -> Swin on all F_cap rows with the head's BatchNorm over the real ones -> the frame filter with the same count.
        num_imgs as a list or CPU tensor (the reference's collate) is checked against F_cap on the host (ValueError); a device tensor is the
        caller's contract and `frame_counts` (int32 [n_valid, total], device) is there for a check at the end of an epoch.  The default
        single-graph mode and the two-piece mode of an active averager: NotImplementedError together with pipeline_swin / branch_graphs /
        fork_streams.
        An ascending tuple (c_1 < ... < c_k) ("buckets", `frame_buckets`) captures the forward/backward graph once per capacity -- pack into c_i rows,
        Swin on c_i rows, everything behind it as above -- and a call replays the smallest that holds its batch (`frame_bucket`: num_imgs on the
        host; more frames than c_k: ValueError before any copy or launch; a device tensor replays c_k unread).  The captures share the static
        inputs, the flat gradient buffers with the hand-over's destinations, graph B, the optimizer state and learning-rate word, the bf16
        shadows, the generator and `frame_counts`, so an accumulation window may mix capacities; each keeps its saved activations in a memory pool
        of its own (BUCKET_NOTE).  Under an active averager each capacity is a PAIR of graphs (A1_c, A2_c) in one pool, the exchange is issued
        between them from the host and only sees the flat buffers: ranks may replay different capacities in the same step.  A capacity below the sample batch's total is warmed up and captured on the sample's counts cut down to fit, and
        every warm-up is undone as the single one is.  `capacities`: the tuple; `capacity`: the last call's; `replays`: {capacity: calls};
        `capture_bytes` / `capture_reserved_bytes`: {capacity: growth of torch.cuda.memory_allocated / memory_reserved over its capture} (the
        saved activations are free blocks of the capture's private pool once it ends: the reserved figure is the memory a capacity costs).
        `pad_rows` (default False: a batch of another shape raises ValueError): a batch with 1 <= b <= B utterances whose other dimensions match is
        padded to the captured B by pad_target_batch (PAD_NOTE) and replayed through the same captures -- same flat buffers, same fused optimizer,
        same generator; the bucket is chosen from the padded num_imgs, which sum to the real frames; the loss is F.cross_entropy's mean over the
        real rows (label -100 is its ignore_index).  Nothing captured depends on B other than through shapes the padding keeps fixed: the only
        cross-row operations are the head's BatchNorm and the filter's "any face passed" (both over the device frame count) and the loss's mean.
        Needs frame_capacity (compact frames change shape with the batch: ValueError); not with pipeline_swin / branch_graphs / fork_streams
        (NotImplementedError, as frame_capacity).  `rows`: the real rows of the last call; `padded_calls`: the calls that padded.  Under an active
        averager ranks may hold different numbers of real rows: pass `global_rows` to the call (ROW_WEIGHT_NOTE).
        `skip_nonfinite`: GUARD_NOTE -- the learning-rate schedule advances on a skipped update too; several capacities share the one monitor.
        `grad_report`: REPORT_NOTE -- `step.grad_report`, a GradReport named by named_step_parameters(multimodal_model, masters).
        `color_jitter` (an augment.ColorJitter; None: no augmentation, the launches of before): the MELD train transform (utils/dataset.py:35-39,
        62-63) inside the uint8 pre-step.  The draw of the per-frame table is PART of every capture in front of Swin's forward (every capacity's, and
        graph S of pipeline_swin): one torch.rand on the device generator and elementwise launches, so every replay jitters anew and a resumed
        generator walks the same tables.  With a frame capacity the table has that many records (padded slots are jittered like any bytes: nothing
        reads them).  `last_jitter`: the table of the last Swin forward replayed (device, int32 (frames, 8)).  Frames must be uint8 (ValueError).
        `token_capacity` (PACK_NOTE; the default single-graph mode and the two-piece mode of an active averager, with or without frame capacities):
        the text encoder's layers and text_linear run on the real tokens of the batch packed into that many rows -- a fixed number, the captured
        shape.  None (default): the sample batch's real tokens rounded up to TOKEN_GRANULE (0 when its mask has a hole, or under pipeline_swin /
        branch_graphs / fork_streams); an integer: that many rows (NotImplementedError with those three modes); 0: the padded layout, the captures
        of before.  With packing on, every forward/backward graph is captured TWICE, on packed rows and on the padded layout (a pool each; the
        update graph, the flat buffers and the static inputs are shared): a call counts the real tokens of its mask on the host (count_tokens: a
        device mask costs one synchronisation per new tensor or version) and replays the packed capture when every row of the mask is a prefix
        of ones, the padded one when it has a hole; more real tokens than the capacity: ValueError before any copy or launch.  The setting holds
        for every frame capacity.  `token_capacity`: the rows; `token_replays`: {"packed": calls, "padded": calls}; `twin_capture_bytes` /
        `twin_capture_reserved_bytes`: {frame capacity, or None without one: what the padded twin's capture added}, as `capture_bytes` /
        `capture_reserved_bytes` say it of the packed captures -- a twin costs about what its packed capture costs, in memory and in capture time.
        The hand-over's pinned capture tables are sized for both sets (two per frame capacity)."""
        from . import ops
        from .parallel import GradientAverager
        if discarded_swin_gradients not in ("compute", "skip"):
            raise ValueError("discarded_swin_gradients: 'compute' or 'skip'")
        other_mode = bool(pipeline_swin or branch_graphs or fork_streams)
        box = token_box(multimodal_model)
        if token_capacity is None:
            token_capacity = 0 if (other_mode or box is None) else default_token_capacity(batch[1])
        self.token_capacity = int(token_capacity)
        if self.token_capacity and box is None:
            raise ValueError("token_capacity: the text encoder is not the fused bf16 encoder (MasterWeights / fuse_text_encoder) that can run on packed rows")
        if self.token_capacity < 0:
            raise ValueError("token_capacity: a number of rows, 0 (padded layout) or None (from the sample batch)")
        if self.token_capacity and other_mode:
            _default_mode_only("token_capacity")
        if self.token_capacity and not token_fit(batch[1], self.token_capacity):      # ValueError: the sample itself does not fit
            raise ValueError("token_capacity: the sample batch's text mask has a hole; the captures need a sample that packs")
        self.token_replays = {"packed": 0, "padded": 0}
        self.twin_capture_bytes, self.twin_capture_reserved_bytes = {}, {}
        self._rows_now = self.token_capacity                # what the pass in progress (warm-up, capture) runs the text branch with: _text_rows sets it on
                                                            # the model for the length of that forward only, so nobody else who calls the model ever packs
        self.criterion = _check_criterion(criterion, getattr(args, "num_labels", None))
        self.skip_swin_bwd = discarded_swin_gradients == "skip"
        self.pipeline = bool(pipeline_swin)
        self.branches = bool(branch_graphs)                 # BRANCH_NOTE at _capture_branches
        self.forked = bool(fork_streams)                    # FORK_NOTE at _fwd_bwd_forked
        self.pad_rows, self.rows, self.padded_calls = bool(pad_rows), None, 0
        if self.pad_rows and frame_capacity is None:
            raise ValueError("pad_rows: only with frame_capacity (compact frames change their shape with the batch's rows)")
        if self.pad_rows and other_mode:
            _default_mode_only("pad_rows")
        if (self.pad_rows or frame_capacity is not None) and bool(getattr(averager, "active", False)) and not isinstance(averager, GradientAverager):
            # the per-capacity pairs and the row weight are built on GradientAverager: its flat buffers are what the capacities share, its
            # world size is what weights the rows.  Another object that calls itself active is an exchange this step has no path for.
            raise NotImplementedError("pad_rows / frame_capacity under a gradient exchange: only with a parallel.GradientAverager(hooks=False)")
        self.capacities = frame_buckets(frame_capacity)    # None, (F_cap,) or the ascending buckets: ValueError before anything touches the GPU
        self.frame_capacity = None if self.capacities is None else self.capacities[-1]
        self.frame_counts = None
        self.capacity, self.replays, self.capture_bytes, self.capture_reserved_bytes = None, {c: 0 for c in self.capacities or ()}, {}, {}
        self._cap = self.frame_capacity                     # the capacity the pass in progress (warm-up, capture) packs into
        if self.frame_capacity is not None:
            if other_mode:
                _default_mode_only("frame_capacity")
            if batch[8].dim() < 3:
                raise ValueError("frame_capacity: a positive number of frames, and `frames` as the loader pads them, (B, Lv, ...)")
            check_frame_total(batch[9], batch[8].shape[1], self.frame_capacity)
        multi = self.capacities is not None and len(self.capacities) > 1
        require_packet_capture_off("GraphedTargetStep")
        self.swin, self.mm, self.opt, self.sched, self.args = swin_model, multimodal_model, optimizer, scheduler, args
        self.autocast_dtype = autocast_dtype
        self.i_batch = 0
        self.timing = None
        dev = batch[0].device
        self.color_jitter, self._jitter_buf = _check_color_jitter(color_jitter), None
        if self.color_jitter is not None:
            _need_u8_frames(torch.as_tensor(batch[8]))
            rows = self.frame_capacity if self.frame_capacity is not None else batch[8].shape[0]
            self._jitter_buf = torch.empty((rows, 8), dtype=torch.int32, device=dev)      # static: every capture's draw lands in its first rows
        # every batch entry becomes a static device tensor: a python list / int baked into the capture would silently be reused
        # by every replay (the reference's collate hands num_imgs and the utterance index over as lists)
        self.static = [t.clone() if torch.is_tensor(t) else torch.as_tensor(t, device=dev) for t in batch]
        # static flat gradient buffers for the multimodal parameters, hand-over and update: FlatGradientTail
        flat = averager if averager is not None else GradientAverager(step_parameters(self.mm, masters), hooks=False)
        if flat._handles:
            raise ValueError("GraphedTargetStep needs GradientAverager(..., hooks=False): the exchange runs between the graphs")
        self.monitor = TrainMonitor(dev) if skip_nonfinite else None
        self.grad_report = GradReport(named_step_parameters(self.mm, masters)) if grad_report else None
        # ROW_WEIGHT_NOTE.  Padded rows under an exchange: the all-reduce takes the mean of the ranks' means, which is the mean over the real rows
        # only when every rank holds as many.  One static fp32 word multiplies the loss that is DIFFERENTIATED (row_weight: b * world /
        # global_rows, filled per call; 1.0 without global_rows); the loss returned and the one the monitor counts stay the rank's own mean.
        # Captures without (pad_rows and an active exchange) have no such word and keep their launch sequence.
        self.row_weight = torch.ones((), dtype=torch.float32, device=dev) if (self.pad_rows and flat.active) else None
        self.tail = tail = FlatGradientTail(flat, optimizer, args.clip, args.trg_accumulation_steps > 1, masters=masters, exchanging=bool(flat.active),
                                            capture_tables=max(4, (2 if self.token_capacity else 1) * len(self.capacities or ())), monitor=self.monitor, report=self.grad_report)
        self.flat, self.flat_view_of, self.pairs, self.fused, self.handover = tail.flat, tail.flat_view_of, tail.pairs, tail.fused, tail.handover
        self.mm.text_stream = None
        # inside ONE graph the fork / join below become parallel branches; which hardware queue the branches replay on is the
        # runtime's choice at replay time, not a property of the stream object used during capture
        # warm-up / capture stream and the two branch streams: three different HIP streams (distinct_stream)
        cap = distinct_stream(dev)
        self.shadows = None                                 # set after the warm-up passes, before capture
        self.text_stream = distinct_stream(dev, (cap,)) if overlap_text else None
        self.mm.pair_stream = distinct_stream(dev, (cap, self.text_stream)) if parallel_fusion else None
        if self.forked:
            if self.text_stream is None:
                self.text_stream = distinct_stream(dev, (cap,))
            self.swin_stream = distinct_stream(dev, tuple(x for x in (cap, self.text_stream, self.mm.pair_stream) if x is not None))
            self._tick = torch.zeros(1, device=dev)
        # With an exchange to hide (N > 1) the forward/backward is TWO graphs, cut where the multimodal gradients are complete; alone on
        # the GPU it stays ONE graph: inside it the text encoder's backward runs as a branch beside Swin's backward, which a cut in
        # front of Swin's backward would serialise (measured at N = 1: 72.1 ms per step cut, 69 ms uncut).
        self.split = bool(getattr(self.flat, "active", False))
        if swin_cut not in (0, 1, 2):
            raise ValueError("swin_cut: 0, 1 or 2")
        self.SWIN_CUT = int(swin_cut)                      # the window behind the cut has to hold the exchange: see pick_swin_cut
        if self.pipeline and (self.split or self.skip_swin_bwd):
            raise ValueError("pipeline_swin: one rank without a gradient exchange, Swin's backward computed")
        if self.branches and (self.split or self.skip_swin_bwd or self.pipeline):
            raise ValueError("branch_graphs: one rank without a gradient exchange, Swin's backward computed, not together with pipeline_swin")
        if self.forked and (self.split or self.skip_swin_bwd or self.pipeline or self.branches):
            raise ValueError("fork_streams: one rank without a gradient exchange, Swin's backward computed, not together with pipeline_swin / branch_graphs")
        # -- warm-up on a side stream (lazy initialisations: kernel attributes, shadow caches, optimizer state), undone below
        snap = [(t, t.detach().clone()) for m in (self.swin, self.mm) for t in list(m.parameters()) + list(m.buffers())]
        if masters is not None:
            snap += [(t, t.detach().clone()) for t in masters.masters]
        # several capacities: ONE counts word for all captures, and every capacity gets its own warm-up passes (lazy initialisations are per shape) on
        # the sample's counts cut down to fit it (_clamp_counts) -- no shape of a pass depends on the counts, only on `_cap`.  After EACH
        # capacity's passes everything they touched is put back, as the single-capacity constructor does it
        self._counts_buf = torch.empty(2, dtype=torch.int32, device=dev) if multi else None
        for c in self.capacities or (None,):
            if multi:
                self._use_capacity(c, batch)
            with warmup_undone(snap, dev, cap, tail.undo_warmup):
                self._rows_now = self.token_capacity
                ran = box.packed_forwards if box is not None else 0
                for _ in range(warmup_iters):
                    self._fwd_bwd()
                    tail.update()
                if self.token_capacity and warmup_iters and box.packed_forwards == ran:
                    raise RuntimeError("token_capacity: the text encoder's forward did not run on packed rows (PACK_NOTE): no quiet padded capture")
                if self.token_capacity and warmup_iters:       # the padded twin's shapes have lazy initialisations of their own
                    self._rows_now = 0
                    self._fwd_bwd()
                    tail.update()
                    self._rows_now = self.token_capacity
                self.swin.zero_grad(set_to_none=True)
        del snap
        # -- capture
        self.shadows = _pin_shadows([self.swin, self.mm])
        self.swin_shadows = self.mm_shadows = None
        self._swin_params = [q for q in self.swin.parameters()]
        self.graph_a, self.graph_a2, self.graph_b = torch.cuda.CUDAGraph(), (torch.cuda.CUDAGraph() if self.split else None), torch.cuda.CUDAGraph()
        self.sets, self.side_stream, self.cur, self.prefetched = [], None, 0, None
        # the default mode's forward/backward captures, the ONE table __call__ looks a batch's up in: (frame capacity -- None without one --,
        # packed) -> a1, a2 (None unless split), loss, mask.  packed=True: the capture on packed token rows, and the only one with token_capacity
        # == 0; packed=False: its padded twin.  graph_a / graph_a2 / loss / new_mask are the sample batch's own record: largest capacity, packed
        self._captures = {}
        if self.pipeline:
            self._capture_pipelined(cap)
        elif self.branches:
            self._capture_branches(cap)
        else:
            caps = self.capacities or (None,)
            with capture_window(), ops.pinned_scope(self.shadows):
                for c in caps:
                    own = (self.graph_a, self.graph_a2) if c == caps[-1] else None
                    self._captures[c, True] = self._capture(c, True, batch, cap, own)
                # graph B reads none of a graph A's pool (the gradients have left it through the hand-over) and therefore runs behind whichever A
                # ran: with several capacities it gets a pool of its own as well (BUCKET_NOTE), with one it shares graph A's
                with torch.cuda.graph(self.graph_b, pool=None if multi else self.graph_a.pool(), stream=cap):
                    tail.update()
                if self.token_capacity:
                    # the padded twins (token_capacity above): per frame capacity the same forward/backward with the text encoder on the padded layout
                    for c in caps:
                        self._captures[c, False] = self._capture(c, False, batch, cap)
            self.loss, self.new_mask = self._captures[caps[-1], True].loss, self._captures[caps[-1], True].mask
        _KEEP_GRAPHS.append((self.graph_a, self.graph_a2, self.graph_b))
        if multi:
            self._use_capacity(self.capacities[-1], batch)  # the sample's own counts (they fit the largest capacity) back in the static input
        self.swin.zero_grad(set_to_none=True)              # drop the references; the graph's pool keeps the buffers
        self.mm.pair_stream = None
        self.flat.zero_grad()                              # the capture itself executes nothing

    def _capture(self, c, packed, batch, cap, graphs=None):
        """ONE forward/backward capture of the default mode, on stream `cap`: into frame capacity `c` (None: the step has none), with the text branch on
        packed token rows or (`packed` False: a padded twin) on the padded layout; into `graphs` = (A1, A2) -- the constructor's graph_a / graph_a2 for
        the sample batch's own capture -- or fresh ones.  Returns the record of `_captures`; the byte deltas go to capture_bytes / twin_capture_bytes
        (and their reserved twins) under `c`.
        Alone on the GPU the forward/backward is one graph (_fwd_bwd).  Split (an active exchange): a PAIR (A1, A2), A2 in A1's pool -- it continues
        from the activations A1 saved; the exchange between the two only sees the flat buffers, which no capacity sizes: ranks may replay different
        capacities in the same step.
        BUCKET_NOTE.  Every capture but the sample's own single one gets a memory pool of ITS OWN: a graph keeps its saved activations in its pool
        between its forward and its backward, and graphs that replay in an order the batches decide must not hand each other's blocks out.  Shared,
        because every capture addresses the same objects: the static inputs, the flat gradient buffers and the hand-over's destinations, the
        shadows, the generator, the counts word -- and graph B."""
        dev = self.static[0].device
        if self._counts_buf is not None:                    # several capacities: pack into `c`, on the sample's counts cut down to fit it
            self._use_capacity(c, batch)
        # every capture starts, as the first does, without Swin gradients: left in place, this capture's backward would ADD into an earlier one's --
        # ~170 more launches per replay, writing into that capture's pool.  Split, that includes the parameters above the cut, whose .grad A1
        # assigns (`late` in _fwd_bwd_multimodal)
        self.swin.zero_grad(set_to_none=True)
        self._rows_now = self.token_capacity if packed else 0
        a1, a2 = graphs if graphs is not None else (torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph() if self.split else None)
        before = (torch.cuda.memory_allocated(dev), torch.cuda.memory_reserved(dev))
        if self.split:
            with torch.cuda.graph(a1, stream=cap):
                loss, new_mask, swin_out = self._fwd_bwd_multimodal()
            with torch.cuda.graph(a2, pool=a1.pool(), stream=cap):
                self._bwd_swin(swin_out)
            del swin_out
        else:
            with torch.cuda.graph(a1, stream=cap):
                loss, new_mask = self._fwd_bwd()
        grew = (torch.cuda.memory_allocated(dev) - before[0], torch.cuda.memory_reserved(dev) - before[1])
        if not packed:                                      # a twin is recorded under None as well: a step without a frame capacity has one too
            self.twin_capture_bytes[c], self.twin_capture_reserved_bytes[c] = grew
        elif c is not None:
            self.capture_bytes[c], self.capture_reserved_bytes[c] = grew
        self._rows_now = self.token_capacity
        _KEEP_GRAPHS.append((a1, a2))
        return types.SimpleNamespace(a1=a1, a2=a2, loss=loss, mask=new_mask)

    # one micro-step: forward + backward (runs eagerly during warm-up, once more under capture), in the two pieces the graphs hold
    def _fwd_bwd(self):
        if getattr(self, "forked", False):
            return self._fwd_bwd_forked()
        loss, new_mask, _ = self._fwd_bwd_multimodal(whole=True)
        return loss, new_mask

    def _fwd_bwd_forked(self):
        """FORK_NOTE.  ONE graph whose two branches really start together.  The replay enqueues a graph branch by branch; the branch that CONTINUES on
        the launch queue (the fork node's first-created child) goes first and whole, and a branch that moves to another queue waits for the launch
        queue's tail as of then -- so with the text encoder (or Swin) as that first child the other branch starts when it has finished
        (profiles/r05_timeline*.txt).  Here the fork node's first child is a one-element tick on the launch queue that leads straight to the join; the
        text encoder and Swin are its second and third child, each on a stream of its own, and wait for a tail that ends at the tick.  Forward and
        backward are forked the same way (the backward by hand: the fusion stack is differentiated down to detached branch outputs, as branch_graphs)."""
        cap, ts, ss = torch.cuda.current_stream(), self.text_stream, self.swin_stream
        frames = self.static[8]
        if self.shadows is not None:
            self.shadows.refresh()
        ev = torch.cuda.Event()
        ev.record(cap)
        self._tick.add_(1.0)                                # first child of the fork: the launch queue's own continuation
        ts.wait_event(ev)
        ss.wait_event(ev)
        with torch.cuda.stream(ts):
            feat, tmask = self._text_forward(refresh=False)
        with torch.cuda.stream(ss):
            preds = self.swin(frames, is_trg_task=True, **self._draw_jitter(frames.shape[0]))
        cap.wait_stream(ts)
        cap.wait_stream(ss)
        for t in (feat, tmask, preds):
            if torch.is_tensor(t):
                t.record_stream(cap)
        loss, new_mask, dfeat, dpreds = self._fusion_fwd_bwd(feat, tmask, preds)
        ev2 = torch.cuda.Event()
        ev2.record(cap)
        self._tick.add_(1.0)
        ts.wait_event(ev2)
        ss.wait_event(ev2)
        if dfeat is not None:
            dfeat.record_stream(ts)
        if dpreds is not None:
            dpreds.record_stream(ss)
        with torch.cuda.stream(ts):
            self._text_backward(feat, dfeat, handover=False)
        with torch.cuda.stream(ss):
            self._bwd_swin((preds, dpreds))
        cap.wait_stream(ts)
        cap.wait_stream(ss)
        self.tail.hand_over()
        return loss, new_mask

    def _text_forward(self, refresh=True):
        """branch_graphs, graph T: the multimodal model's bf16 shadows (text encoder AND fusion stack: one launch), then the text branch"""
        (ids, attn_mask, sep_mask, _a, _am, _v, _vm, _l, _f, _n, utt_idx) = self.static
        if refresh and self.mm_shadows is not None:
            self.mm_shadows.refresh()
        with _autocast(self.autocast_dtype), _text_rows(self.mm, self._rows_now):
            return self.mm.text_branch(ids, attn_mask, sep_mask, torch.as_tensor(utt_idx, device=ids.device))

    def _fusion_fwd_bwd(self, feat, tmask, preds):
        """branch_graphs, graph F: frame filter, fusion stack, loss and their backward, down to detached copies of the two branch outputs;
        returns (loss, kept-frame mask, d(text features), d(Swin output)).  The fusion stack's parameter gradients are complete here."""
        (_i, _m, _s, audio, audio_mask, vision_inputs, vision_mask, labels, _f, num_imgs, _u) = self.static
        feat_d = feat.detach().requires_grad_(True)
        preds_d = preds.detach().requires_grad_(True)
        vis_concat, new_mask = select_frames(preds_d.float(), vision_inputs, vision_mask, num_imgs, self.args.FacialEmoImpor_threshold)
        with _autocast(self.autocast_dtype):
            logits = self.mm.fusion_branch(feat_d, tmask, audio, audio_mask, vis_concat, new_mask)
        loss = _loss_of(self.criterion, logits, labels) / self.args.trg_accumulation_steps
        leaves = [l for l, _ in self.pairs if l.requires_grad]
        got = torch.autograd.grad(loss, [feat_d, preds_d] + leaves, allow_unused=True)
        for l, gr in zip(leaves, got[2:]):
            l.grad = gr
        self._monitor_loss(loss)
        return loss.detach(), new_mask, got[0], got[1]

    def _text_backward(self, feat, dfeat, handover=True):
        """branch_graphs, graph TB: the text branch's backward from the gradient of its output, then the hand-over of EVERY multimodal gradient
        (graph F's included) to the optimizer's flat buffers with the clip norm in the same pass"""
        leaves = [l for l, _ in self.pairs if l.requires_grad]
        if dfeat is not None:
            got = torch.autograd.grad(feat, leaves, dfeat, allow_unused=True)
            for l, gr in zip(leaves, got):
                if gr is not None:
                    l.grad = gr if l.grad is None else l.grad + gr      # (a parameter both pieces use: none in this model)
        if handover:
            self.tail.hand_over()

    # branch_graphs and fork_streams are measured and not adopted (BRANCH_NOTE, FORK_NOTE).  They stay: bench.py passes both keywords on every
    # construction, and tests/test_gpu_train_step.py holds them to the in-order trajectory.
    def _capture_branches(self, cap):
        """branch_graphs: the constructor's captures on stream `cap` (_call_branches replays them)"""
        from . import ops
        dev, tail = self.static[0].device, self.tail
        # BRANCH_NOTE.  Inside ONE graph the text encoder and Swin are two branches, but the replay does not run them side by side: the
        # runtime enqueues a graph branch by branch, and a branch that continues on another queue waits for EVERYTHING the first branch
        # has enqueued so far, not for the node it depends on (profiles/r05_timeline.txt: the text encoder's forward runs alone for
        # ~4 ms in front of Swin's forward -- behind it when the capture order is swapped, TEXT_FORK_AT --, its backward starts ~12 ms
        # into Swin's backward and ends ~5 ms after it).  Here every branch is a graph of its own, launched on one of two streams with
        # events between them -- dependencies exactly where the data flow has them:
        #     side:  T  text encoder forward ............................ TB text encoder backward, hand-over | B update
        #     main:  S  Swin forward -> [T] F  frame filter, fusion stack, loss, its backward -> SB Swin backward
        # Autograd crosses the graph boundaries on detached copies of the two branch outputs (F differentiates down to them, TB / SB
        # continue from their gradients).  Pools: graphs that may run at the same time never share one (T, TB, B | S, SB | F).
        self.side_stream = distinct_stream(dev, (cap,))
        self.swin_shadows, self.mm_shadows = _pin_shadows([self.swin]), _pin_shadows([self.mm])
        g = types.SimpleNamespace(T=torch.cuda.CUDAGraph(), S=torch.cuda.CUDAGraph(), F=torch.cuda.CUDAGraph(), TB=torch.cuda.CUDAGraph(),
                                  SB=torch.cuda.CUDAGraph(), ev_t=torch.cuda.Event(), ev_f=torch.cuda.Event())
        with capture_window(), ops.pinned_scope(self.shadows):
            with torch.cuda.graph(g.T, stream=cap):
                feat, tmask = self._text_forward()
            with torch.cuda.graph(g.S, stream=cap):
                preds = self._swin_forward(self.static[8])
            with torch.cuda.graph(g.F, stream=cap):
                self.loss, self.new_mask, dfeat, dpreds = self._fusion_fwd_bwd(feat, tmask, preds)
            with torch.cuda.graph(g.TB, pool=g.T.pool(), stream=cap):
                self._text_backward(feat, dfeat)
            with torch.cuda.graph(g.SB, pool=g.S.pool(), stream=cap):
                self._bwd_swin((preds, dpreds))
            del feat, tmask, preds, dfeat, dpreds
            with torch.cuda.graph(self.graph_b, pool=g.T.pool(), stream=cap):
                tail.update()
        self.bg = g
        _KEEP_GRAPHS.append((g.T, g.S, g.F, g.TB, g.SB))

    def _call_branches(self, batch):
        g, main, side = self.bg, torch.cuda.current_stream(), self.side_stream
        main.wait_stream(side)                              # the previous step's side-stream work read the static inputs
        copy_into_static(self.static, batch, "GraphedTargetStep")
        side.wait_stream(main)
        with torch.cuda.stream(side):
            g.T.replay()
            g.ev_t.record(side)
        g.S.replay()
        main.wait_event(g.ev_t)
        g.F.replay()
        g.ev_f.record(main)
        side.wait_event(g.ev_f)
        self.i_batch += 1
        last = self.i_batch % self.args.trg_accumulation_steps == 0
        with torch.cuda.stream(side):
            g.TB.replay()
            if last:
                self.graph_b.replay()
        g.SB.replay()
        main.wait_stream(side)                              # what follows this call on the current stream sees the finished step
        if last:
            _bump_versions(self.flat.params)
            if self.sched is not None:
                self.sched.step()
        return self.loss, self.new_mask

    def _monitor_loss(self, loss):
        """skip_nonfinite: one launch behind the micro-step's loss that counts it in the monitor (undivided: times trg_accumulation_steps)"""
        if self.monitor is not None:
            self.monitor.loss(loss.detach(), self.args.trg_accumulation_steps)

    @property
    def last_jitter(self):
        """color_jitter: the table the last Swin forward ran with (a view of the static buffer the captured draws write)"""
        if self._jitter_buf is None:
            return None
        return self._jitter_buf[:self.capacity if self.capacities is not None and self.capacity is not None else self._jitter_buf.shape[0]]

    def _draw_jitter(self, n):
        """color_jitter: {} or the keyword that hands Swin a fresh table for n frames (a draw on the device generator, captured with the forward)"""
        if self.color_jitter is None:
            return {}
        table = self._jitter_buf[:n]
        table.copy_(self.color_jitter.draw(n, table.device))
        return {"jitter": table}

    def _swin_preds(self, frames, num_imgs):
        """Swin's target-task forward on the step's frames; with a frame capacity: packed on the device first (-> self.frame_counts)"""
        if self.frame_capacity is None:
            return self.swin(frames, is_trg_task=True, **self._draw_jitter(frames.shape[0]))
        from . import ops
        packed, self.frame_counts = ops.pack_frames(frames, num_imgs, self._cap, counts=self._counts_buf)
        return self.swin(packed, is_trg_task=True, n_valid=self.frame_counts, **self._draw_jitter(self._cap))

    def _use_capacity(self, c, batch):
        """several capacities: the next warm-up / capture packs into `c`, on the sample batch's counts cut down to fit it"""
        self._cap = c
        with torch.no_grad():
            self.static[9].copy_(torch.as_tensor(_clamp_counts(batch[9], batch[8].shape[1], c)))

    def _swin_forward(self, frames):
        """pipeline_swin, graph S: Swin's forward alone (its bf16 shadows refreshed at the head: an auxiliary step may have moved the weights)"""
        if self.swin_shadows is not None:
            self.swin_shadows.refresh()
        return self.swin(frames, is_trg_task=True, **self._draw_jitter(frames.shape[0]))

    def _fwd_bwd_multimodal(self, whole=False, preds=None):
        """forward of everything + backward of the loss down to (a) the multimodal parameters and (b) Swin's output; returns
        (loss, kept-frame mask, (Swin output, its gradient)) -- the second piece continues from the latter.  `preds` (pipeline_swin): Swin's
        output comes from graph S; this piece starts behind it and its backward runs through S's autograd graph."""
        (ids, attn_mask, sep_mask, audio, audio_mask, vision_inputs, vision_mask, labels, frames, num_imgs, utt_idx) = self.static
        mm, args = self.mm, self.args
        main = torch.cuda.current_stream()
        pending = None
        if preds is not None:
            if self.mm_shadows is not None:
                self.mm_shadows.refresh()                   # Swin's shadows belong to graph S
        elif self.shadows is not None:
            self.shadows.refresh()                          # every bf16 weight shadow of the step, one launch (ops.PinnedShadows)
        fork_hook = None
        if self.text_stream is not None:
            # fork: the text branch does not depend on the visual path.  WHERE its launches sit in the capture order decides when the
            # replay lets the other branch start (TEXT_FORK_AT below)
            fork_ev = torch.cuda.Event()
            fork_ev.record(main)
            box = {}

            def launch_text(*_):
                self.text_stream.wait_event(fork_ev)
                with torch.cuda.stream(self.text_stream), _autocast(self.autocast_dtype), _text_rows(mm, self._rows_now):
                    box["out"] = mm.text_branch(ids, attn_mask, sep_mask, torch.as_tensor(utt_idx, device=ids.device))

            where = self.TEXT_FORK_AT if preds is None and not self.skip_swin_bwd else "start"
            sw = getattr(self.swin, "swin", None)
            mod = None
            if where == "pe":
                mod = getattr(sw, "patch_embed", None)
            elif where.startswith("s") and where[1:].isdigit() and getattr(sw, "layers", None) is not None:
                mod = sw.layers[int(where[1:])]
            if mod is None:
                launch_text()
                pending = box["out"]
            else:
                fork_hook = mod.register_forward_hook(launch_text)
        cut, hook = {}, None
        if preds is not None:
            pass
        elif self.skip_swin_bwd:
            with torch.no_grad():
                preds = self._swin_preds(frames, num_imgs)
        else:
            if not whole:
                # two-piece backward: the cut goes INSIDE Swin, behind stage SWIN_CUT (below): the first piece then holds the text
                # encoder's backward beside Swin's head / stage-3 / -2 / -1 backward -- as the single graph does --, the second piece
                # Swin's stage-0 backward beside the gradient exchange.  (Cut at Swin's output, the text backward ran alone in front
                # of all of Swin's backward: 71.6 against 66.8 ms per step at one rank.)
                layers = getattr(getattr(self.swin, "swin", None), "layers", None)
                if layers is not None and len(layers) > self.SWIN_CUT + 1:
                    hook = layers[self.SWIN_CUT].register_forward_hook(lambda m, i, o: cut.__setitem__("x", o))
            preds = self._swin_preds(frames, num_imgs)
            if hook is not None:
                hook.remove()
            if fork_hook is not None:
                fork_hook.remove()
                if "out" not in box:                        # the hooked module was not called through __call__ on this path
                    launch_text()
                pending = box["out"]
        vis_concat, new_mask = select_frames(preds.float(), vision_inputs, vision_mask, num_imgs, args.FacialEmoImpor_threshold,
                                             self.frame_counts if self.frame_capacity is not None else None)
        with _autocast(self.autocast_dtype):
            if pending is None:
                with _text_rows(mm, self._rows_now):
                    pending = mm.text_branch(ids, attn_mask, sep_mask, torch.as_tensor(utt_idx, device=ids.device))
            else:
                main.wait_stream(self.text_stream)         # join
                for t in pending:
                    t.record_stream(main)
            logits = mm.fusion_branch(pending[0], pending[1], audio, audio_mask, vis_concat, new_mask)
        loss = _loss_of(self.criterion, logits, labels) / args.trg_accumulation_steps
        returned, w = loss, self.row_weight
        if w is not None:                                    # ROW_WEIGHT_NOTE: the gradients carry the weight, the loss handed back does not
            loss = loss * w
        if whole:                                            # one piece: autograd runs the text branch's backward beside Swin's
            loss.backward()
            self.tail.hand_over()
            self._monitor_loss(returned)
            return returned.detach(), new_mask, None
        # backward, first piece: every leaf the optimizer steps plus Swin's output (the autograd graph below `preds` -- Swin -- is
        # left untouched, with its saved activations, for the second piece)
        leaves = [l for l, _ in self.pairs if l.requires_grad]
        x_cut = cut.get("x") if torch.is_tensor(cut.get("x")) and cut["x"].requires_grad else None
        late = []
        if self.skip_swin_bwd:
            got = (None,) + tuple(torch.autograd.grad(loss, leaves, allow_unused=True))
        elif x_cut is not None:
            # Swin's parameters ABOVE the cut get their gradients in this piece (requested explicitly: autograd.grad computes nothing it is
            # not asked for, and the reference computes them)
            early = {id(q) for q in self.swin.swin.patch_embed.parameters()}
            for lyr in list(self.swin.swin.layers)[:self.SWIN_CUT + 1]:
                early |= {id(q) for q in lyr.parameters()}
            if getattr(self.swin.swin, "absolute_pos_embed", None) is not None:
                early.add(id(self.swin.swin.absolute_pos_embed))
            late = [q for q in self.swin.parameters() if q.requires_grad and id(q) not in early]
            got = torch.autograd.grad(loss, [x_cut] + leaves + late, allow_unused=True)
        else:
            x_cut = preds
            got = torch.autograd.grad(loss, [preds] + leaves, allow_unused=True)
        dpreds = got[0]
        for l, g in zip(leaves, got[1:1 + len(leaves)]):
            l.grad = g
        for q, g in zip(late, got[1 + len(leaves):]):        # discarded like all of Swin's target-step gradients (train.py:20,33)
            q.grad = g
        # (Letting the fused update read the model's own .grad tensors instead -- no hand-over, 2.8 GB less traffic -- was
        #  tried: the ~870 gradient tensors then stay allocated across the graph and the step got 2.8 ms SLOWER; not kept.)
        # N > 1 (two-piece backward): the same one-pass hand-over in front of the exchange; its norm is of the LOCAL gradients and is discarded
        self.tail.hand_over()
        self._monitor_loss(returned)
        return returned.detach(), new_mask, (x_cut, dpreds)

    # two-piece backward: cut behind Swin stage SWIN_CUT.  Measured at one rank with the exchange forced (ms per step, same call; the
    # single graph: 66.9): cut at Swin's output 71.6, behind stage 2: 72.3, stage 1: 70.9-71.0, stage 0: 69.7-69.9 -- the second piece
    # (stage 0's backward, ~10 ms) is the window the bucketed all-reduce of 0.87 GB has to fit into
    SWIN_CUT = 0                                         # class default; the instance's value is the constructor's `swin_cut`

    def _bwd_swin(self, swin_out):
        """backward, second piece: Swin from the gradient of its output.  Nobody reads the result in the target step (train.py:20,141
        zero Swin's gradients before the auxiliary task uses its optimizer); it is computed because the reference computes it."""
        preds, dpreds = swin_out
        if dpreds is not None:
            torch.autograd.backward(preds, dpreds)

    def _swin_version(self):
        ps = self._swin_params
        return (ps[0]._version, ps[-1]._version)

    def _launch_swin(self, k, frames):
        """graph S of set k for `frames` on the side stream: behind whatever produced `frames` (the current stream so far) and behind the last
        graph A' that read the set's activations"""
        st, side = self.sets[k], self.side_stream
        side.wait_stream(torch.cuda.current_stream())
        side.wait_event(st.ev_a)
        with torch.cuda.stream(side), torch.no_grad():
            if frames is not st.frames:
                if tuple(frames.shape) != tuple(st.frames.shape):
                    raise ValueError(f"GraphedTargetStep: frames of shape {tuple(frames.shape)}, the captured graphs are for {tuple(st.frames.shape)}")
                st.frames.copy_(frames, non_blocking=True)
                frames.record_stream(side)
            st.S.replay()
            st.ev_s.record(side)

    def _capture_pipelined(self, cap):
        """pipeline_swin: the constructor's captures on stream `cap` (_call_pipelined replays them)"""
        from . import ops
        dev, tail = self.static[0].device, self.tail
        # two sets (graph S: Swin forward; graph A': everything else), each in a memory pool of ITS OWN: S of one set replays beside A' of the
        # other, and inside a shared pool the capture of the second set would reuse blocks the first set's backward freed
        self.side_stream = distinct_stream(dev, tuple(x for x in (cap, self.text_stream, self.mm.pair_stream) if x is not None))
        self.swin_shadows, self.mm_shadows = _pin_shadows([self.swin]), _pin_shadows([self.mm])
        with capture_window(), ops.pinned_scope(self.shadows):
            for k in range(2):
                frames_k = self.static[8] if k == 0 else self.static[8].clone()
                g_s, g_a = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_s, stream=cap):
                    preds = self._swin_forward(frames_k)
                with torch.cuda.graph(g_a, pool=g_s.pool(), stream=cap):
                    loss, new_mask, _ = self._fwd_bwd_multimodal(whole=True, preds=preds)
                del preds
                self.sets.append(types.SimpleNamespace(S=g_s, A=g_a, frames=frames_k, loss=loss, mask=new_mask,
                                                       ev_s=torch.cuda.Event(), ev_a=torch.cuda.Event()))
                _KEEP_GRAPHS.append((g_s, g_a))
            with torch.cuda.graph(self.graph_b, stream=cap):
                tail.update()
        self.loss, self.new_mask = self.sets[0].loss, self.sets[0].mask

    def _call_pipelined(self, batch, next_batch):
        k, st = self.cur, self.sets[self.cur]
        copy_into_static(self.static, batch, "GraphedTargetStep", skip=(8,))      # the frames belong to graph S (_launch_swin)
        pf = self.prefetched
        if not (pf is not None and pf[0] == k and pf[1] is batch[8] and pf[2] == batch[8]._version and pf[3] == self._swin_version()):
            self._launch_swin(k, batch[8])                  # nothing (valid) prefetched: Swin's forward for this batch, in order
        self.prefetched = None
        if next_batch is not None:                          # enqueued BEFORE graph A': the two then run side by side
            self._launch_swin(k ^ 1, next_batch[8])
            self.prefetched = (k ^ 1, next_batch[8], next_batch[8]._version, self._swin_version())
        main = torch.cuda.current_stream()
        main.wait_event(st.ev_s)
        st.A.replay()
        st.ev_a.record(main)
        self.cur = k ^ 1
        replay_update(self, self.args.trg_accumulation_steps)
        self.loss, self.new_mask = st.loss, st.mask
        return st.loss, st.mask

    def __call__(self, batch, next_batch=None, global_rows=None):
        """`next_batch` (pipeline_swin only): the batch the NEXT call will be given -- its Swin forward is replayed now, beside this step.  Pass
        None in front of an auxiliary step (it moves Swin's weights: the prefetch would be thrown away) and for the last step of an epoch.
        `global_rows` (pad_rows under an active exchange only, ValueError otherwise): the real rows ALL ranks hold in this micro-step, which the
        caller knows from its sampler -- the gradients are then those of the mean over these rows (ROW_WEIGHT_NOTE, row_weight; an impossible
        value: ValueError before any copy or launch).  None: every rank holds the same number of real rows (DistributedSampler's contract).
        Under an exchange with several capacities every rank picks its own bucket from its own host counts; `replays`, `capacity`,
        `frame_counts`, `rows` and `padded_calls` are this rank's.  Not covered: a rank with no real row at all (b == 0 is refused)."""
        if len(batch) != len(self.static):
            raise ValueError(f"GraphedTargetStep: batch of {len(batch)} entries, captured with {len(self.static)}")
        check_criterion_rows("GraphedTargetStep", self.criterion, global_rows)
        if global_rows is not None and (self.pipeline or self.branches):
            raise ValueError("GraphedTargetStep: global_rows needs pad_rows=True and an active gradient exchange")
        if self.pipeline:
            return self._call_pipelined(batch, next_batch)
        if self.branches:
            return self._call_branches(batch)
        rows = self.static[7].shape[0]
        b = len(batch[7]) if self.pad_rows else rows
        weight = _check_global_rows("GraphedTargetStep", global_rows, self.row_weight, b, self.flat.world, rows)     # ValueError first of all
        if self.pad_rows and b != rows:
            batch = pad_target_batch(batch, rows)           # ValueError for b == 0 or b > rows, before any copy or launch
        packed = token_fit(batch[1], self.token_capacity)   # ValueError before any copy or launch; False: padding off, or a mask with a hole
        c = None
        if self.capacities is not None:
            # the smallest capacity that holds the batch (host counts; a device tensor: the largest, unread); ValueError before any copy or launch
            c = frame_bucket(batch[9], self.static[8].shape[1], self.capacities)
        rec = self._captures[c, packed or not self.token_capacity]      # padding off: the only capture per capacity is filed as the packed one
        copy_into_static(self.static, batch, "GraphedTargetStep")
        if self.row_weight is not None:
            self.row_weight.fill_(weight)                   # a device fill: no host synchronisation
        rec.a1.replay()
        self.loss, self.new_mask = rec.loss, rec.mask       # every capture has its own outputs
        self.rows = b
        self.padded_calls += int(b != rows)
        if self.capacities is not None:
            self.capacity = c
            self.replays[c] += 1
        if self.token_capacity:
            self.token_replays["packed" if packed else "padded"] += 1
        self.i_batch += 1
        last = self.i_batch % self.args.trg_accumulation_steps == 0
        if last:
            self.flat.exchange_begin()                     # no-op at world size 1; the collectives run beside graph A2
            if self.timing is not None:
                self.timing["begin"].record()
        if rec.a2 is not None:
            rec.a2.replay()
        if last:
            if self.timing is not None:
                self.timing["a2_done"].record()
            self.flat.exchange_end()
            if self.timing is not None:
                self.timing["end"].record()
            self.graph_b.replay()
            _bump_versions(self.flat.params)                # a replay changes the parameters behind autograd's back
            if self.sched is not None:
                self.sched.step()
        return self.loss, self.new_mask

    def replica_digest(self):
        """six int64 device words over the bits of every stepped parameter and its moments (FlatGradientTail.replica_digest; compare across
        ranks with parallel.replicas_agree); ValueError without the fused update"""
        return self.tail.replica_digest()

    def time_exchange(self, on: bool = True):
        """record three events per step around the exchange (issue / Swin backward enqueued / collectives waited for):
        `exchange_ms()` then returns (ms from issue to the end of the wait, ms of that the stream spent waiting AFTER graph A2)"""
        self.timing = {k: torch.cuda.Event(enable_timing=True) for k in ("begin", "a2_done", "end")} if on else None

    def exchange_ms(self):
        t = self.timing
        torch.cuda.synchronize()
        return t["begin"].elapsed_time(t["end"]), t["a2_done"].elapsed_time(t["end"])

    def start_epoch(self):
        """a partial accumulation window does not carry into the next epoch (train.py:52,54 restart the counter per epoch)"""
        self.i_batch = 0
        self.prefetched = None
        self.flat.zero_grad()


# GPU time of Swin's backward below a cut (ms, 640 frames bf16, profiles/r03_swin_kernel_stats.md): what the exchange can hide behind
SWIN_TAIL_MS = {0: 10.0, 1: 17.0, 2: 27.0}


def measure_swin_tail_ms(swin_model, frames, is_trg_task=True, passes: int = 2):
    """GPU time of Swin's backward BELOW each possible cut, measured on this device with this batch: {0: ms, 1: ms, 2: ms} (cut c: the
    backward of stages 0 .. c and the patch embedding -- the window the gradient exchange has to fit into).  HIP events recorded by backward
    hooks on the stages during `passes` eager forward + backward passes (the last one counts); no parameter is stepped, the gradients are
    dropped.  Replaces the table below, which is one box's profile (round-4 VERDICT weak 11)."""
    layers = list(swin_model.swin.layers)
    dev = frames.device
    out = {}
    for _ in range(max(1, passes)):
        evs = {}

        def mk(i):
            def hook(mod, gin, gout):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                evs[i] = e                                   # gradients of everything inside stage i are computed: the backward moves on to stage i - 1
            return hook
        hs = [layers[i].register_full_backward_hook(mk(i)) for i in range(len(layers))]
        try:
            x = frames.detach()
            if x.is_floating_point():
                x = x.clone().requires_grad_(True)           # so that stage 0's hook fires
            preds = swin_model(x, is_trg_task=is_trg_task)
            end = torch.cuda.Event(enable_timing=True)
            preds.float().square().mean().backward()
            end.record()
            torch.cuda.synchronize(dev)
        finally:
            for h in hs:
                h.remove()
        for q in swin_model.parameters():
            q.grad = None
        if all(i in evs for i in (1, 2, 3)) and len(layers) >= 4:
            out = {c: float(evs[c + 1].elapsed_time(end)) for c in (0, 1, 2)}
    return out


def pick_swin_cut(exchange_ms_alone: float, frames: int = 640, tail_ms: dict | None = None) -> int:
    """The lowest cut whose second piece is at least as long as the exchange MEASURED alone on this communicator (each step up costs
    ~1 ms of lost overlap between the text backward and Swin's, so the lowest that fits wins); 2 if none does.  tail_ms: the piece lengths
    measured on this device (measure_swin_tail_ms); without them the profiled table above, scaled by the frame count."""
    table = tail_ms if tail_ms else {c: SWIN_TAIL_MS[c] * (frames / 640.0) for c in (0, 1, 2)}
    for cut in (0, 1, 2):
        if table[cut] >= exchange_ms_alone:
            return cut
    return 2


class GraphedAuxStep(StepState):
    """The auxiliary-task step (train.py:15-41: Swin -> logits -> cross-entropy -> backward -> clip -> AdamW on the Swin
    model) as two HIP graphs, same construction as GraphedTargetStep; the Swin gradients are the exchanged ones here."""
    STATE_KIND, STATE_MODELS, STATE_WINDOW = "aux", ("swin",), "aux_accumulation_steps"

    def __init__(self, swin_model, optimizer, scheduler, args, images, labels, averager=None, warmup_iters=2, pad_rows: bool = False,
                 skip_nonfinite: bool = False, augment=None, grad_report: bool = False, criterion=None):
        """`criterion` (None: F.cross_entropy, every launch as before): a Criterion -- CRITERION_NOTE at GraphedTargetStep.
        `pad_rows` (default False: a batch of another shape raises ValueError): a batch with 1 <= b <= B images is padded to the captured B by
        pad_aux_batch (zero images, label -100) and replayed through the same graphs.  The capture then runs Swin with n_valid = a static int32
        device word that __call__ fills with b: the head's BatchNorm takes its statistics over the real rows only and a full batch
        (n_valid == B) gives the unmasked bits.  `rows`: the real rows of the last call; `padded_calls`: the calls that padded.
        Under an active averager `__call__(images, labels, global_rows=...)` weights the differentiated loss with row_weight (ROW_WEIGHT_NOTE at
        GraphedTargetStep): ranks that hold different numbers of real rows then step on the mean over all real rows.
        `skip_nonfinite`: GUARD_NOTE -- the learning-rate schedule advances on a skipped update too.
        `grad_report`: REPORT_NOTE -- `step.grad_report`, a GradReport named by swin_model.named_parameters().
        `augment` (an augment.AffWildAugment; None: no augmentation, the launches of before): the Aff-Wild2 train transform (utils/util.py:22-60)
        inside the uint8 pre-step.  The draw of the per-image table is PART of graph A, in front of Swin's forward: every replay augments anew and a
        resumed generator walks the same tables (nothing is added to state_dict()).  With pad_rows the padded zero images get records too; their
        rows stay out of BatchNorm and the loss.  `last_augment`: the table of the last replay (device, int32 (B, 20), a view of the static buffer
        the captured draw writes).  Images must be uint8 (ValueError, here and at the call)."""
        from . import ops
        from .parallel import GradientAverager
        self.swin, self.opt, self.sched, self.args = swin_model, optimizer, scheduler, args
        self.criterion = _check_criterion(criterion, getattr(args, "num_labels", None))
        self.augment, self.last_augment = _check_augment(augment), None
        if self.augment is not None:
            _need_u8_images(images)
            from ._lib import AUG_WORDS
            self.last_augment = torch.zeros((images.shape[0], AUG_WORDS), dtype=torch.int32, device=images.device)   # static: graph A's draw lands here
        self.static = [images.clone(), labels.clone()]
        self.pad_rows, self.rows, self.padded_calls = bool(pad_rows), None, 0
        self.n_valid = torch.full((1,), images.shape[0], dtype=torch.int32, device=images.device) if self.pad_rows else None
        self.shadows = None
        self.i_batch = 0
        dev = images.device
        flat = averager if averager is not None else GradientAverager(self.swin.parameters(), hooks=False)
        self.row_weight = torch.ones((), dtype=torch.float32, device=dev) if (self.pad_rows and flat.active) else None
        self.monitor = TrainMonitor(dev) if skip_nonfinite else None
        self.grad_report = GradReport(self.swin.named_parameters()) if grad_report else None
        self.tail = tail = FlatGradientTail(flat, optimizer, args.clip, args.aux_accumulation_steps > 1, exchanging=bool(flat.active), monitor=self.monitor,
                                            report=self.grad_report)
        self.flat, self.flat_view_of, self.pairs, self.fused, self.handover = tail.flat, tail.flat_view_of, tail.pairs, tail.fused, tail.handover
        snap = [(t, t.detach().clone()) for t in list(self.swin.parameters()) + list(self.swin.buffers())]
        cap = distinct_stream(dev)
        with warmup_undone(snap, dev, cap, tail.undo_warmup):
            for _ in range(warmup_iters):
                self._fwd_bwd()
                tail.update()
        del snap
        self.shadows = _pin_shadows([self.swin])
        self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with capture_window(), ops.pinned_scope(self.shadows):
            with torch.cuda.graph(self.graph_a, stream=cap):
                self.loss = self._fwd_bwd()
            with torch.cuda.graph(self.graph_b, pool=self.graph_a.pool(), stream=cap):
                tail.update()
        _KEEP_GRAPHS.append((self.graph_a, self.graph_b))
        self.flat.zero_grad()

    def _fwd_bwd(self):
        if self.shadows is not None:
            self.shadows.refresh()
        images, labels = self.static
        kw = {}
        if self.augment is not None:                         # one record per image of the captured batch, drawn just ahead of Swin
            self.last_augment.copy_(self.augment.draw(images.shape[0], images.device))
            kw["augment"] = self.last_augment
        crit = F.cross_entropy if self.criterion is None else self.criterion
        if self.pad_rows:
            loss = self.swin(images, False, labels, crit, n_valid=self.n_valid, **kw) / self.args.aux_accumulation_steps
        else:
            loss = self.swin(images, False, labels, crit, **kw) / self.args.aux_accumulation_steps
        (loss if self.row_weight is None else loss * self.row_weight).backward()
        self.tail.hand_over()
        if self.monitor is not None:
            self.monitor.loss(loss.detach(), self.args.aux_accumulation_steps)
        return loss.detach()

    def __call__(self, images, labels, global_rows=None):
        """`global_rows`: GraphedTargetStep.__call__'s -- the real rows all ranks hold in this micro-step; pad_rows under an active exchange only"""
        if self.augment is not None:
            _need_u8_images(images)                          # ValueError before anything is copied or launched
        check_criterion_rows("GraphedAuxStep", self.criterion, global_rows)
        rows = b = self.static[0].shape[0]
        padding = self.pad_rows and images.dim() == self.static[0].dim() and images.shape[0] != rows
        if padding:
            b = images.shape[0]
        weight = _check_global_rows("GraphedAuxStep", global_rows, self.row_weight, b, self.flat.world, rows)     # ValueError first of all
        if padding:
            images, labels = pad_aux_batch(images, labels, rows)     # ValueError for b == 0 or b > rows, before any copy or launch
        copy_into_static(self.static, (images, labels), "GraphedAuxStep")
        if self.row_weight is not None:
            self.row_weight.fill_(weight)
        if self.n_valid is not None:
            self.n_valid.fill_(b)                            # a device fill: no host synchronisation
        self.graph_a.replay()
        self.rows = b
        self.padded_calls += int(b != rows)
        replay_update(self, self.args.aux_accumulation_steps, self.flat.exchange_all)     # Swin's gradients: 187 MB fp32, nothing left in the step to hide them behind
        return self.loss

    def replica_digest(self):
        """GraphedTargetStep.replica_digest's, over Swin's parameters and moments"""
        return self.tail.replica_digest()

    def start_epoch(self):
        """a partial accumulation window does not carry into the next epoch (train.py:17,20 restart per epoch)"""
        self.i_batch = 0
        self.flat.zero_grad()


class AuxStep(StepState):
    """One auxiliary-task (Aff-Wild2 frame classification) step, train.py:15-41: Swin -> logits (no Gumbel)
    -> cross-entropy -> backward -> clip (0.8) -> AdamW on the Swin model (aux_lr 5e-5) every
    `aux_accumulation_steps`.  BASELINE.json configs[4] alternates these steps with target steps per epoch."""
    STATE_KIND, STATE_MODELS, STATE_WINDOW = GraphedAuxStep.STATE_KIND, GraphedAuxStep.STATE_MODELS, GraphedAuxStep.STATE_WINDOW

    def __init__(self, swin_model, optimizer, scheduler, args, augment=None, criterion=None):
        """`criterion` (None: F.cross_entropy): a Criterion -- CRITERION_NOTE at GraphedTargetStep.
        `augment` (an augment.AffWildAugment; None: no augmentation): the Aff-Wild2 train transform (utils/util.py:22-60) on the uint8 images,
        inside the pre-step -- every call draws a table from the device generator, one record per image, and keeps it in `last_augment`."""
        self.swin, self.opt, self.sched, self.args = swin_model, optimizer, scheduler, args
        self.i_batch = 0
        self.augment, self.last_augment = _check_augment(augment), None
        self.criterion = _check_criterion(criterion, getattr(args, "num_labels", None))

    def __call__(self, images, labels):
        kw = {}
        if self.augment is not None:
            _need_u8_images(images)                          # ValueError before anything is launched
            self.last_augment = kw["augment"] = self.augment.draw(images.shape[0], images.device)
        loss = self.swin(images, False, labels, F.cross_entropy if self.criterion is None else self.criterion, **kw) / self.args.aux_accumulation_steps
        loss.backward()
        self.i_batch += 1
        if self.i_batch % self.args.aux_accumulation_steps == 0:
            torch.nn.utils.clip_grad_norm_(self.swin.parameters(), self.args.clip)
            self.opt.step()
            if self.sched is not None:
                self.sched.step()
            self.opt.zero_grad(set_to_none=True)
        return loss.detach()


class UnimodalStep(StepState):
    """One V-only training step, train.py:245-273 (choice_modality 'V'): meld_utt_transformer on pre-extracted face features -> cross-entropy /
    trg_accumulation_steps -> backward; every trg_accumulation_steps micro-steps clip over the model's parameters (args.clip), optimizer step,
    scheduler step, gradients cleared.  batch = (modality_feature, utterance_mask, labels); returns the detached micro-loss.  The tail behind the
    encoder -- pooling, dropout, classifier, loss -- is models.meld_utt_transformer.forward_loss (ops.pool_head_loss)."""
    STATE_KIND, STATE_MODELS, STATE_WINDOW = "unimodal", ("model",), "trg_accumulation_steps"

    def __init__(self, model, optimizer, scheduler, args, criterion=None):
        """`criterion` (None: the plain cross-entropy of the pooling head): a Criterion -- CRITERION_NOTE at GraphedTargetStep"""
        self.model, self.opt, self.sched, self.args = model, optimizer, scheduler, args
        self.criterion = _check_criterion(criterion, getattr(args, "num_labels", None))
        self.i_batch = 0

    def __call__(self, batch):
        feature, mask, labels = batch
        kw = {} if self.criterion is None else {"criterion": self.criterion}
        loss, _ = self.model.forward_loss(feature, mask, labels, **kw)
        loss = loss / self.args.trg_accumulation_steps
        loss.backward()
        self.i_batch += 1
        if self.i_batch % self.args.trg_accumulation_steps == 0:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.args.clip)
            self.opt.step()
            if self.sched is not None:
                self.sched.step()
            self.opt.zero_grad(set_to_none=True)
        return loss.detach()

    def start_epoch(self):
        """a partial accumulation window does not carry into the next epoch (train.py:250-251 restart per epoch)"""
        self.i_batch = 0
        self.opt.zero_grad(set_to_none=True)


class GraphedUnimodalStep(StepState):
    """UnimodalStep as two HIP graphs, the construction of GraphedAuxStep: graph A = bf16 shadow refresh, forward_loss, backward, gradient hand-over into
    flat fp32 buffers (+ the clip norm); graph B = clip + optimizer step (one fused launch for AdamW / HFAdamW with a device learning rate).  The warm-up
    passes run on a side stream and are undone (parameter snapshot, optimizer state zeroed); the dropout seeds are drawn on the device inside graph A,
    so every replay draws fresh masks.  The batch shape is the captured one: another shape raises ValueError.  A short last batch of an epoch must NOT
    go through an eager UnimodalStep on the same model and optimizer: with the fused optimizer on, the moments and the step counter live in
    FusedClipAdamW and `optimizer.state` is empty, so the eager update would start Adam from zero for that one step and the graphs would continue
    with moments that never saw it; with trg_accumulation_steps > 1 the eager micro-step accumulates in p.grad, which graph B never reads.
    `pad_rows=True` is the way: the capture runs forward_loss(..., valid_mean=True) -- the loss is the mean over the rows that have a label, the
    same bits as the plain loss on a full batch --, and a batch with 1 <= b <= B rows is padded to B by pad_unimodal_batch (copies of row 0, label
    -100) and replayed through the same graphs, flat buffers and optimizer state; the loss returned is the mean over the b real rows /
    trg_accumulation_steps.  `rows`: the real rows of the last call; `padded_calls`: the calls that padded.
    `skip_nonfinite`: GUARD_NOTE -- the learning-rate schedule advances on a skipped update too.
    `grad_report`: REPORT_NOTE -- `step.grad_report`, a GradReport named by model.named_parameters().
    `averager` (default None: this step never exchanges): a GradientAverager(hooks=False) over the model's parameters -- its buckets are averaged
    over the ranks between graph A and graph B of a window's last micro-step, as GraphedAuxStep does it; with pad_rows the call then takes
    `global_rows` (ROW_WEIGHT_NOTE at GraphedTargetStep).
    `criterion` (None: the plain or _rows head, every launch as before): a Criterion -- CRITERION_NOTE at GraphedTargetStep; the capture then runs
    the pooling head's _crit pair, whose mean runs over the labelled rows with or without pad_rows."""
    STATE_KIND, STATE_MODELS, STATE_WINDOW = UnimodalStep.STATE_KIND, UnimodalStep.STATE_MODELS, UnimodalStep.STATE_WINDOW

    def __init__(self, model, optimizer, scheduler, args, batch, autocast_dtype=None, warmup_iters=2, pad_rows: bool = False,
                 skip_nonfinite: bool = False, averager=None, grad_report: bool = False, criterion=None):
        from . import ops
        self.model, self.opt, self.sched, self.args = model, optimizer, scheduler, args
        self.criterion = _check_criterion(criterion, getattr(args, "num_labels", None))
        self.autocast_dtype = autocast_dtype
        feature, mask, labels = batch
        self.static = [feature.clone(), mask.clone(), torch.as_tensor(labels, device=feature.device).clone()]
        self.pad_rows, self.rows, self.padded_calls = bool(pad_rows), None, 0
        self.shadows = None
        self.i_batch = 0
        dev = feature.device
        # without an averager this step never exchanges (exchanging=False): the hand-over's norm is then always the update's
        if averager is not None and averager._handles:
            raise ValueError("GraphedUnimodalStep needs GradientAverager(..., hooks=False): the exchange runs between the graphs")
        self.exchange = averager.exchange_all if averager is not None else None
        self.row_weight = torch.ones((), dtype=torch.float32, device=dev) if (self.pad_rows and averager is not None and averager.active) else None
        self.monitor = TrainMonitor(dev) if skip_nonfinite else None
        self.grad_report = GradReport(self.model.named_parameters()) if grad_report else None
        self.tail = tail = FlatGradientTail(averager if averager is not None else self.model.parameters(), optimizer, args.clip,
                                            args.trg_accumulation_steps > 1, exchanging=bool(averager is not None and averager.active), monitor=self.monitor,
                                            report=self.grad_report)
        self.flat, self.flat_view_of, self.pairs, self.fused, self.handover = tail.flat, tail.flat_view_of, tail.pairs, tail.fused, tail.handover
        snap = [(t, t.detach().clone()) for t in list(self.model.parameters()) + list(self.model.buffers())]
        cap = distinct_stream(dev)
        with warmup_undone(snap, dev, cap, tail.undo_warmup):
            for _ in range(warmup_iters):
                self._fwd_bwd()
                tail.update()
        del snap
        self.shadows = _pin_shadows([self.model])
        self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with capture_window(), ops.pinned_scope(self.shadows):
            with torch.cuda.graph(self.graph_a, stream=cap):
                self.loss = self._fwd_bwd()
            with torch.cuda.graph(self.graph_b, pool=self.graph_a.pool(), stream=cap):
                tail.update()
        _KEEP_GRAPHS.append((self.graph_a, self.graph_b))
        self.flat.zero_grad()

    def _fwd_bwd(self):
        if self.shadows is not None:
            self.shadows.refresh()
        kw = {"valid_mean": True} if self.pad_rows else {}
        if self.criterion is not None:
            kw["criterion"] = self.criterion
        feature, mask, labels = self.static
        with _autocast(self.autocast_dtype, cache_enabled=False):
            loss, logits = self.model.forward_loss(feature, mask, labels, **kw)
        self.logits = logits.detach()
        loss = loss / self.args.trg_accumulation_steps
        (loss if self.row_weight is None else loss * self.row_weight).backward()
        self.tail.hand_over()
        if self.monitor is not None:
            self.monitor.loss(loss.detach(), self.args.trg_accumulation_steps)
        return loss.detach()

    def __call__(self, batch, global_rows=None):
        """`global_rows`: GraphedTargetStep.__call__'s -- the real rows all ranks hold in this micro-step; pad_rows under an active exchange only"""
        feature, mask, labels = batch
        check_criterion_rows("GraphedUnimodalStep", self.criterion, global_rows)
        rows = b = self.static[0].shape[0]
        padding = self.pad_rows and feature.dim() == self.static[0].dim() and feature.shape[0] != rows
        if padding:
            b = feature.shape[0]
        weight = _check_global_rows("GraphedUnimodalStep", global_rows, self.row_weight, b, self.flat.world, rows)     # ValueError first of all
        if padding:
            feature, mask, labels = pad_unimodal_batch(batch, rows)     # ValueError for b == 0 or b > rows, before any copy or launch
        copy_into_static(self.static, (feature, mask, labels), "GraphedUnimodalStep")
        if self.row_weight is not None:
            self.row_weight.fill_(weight)
        self.graph_a.replay()
        self.rows = b
        self.padded_calls += int(b != rows)
        replay_update(self, self.args.trg_accumulation_steps, self.exchange)
        return self.loss

    def replica_digest(self):
        """GraphedTargetStep.replica_digest's, over the model's parameters and moments"""
        return self.tail.replica_digest()

    def start_epoch(self):
        """a partial accumulation window does not carry into the next epoch (train.py:250-251 restart per epoch)"""
        self.i_batch = 0
        self.flat.zero_grad()
