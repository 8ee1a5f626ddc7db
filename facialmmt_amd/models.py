"""Task models; host-side mirror of the reference's src/models.py (callers of
the hot path, API preserved): same class names, constructor arguments (an argparse-style namespace),
attribute names / state_dict keys and forward signatures.  The Swin backbone, the two cross-modal encoders,
the per-modality self-attention encoders and the P-projection of the additive-attention pooling run on
libfmmt_hip; the text encoder stays the HuggingFace RoBERTa/BERT on PyTorch-ROCm, and the three input
projections whose widths the kernels' 16-byte alignment excludes (audio 300, vision 519, classifier -> 7)
stay nn.Linear.

Differences from the reference, on purpose:
  * no hard-coded .cuda() (ref src/models.py:114-115): buffers are created on the input's device;
  * the per-utterance token slicing (ref :112-150), a Python double loop with one host sync per token,
    is restated as cumsum + gather on the device with no host synchronisation (same result; pinned by
    tests/test_host_cpu.py::test_slice_target_utterance_matches_literal_loop and, on device tensors,
    tests/test_gpu_glue.py against a literal loop);
  * the activations handed to the HIP encoders are cast to the compute dtype of the module
    (`compute_dtype`, bf16 for throughput / fp32 for parity) and back."""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .modules.CrossmodalTransformer import CrossModalTransformerEncoder
from .modules.SwinTransformer.backbone_def import BackboneFactory
from .modules.Transformer import AdditiveAttention, MELDTransEncoder


class InputProjection(nn.Linear):
    """nn.Linear (same parameters, same state_dict keys) for the audio / vision input projections (src/models.py:66-67): vendor GEMMs as
    autograd would call them, the bias gradient through fmmt_colsum (ops.VendorLinearFn).  Why not the stock module: inside the replayed
    multi-stream HIP graph of train_step.GraphedTargetStep torch's own bias-gradient reduction of these two layers was not reproducible
    (16-48 of 768 sums off by up to 3 % of the largest in most replays, the gradient that reaches the layer bit-identical:
    tests/support_replay_step.py); the column-sum launch is."""

    def forward(self, x):
        if self.bias is None or not x.is_cuda or not torch.is_grad_enabled() or self.weight.shape[0] % 8:
            return super().forward(x)
        from . import ops
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else x.dtype
        if dt not in (torch.bfloat16, torch.float32):
            return super().forward(x)
        with torch.autocast("cuda", enabled=False):          # the casts autocast would insert, spelled out (differentiable)
            return ops.VendorLinearFn.apply(x.to(dt), self.weight.to(dt), self.bias.to(dt))

DEFAULT_SWIN_CONF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "modules", "SwinTransformer", "swin_conf.yaml")


class SwinForAffwildClassification(nn.Module):
    """Swin features -> Linear(512,64) -> ReLU -> Linear(64,num_labels) [-> Gumbel-softmax on the
    target task] [-> loss]  (ref src/models.py:14-37)."""

    def __init__(self, args):
        super().__init__()
        self.num_labels = args.num_labels
        self.swin = BackboneFactory(args.backbone_type, args.backbone_conf_file).get_backbone()
        self.linear = nn.Linear(512, 64)
        self.nonlinear = nn.ReLU()
        self.classifier = nn.Linear(64, args.num_labels)
        self.tau = args.tau

    def forward(self, images_feature=None, is_trg_task=None, labels=None, criterion=None, n_valid=None, jitter=None, augment=None):
        """jitter (None: no augmentation): augment.ColorJitter's table for uint8 images_feature -- the MELD train transform; the auxiliary task never passes one.
        augment (None: no augmentation): augment.AffWildAugment's table for uint8 images_feature -- the Aff-Wild2 train transform of the auxiliary task"""
        kw = {} if jitter is None else {"jitter": jitter}
        if augment is not None:
            kw["augment"] = augment
        feats = self.swin(images_feature, **kw) if n_valid is None else self.swin(images_feature, n_valid=n_valid, **kw)
        logits = self.classifier(self.nonlinear(self.linear(feats.to(self.linear.weight.dtype))))
        if is_trg_task:
            logits = F.gumbel_softmax(logits, self.tau)
        if labels is not None:
            return criterion(logits, labels)
        return logits


def slice_target_utterance(text_feats, sep_mask, utt_idx, max_len: int, roberta: bool):
    """Word-level features of the target utterance of each dialogue (ref src/models.py:112-150).

    text_feats (B, T, H); sep_mask (B, T) marks each utterance's closing separator; utt_idx (B,) is the
    position of the target utterance in its dialogue.  Utterance 0 spans tokens [1, first_sep); utterance
    u > 0 spans [prev_sep + (2 if roberta else 1), cur_sep); at most max_len tokens are kept; rows whose
    dialogue has fewer than u+1 separators stay zero.  Returns (features (B,max_len,H), mask (B,max_len))."""
    B, T, H = text_feats.shape
    dev = text_feats.device
    sep = sep_mask.to(dev) == 1
    order = torch.cumsum(sep.long(), dim=1)                                    # 1-based rank of each separator
    u = torch.as_tensor(utt_idx, device=dev).long().view(B, 1)
    is_cur = sep & (order == u + 1)
    is_prev = sep & (order == u)
    has_cur = is_cur.any(dim=1)
    cur = torch.argmax(is_cur.long(), dim=1)
    prev = torch.argmax(is_prev.long(), dim=1)
    first = u.view(B) == 0
    gap = 2 if roberta else 1
    start = torch.where(first, torch.ones_like(cur), prev + gap)
    length = torch.where(first, cur - 1, cur - prev - gap)
    length = torch.where(has_cur, length, torch.zeros_like(length)).clamp(min=0, max=max_len)
    t = torch.arange(max_len, device=dev).view(1, max_len)
    keep = t < length.view(B, 1)
    idx = (start.view(B, 1) + t).clamp(max=T - 1)
    out = torch.gather(text_feats, 1, idx.unsqueeze(-1).expand(B, max_len, H)) * keep.unsqueeze(-1).to(text_feats.dtype)
    return out, keep.to(torch.float32)


class MultiModalTransformerForClassification(nn.Module):
    """PLM -> target-utterance slicing; audio / vision linear + self-attention encoders; four cross-modal
    encoder calls; additive-attention pooling; classifier (ref src/models.py:41-188)."""

    def __init__(self, config):
        super().__init__()
        self.choice_modality = config.choice_modality
        self.num_labels = config.num_labels
        self.get_text_utt_max_lens = config.get_text_utt_max_lens
        self.hidden_size = config.hidden_size
        self.text_pretrained_model = 'roberta' if config.pretrainedtextmodel_path.split('/')[-1] == 'roberta-large' else 'bert'
        self.audio_emb_dim = config.audio_featExtr_dim
        self.audio_utt_Transformernum = config.audio_utt_Transformernum
        self.get_audio_utt_max_lens = config.get_audio_utt_max_lens
        self.crossmodal_num_heads_TA = config.crossmodal_num_heads_TA
        self.crossmodal_layers_TA = config.crossmodal_layers_TA
        self.crossmodal_attn_dropout_TA = config.crossmodal_attn_dropout_TA
        self.crossmodal_num_heads_TA_V = config.crossmodal_num_heads_TA_V
        self.crossmodal_layers_TA_V = config.crossmodal_layers_TA_V
        self.crossmodal_attn_dropout_TA_V = config.crossmodal_attn_dropout_TA_V
        self.vision_emb_dim = config.vision_featExtr_dim + config.num_labels
        self.vision_utt_Transformernum = config.vision_utt_Transformernum
        self.get_vision_utt_max_lens = config.get_vision_utt_max_lens
        self.compute_dtype = getattr(config, "compute_dtype", torch.float32)
        # True: the two directions of each cross-modal encoder run as one sweep over their stacked tokens (same result up to the summation
        # order of the shared weights' gradients); False: two encoder calls per pair, as the reference spells it
        self.stack_directions = bool(getattr(config, "stack_directions", True))

        plm = self._build_plm(config)
        if self.text_pretrained_model == 'roberta':
            self.roberta = plm
        else:
            self.bert = plm
        self.text_linear = InputProjection(plm.config.hidden_size, self.hidden_size)
        self.audio_linear = InputProjection(self.audio_emb_dim, self.hidden_size)
        self.audio_utt_transformer = MELDTransEncoder(config, self.audio_utt_Transformernum, self.get_audio_utt_max_lens, self.hidden_size)
        self.vision_linear = InputProjection(self.vision_emb_dim, self.hidden_size)
        self.vision_utt_transformer = MELDTransEncoder(config, self.vision_utt_Transformernum, self.get_vision_utt_max_lens, self.hidden_size)
        self.attention = AdditiveAttention(self.hidden_size, self.hidden_size)
        self.CrossModalTrans_TA = CrossModalTransformerEncoder(self.hidden_size, self.crossmodal_num_heads_TA,
                                                               self.crossmodal_layers_TA, self.crossmodal_attn_dropout_TA)
        self.CrossModalTrans_TA_V = CrossModalTransformerEncoder(self.hidden_size, self.crossmodal_num_heads_TA_V,
                                                                 self.crossmodal_layers_TA_V, self.crossmodal_attn_dropout_TA_V)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.classifier = nn.Linear(self.hidden_size, self.num_labels)
        for m in (self.audio_utt_transformer, self.vision_utt_transformer, self.attention):
            m.compute_dtype = self.compute_dtype

    def _build_plm(self, config):
        """HF from_pretrained as in the reference (:72-77); `config.plm_config` (a transformers config
        object) selects random initialisation instead -- there are no checkpoints on the benchmark box."""
        injected = getattr(config, "plm_module", None)
        if injected is not None:                       # test fixtures inject a deterministic stand-in encoder
            return injected
        from transformers import BertModel, RobertaModel
        cls = RobertaModel if self.text_pretrained_model == 'roberta' else BertModel
        plm_config = getattr(config, "plm_config", None)
        if plm_config is not None:
            plm = cls(plm_config, add_pooling_layer=False) if getattr(config, "plm_no_pooler", False) else cls(plm_config)
        else:
            plm = cls.from_pretrained(config.pretrainedtextmodel_path)
        # forward() reads last_hidden_state only (ref :101-107): the pooler never receives a gradient.  It stays in the
        # module (state_dict keys of the reference's checkpoints) but is frozen, so that a data-parallel gradient
        # exchange never waits for a gradient that cannot arrive (parallel.GradientAverager raises on that, as DDP does);
        # the optimizer skips gradient-less parameters either way, so training is unchanged.
        if getattr(plm, "pooler", None) is not None:
            for p in plm.pooler.parameters():
                p.requires_grad_(False)
        return plm

    # ---- the forward in two branches (the text branch does not depend on the visual path) ------------------
    def text_branch(self, batch_text_input_ids, batch_text_input_mask, batch_text_sep_mask, batchUtt_in_dia_idx):
        """PLM -> text_linear -> tokens of the target utterance (ref :95-150): (B, L_t, H), mask (B, L_t)"""
        plm = self.roberta if self.text_pretrained_model == 'roberta' else self.bert
        # `text_token_capacity` (set by the training steps, train_step PACK_NOTE; absent or 0: the padded layout): the fused encoder's layers and
        # text_linear run on the real tokens packed into that many rows; the rows go back to (B, T, H) in front of the slicing, zeros at the padding
        box = getattr(plm, "_fmmt_box", None)
        if box is not None:
            box.capacity = int(getattr(self, "text_token_capacity", 0) or 0)
        try:
            text_out = self._plm_forward(plm, batch_text_input_ids, batch_text_input_mask)
        finally:
            lay = box.take_layout() if box is not None else None
            if box is not None:
                box.capacity = 0
        text_utt_linear = self.text_linear(text_out.to(self.text_linear.weight.dtype))
        if lay is not None:
            from . import ops
            text_utt_linear = ops.unpack_rows(text_utt_linear[0], lay)
        return slice_target_utterance(text_utt_linear, batch_text_sep_mask, batchUtt_in_dia_idx,
                                      self.get_text_utt_max_lens, self.text_pretrained_model == 'roberta')

    @staticmethod
    def _plm_forward(plm, batch_text_input_ids, batch_text_input_mask):
        if next(plm.parameters()).dtype in (torch.bfloat16, torch.float16) and batch_text_input_ids.is_cuda:
            # a text encoder whose parameters already are low precision (train_step.MasterWeights) runs as it is: autocast
            # would still force its LayerNorms / softmax through fp32 tensors and casts
            with torch.autocast("cuda", enabled=False):
                return plm(batch_text_input_ids, batch_text_input_mask)[0]
        return plm(batch_text_input_ids, batch_text_input_mask)[0]                       # (B, T, plm_hidden); packed: (1, capacity, plm_hidden)

    def _pair(self, fa, fb, reads=()):
        """Run two independent sub-computations; with `self.pair_stream` set (by train_step.graph_multimodal) the first one
        runs on that stream, forked from and joined to the current one.  Inside a HIP-graph capture this records two
        parallel branches (and, because autograd replays a node on its forward stream, two in the backward graph as well):
        the fusion stack's launches are 50-250 workgroups each, so two of them side by side still leave the GPU room.
        `reads`: the main-stream tensors fa consumes.  The caching allocator tracks a block by the stream it was allocated
        on; both directions of the hand-over are therefore declared with record_stream (inputs read on the side stream,
        results consumed on the main stream), so a block freed on the host is not handed out again on its home stream
        while the other stream may still be reading it."""
        side = getattr(self, "pair_stream", None)
        if side is None:
            return fa(), fb()
        cur = torch.cuda.current_stream()
        side.wait_stream(cur)                                  # fork: everything fa reads is complete
        for t in reads:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(side)
        with torch.cuda.stream(side):
            ra = fa()
        rb = fb()
        cur.wait_stream(side)                                  # join before anything consumes ra
        for t in (ra if isinstance(ra, (tuple, list)) else (ra,)):
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cur)
        return ra, rb

    def fusion_branch(self, text_feat, text_mask, audio_inputs, audio_mask, vision_inputs, new_vision_mask):
        """self-attention encoders, four cross-modal calls, pooling, classifier (ref :152-188)"""
        cd = self.compute_dtype
        out_dtype = text_feat.dtype
        from . import ops
        # one device draw for every dropout seed of the stack (attention and hidden dropout: ~40 call sites) instead of one launch each
        with ops.seed_scope(text_feat.device, 96, enabled=self.training and text_feat.is_cuda):
            return self._fusion_body(text_feat, text_mask, audio_inputs, audio_mask, vision_inputs, new_vision_mask, cd, out_dtype)

    def _fusion_body(self, text_feat, text_mask, audio_inputs, audio_mask, vision_inputs, new_vision_mask, cd, out_dtype):
        def audio_side():
            audio_ext = (1.0 - audio_mask.unsqueeze(1).unsqueeze(2)) * -10000.0
            audio_utt = self.audio_utt_transformer(self.audio_linear(audio_inputs), audio_ext)
            return audio_utt.transpose(0, 1).contiguous().to(cd)

        def vision_side():
            vision_ext = (1.0 - new_vision_mask.unsqueeze(1).unsqueeze(2)) * -10000.0
            vision_utt = self.vision_utt_transformer(self.vision_linear(vision_inputs), vision_ext)
            return vision_utt.transpose(0, 1).contiguous().to(cd), text_feat.transpose(0, 1).contiguous().to(cd)

        # cross-modal fusion on the HIP path, time-major, in the module's compute dtype
        a_tm, (v_tm, t_tm) = self._pair(audio_side, vision_side, reads=(audio_inputs, audio_mask))
        if self.stack_directions and self.CrossModalTrans_TA.pair_fusable() and self.CrossModalTrans_TA_V.pair_fusable():
            # both directions of an encoder as one sweep over the stacked tokens (CrossModalTransformerEncoder.forward_pair): the stacked
            # results ARE the concatenations the reference builds next (ref :173,178)
            ta = self.CrossModalTrans_TA.forward_pair(t_tm, a_tm)                    # [text x audio ; audio x text]
            final = self.CrossModalTrans_TA_V.forward_pair(ta, v_tm)                 # [ta x vision ; vision x ta]
        else:
            text_x_audio, audio_x_text = self._pair(lambda: self.CrossModalTrans_TA(t_tm, a_tm, a_tm),
                                                    lambda: self.CrossModalTrans_TA(a_tm, t_tm, t_tm), reads=(t_tm, a_tm))
            ta = torch.cat((text_x_audio, audio_x_text), dim=0)
            vision_x_ta, ta_x_vision = self._pair(lambda: self.CrossModalTrans_TA_V(v_tm, ta, ta),
                                                  lambda: self.CrossModalTrans_TA_V(ta, v_tm, v_tm), reads=(v_tm, ta))
            final = torch.cat((ta_x_vision, vision_x_ta), dim=0)
        final = final.transpose(0, 1).to(out_dtype)
        final_mask = torch.cat((text_mask.to(audio_mask.dtype), audio_mask, new_vision_mask), dim=1)

        pooled, _ = self.attention(final, final_mask)
        return self.classifier(self.dropout(pooled))

    def _branch_call(self, name, eager):
        """The HIP-graph replay of a branch (installed by train_step.graph_multimodal) or the eager branch.  The graphs
        were captured in TRAINING mode with the training batch's static shapes (dropout active), and the graphed
        callables are not child modules, so `mm.eval()` cannot reach them: outside training mode -- validation / test
        after an epoch, as the reference's multimodal_evaluate does -- the eager branch runs instead."""
        g = getattr(self, name, None)
        return g if (g is not None and self.training) else eager

    def launch_text(self, batch_text_input_ids, batch_text_input_mask, batch_text_sep_mask, batchUtt_in_dia_idx):
        """Optional: issue the text branch NOW on `self.text_stream` (a second HIP stream) and let the next forward() pick
        the result up.  A training step calls this before it enqueues the Swin forward: the text encoder's many small
        launches then run concurrently with Swin's large ones, and -- because autograd replays a node on the stream of
        its forward, and processes later-created nodes first -- its backward is issued right after Swin's backward has
        been enqueued and overlaps with it as well.  Without a text stream this is a no-op."""
        side = getattr(self, "text_stream", None)
        if side is None or not batch_text_input_ids.is_cuda:
            return
        text_call = self._branch_call("_text_call", self.text_branch)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._pending_text = text_call(batch_text_input_ids, batch_text_input_mask, batch_text_sep_mask,
                                           torch.as_tensor(batchUtt_in_dia_idx, device=batch_text_input_ids.device))

    def forward(self, batch_text_input_ids=None, batch_text_input_mask=None, batch_text_sep_mask=None,
                audio_inputs=None, audio_mask=None, vision_inputs=None, new_vision_mask=None, batchUtt_in_dia_idx=None):
        """Same signature and result as the reference's forward.  `_text_call` / `_fusion_call` are the two branches
        (replaced by their HIP-graph replays by train_step.graph_multimodal); a text branch already in flight on the
        second stream (launch_text) is joined here."""
        fusion_call = self._branch_call("_fusion_call", self.fusion_branch)
        pending = getattr(self, "_pending_text", None)
        if pending is not None:
            self._pending_text = None
            text_feat, text_mask = pending
            main = torch.cuda.current_stream()
            main.wait_stream(self.text_stream)
            text_feat.record_stream(main)                      # produced on the text stream, consumed here
            text_mask.record_stream(main)
        else:
            text_call = self._branch_call("_text_call", self.text_branch)
            text_feat, text_mask = text_call(batch_text_input_ids, batch_text_input_mask, batch_text_sep_mask,
                                             torch.as_tensor(batchUtt_in_dia_idx, device=batch_text_input_ids.device))
        return fusion_call(text_feat, text_mask, audio_inputs, audio_mask, vision_inputs, new_vision_mask)


class meld_utt_transformer(nn.Module):
    """Unimodal (V-only) classifier on pre-extracted features (ref src/models.py:192-223)."""

    def __init__(self, args):
        super().__init__()
        self.modality_origin_emb = args.vision_featExtr_dim
        self.modality_utt_Transformernum = args.vision_utt_Transformernum
        self.get_utt_max_lens = args.get_vision_utt_max_lens
        self.hidden_size = args.hidden_size
        self.hidden_dropout_prob = args.hidden_dropout_prob
        self.modality_linear = nn.Linear(self.modality_origin_emb, self.hidden_size)
        self.utt_transformer = MELDTransEncoder(args, self.modality_utt_Transformernum, self.get_utt_max_lens, self.hidden_size)
        self.attention = AdditiveAttention(self.hidden_size, self.hidden_size)
        self.mm_dropout = nn.Dropout(self.hidden_dropout_prob)
        self.classifier = nn.Linear(self.hidden_size, args.num_labels)
        self.utt_transformer.compute_dtype = self.attention.compute_dtype = getattr(args, "compute_dtype", None)

    def forward(self, inputs=None, utt_mask=None):
        ext = utt_mask.unsqueeze(1).unsqueeze(2).to(dtype=next(self.parameters()).dtype)
        ext = (1.0 - ext) * -10000.0
        h = self.utt_transformer(self.modality_linear(inputs), ext)
        pooled, _ = self.attention(h, utt_mask)
        return self.classifier(self.mm_dropout(pooled))

    def forward_loss(self, inputs=None, utt_mask=None, labels=None, valid_mean=False, criterion=None):
        """(loss, logits) of a training / validation batch (train.py:256-258, :283-285: the model, then cross_entropy): the encoder as `forward` runs it,
        the pooling's two Linear layers (P over the tokens, Q over the query vector) on ops.linear, and everything behind them -- tanh, scores, masked
        softmax, weighted sum, dropout, classifier, cross-entropy -- as ops.pool_head_loss (two launches per direction).  eval(): no dropout.  The
        reference's pooling returns the squeezed input for a one-token sequence (modules/Transformer.py:26-27); a loss has no use for that: L == 1 raises.
        valid_mean: the loss is the mean over the rows whose label lies in [0, num_labels) -- a short batch padded with label -100 rows
        (train_step.pad_unimodal_batch) then gives the compact batch's loss and gradients; every label valid: the same bits as without it.
        criterion (None: the plain cross-entropy; else a train_step.Criterion): the class-weighted, label-smoothed mean over the labelled rows."""
        from . import ops
        if inputs.shape[1] == 1:
            raise ValueError("meld_utt_transformer.forward_loss: a sequence of one token has no attention pooling to train")
        ext = utt_mask.unsqueeze(1).unsqueeze(2).to(dtype=next(self.parameters()).dtype)
        ext = (1.0 - ext) * -10000.0
        h = self.utt_transformer(self.modality_linear(inputs), ext)
        att = self.attention
        cd = att.compute_dtype or h.dtype
        hc = h.to(cd)
        ph = ops.linear(hc, att.P.weight, att.P.bias)
        qq = ops.linear(att.query_vector.to(cd).unsqueeze(0), att.Q.weight, att.Q.bias).float().reshape(-1)
        p = self.mm_dropout.p if self.training else 0.0
        seed = ops.draw_seed(h.device) if p > 0 else 0
        return ops.pool_head_loss(hc, ph, qq, att.value.weight, att.value.bias, utt_mask, self.classifier.weight, self.classifier.bias, labels, p, seed, valid_mean, criterion)
