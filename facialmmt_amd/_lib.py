"""ctypes binding of libfmmt_hip.so (the C ABI declared in include/fmmt.h).

This is exactly the binding a maintainer of the reference would add: device
pointers come from ``tensor.data_ptr()``, the stream from ``torch.cuda.current_stream().cuda_stream``.
There is no fallback: a missing library or a non-zero return code raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfmmt_hip.so")

F32, BF16 = 0, 1
GENERIC = 0x100          # dtype flag of the fused Mlp entry points: the element-type-generic restatement (include/fmmt.h)
EPI_NONE, EPI_GELU, EPI_GELU_BWD, EPI_GELU_DG, EPI_MUL_AUX = 0, 1, 2, 3, 4
SAVE_DG = 0x200
BATCH_MAJOR = 0x400          # include/fmmt.h FMMT_BATCH_MAJOR: fmmt_mha_fwd / _bwd on (batch, tokens, hidden) operands
# include/fmmt.h FMMT_SAVE_DG: dtype flag of the fused Mlp entry points (h_pre = gelu'(pre-activation))
RESIZE_PIL, RESIZE_CV2 = 0, 1

_p, _i, _f, _sz, _u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_uint64

# name -> (restype, argtypes); mirrors include/fmmt.h one to one (tests/test_host_cpu.py::test_header_and_ctypes_signatures_agree checks both ways)
SIGNATURES = {
    "fmmt_version": (_i, []),
    "fmmt_linear_fwd": (_i, [_i, _i, _i, _i, _p, _i, _p, _i, _p, _p, _i, _p, _i, _p, _i, _p, _i, _p, _i, _p]),
    "fmmt_linear_splitk_workspace": (_sz, [_i, _i, _i]),
    "fmmt_linear_fwd_splitk": (_i, [_i, _i, _i, _i, _p, _i, _p, _i, _p, _p, _i, _p, _sz, _p]),
    "fmmt_linear_wgrad_workspace": (_sz, [_i, _i, _i, _i]),
    "fmmt_linear_wgrad": (_i, [_i, _i, _i, _i, _p, _i, _p, _i, _p, _p, _p, _i, _i, _p, _sz, _p]),
    "fmmt_linear_wgrad_partials": (_i, [_i, _i, _i, _i, _p, _i, _p, _i, _i, _p, _i, _i, _p, _sz, _p]),
    "fmmt_mlp_fwd": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "fmmt_mlp_ln_fwd": (_i, [_i, _i, _i, _p, _p, _p, _f, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p]),
    "fmmt_mlp_bwd_input": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p]),
    "fmmt_linear_ln_bwd_workspace": (_sz, [_i]),
    "fmmt_linear_ln_bwd": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "fmmt_mlp_ln_bwd_input_workspace": (_sz, [_i]),
    "fmmt_mlp_ln_bwd_input": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "fmmt_linear_wgrad_finish": (_i, [_i, _i, _i, _i, _p, _p, _p, _sz, _p]),
    "fmmt_layernorm_fwd": (_i, [_i, _i, _i, _p, _p, _p, _f, _p, _p, _p, _i, _p]),
    "fmmt_layernorm_bwd_workspace": (_sz, [_i]),
    "fmmt_layernorm_bwd": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _sz, _p]),
    "fmmt_window_attn_fwd": (_i, [_i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _i, _f, _p, _p, _p]),
    "fmmt_window_attn_bwd_workspace": (_sz, [_i]),
    "fmmt_window_attn_bwd": (_i, [_i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _f, _p, _p, _p, _sz, _p]),
    "fmmt_window_block_fwd": (_i, [_i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fmmt_window_block_fwd_ref": (_i, [_i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fmmt_window_block_attn_bwd": (_i, [_i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _sz, _p]),
    "fmmt_window_block_attn_bwd_ref": (_i, [_i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _sz, _p]),
    "fmmt_linear_fwd_seg3": (_i, [_i, _i, _i, _i, _p, _i, _p, _p, _p, _i, _i, _p, _p, _p, _p, _i, _p]),
    "fmmt_select_frames_fwd": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _f, _p, _p, _p, _p]),
    "fmmt_select_frames_bwd": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "fmmt_mha_fwd": (_i, [_i, _i, _i, _i, _i, _i, _p, _i, _p, _p, _i, _f, _p, _f, _u64, _p, _p, _i, _p, _p]),
    "fmmt_mha_bwd": (_i, [_i, _i, _i, _i, _i, _i, _p, _i, _p, _p, _i, _f, _p, _f, _u64, _p, _p, _p, _i, _p, _p, _i, _p, _p, _i, _p]),
    "fmmt_mha_avg_weights": (_i, [_i, _i, _i, _i, _i, _i, _p, _i, _p, _i, _f, _p, _f, _u64, _p, _p, _p, _p]),
    "fmmt_patch_im2col": (_i, [_i, _i, _p, _p, _p]),
    "fmmt_patch_col2im": (_i, [_i, _i, _p, _p, _p]),
    "fmmt_batchnorm1d_fwd": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _f, _f, _i, _p, _p, _p, _p]),
    "fmmt_batchnorm1d_bwd": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "fmmt_posemb_scale_fwd": (_i, [_i, _i, _i, _i, _p, _p, _f, _p, _p]),
    "fmmt_scale": (_i, [_i, _sz, _p, _f, _p, _p]),
    "fmmt_colsum": (_i, [_i, _i, _i, _i, _p, _i, _p, _p]),
    "fmmt_cast_batch": (_i, [_i, _i, _p, _p]),
    "fmmt_layernorm_bwd_bf16_workspace": (_sz, [_i, _i]),
    "fmmt_layernorm_bwd_bf16": (_i, [_i, _i, _f, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "fmmt_dropadd_ln_fwd": (_i, [_i, _i, _i, _f, _p, _p, _p, _p, _f, _u64, _p, _u64, _p, _p, _p]),
    "fmmt_dropadd_ln_bwd_workspace": (_sz, [_i, _i]),
    "fmmt_dropadd_ln_bwd": (_i, [_i, _i, _i, _f, _p, _p, _p, _f, _u64, _p, _u64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "fmmt_plm_dropadd_ln_fwd": (_i, [_i, _i, _f, _p, _p, _p, _p, _f, _u64, _p, _u64, _p, _p, _p]),
    "fmmt_embedding_bwd": (_i, [_i, _i, _i, _p, C.c_int64, _p, _p, _p]),
    "fmmt_plm_gelu_bwd_colsum_workspace": (_sz, [_i, _i]),
    "fmmt_plm_gelu_bwd_colsum": (_i, [_i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "fmmt_plm_dropadd_ln_bwd_workspace": (_sz, [_i, _i]),
    "fmmt_plm_dropadd_ln_bwd": (_i, [_i, _i, _f, _p, _p, _p, _f, _u64, _p, _u64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "fmmt_grad_handover": (_i, [_i, _i, _p, _p, _p, _p]),
    "fmmt_adamw_batch": (_i, [_i, _i, _p, _p, _p, _p, _f, _f, _f, _f, _f, _i, _p]),
    "fmmt_resize_table": (_i, [_i, _i, _i, _p, _p]),
    "fmmt_resize_band_rows": (_i, [_p, _i]),
    "fmmt_patch_embed_u8": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "fmmt_patch_embed_ln_fwd": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p]),
    "fmmt_patch_embed_u8_ln_fwd": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p]),
    "fmmt_emotion_head_fwd": (_i, [_i, _i, _i, _i, _i, _p, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p]),
    "fmmt_eval_accumulate": (_i, [_i, _i, _i, _p, _i, _p, _p, _p, _p, _p, _p, C.c_int64, C.c_int64, _p]),
}

# include/fmmt_pool_head.h, one to one.  Why a second table and a second header (which fmmt.h includes) instead of three more rows above:
# tests/test_eval_cpu.py pins len(SIGNATURES) == 59 and tests/test_host_cpu.py holds fmmt.h's own prototypes equal to SIGNATURES; both files stay as
# they are, so the pooling head's entry points are declared beside them.  tests/test_unimodal_oracle_cpu.py::test_pool_head_header_signatures_and_library_agree
# holds this table, that header (names and the type of every argument) and the built library together.
POOL_HEAD_SIGNATURES = {
    "fmmt_pool_head_bwd_workspace": (_sz, [_i, _i, _i]),
    "fmmt_pool_head_fwd": (_i, [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f, _u64, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "fmmt_pool_head_bwd": (_i, [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
}

# include/fmmt_ragged.h, one to one: a third table and header for the reason written above POOL_HEAD_SIGNATURES
# (tests/test_ragged_cpu.py::test_ragged_header_signatures_and_library_agree holds table, header and library together)
RAGGED_SIGNATURES = {
    "fmmt_pack_frames": (_i, [_i, _i, _i, _sz, _p, _p, _p, _p, _p]),
    "fmmt_batchnorm1d_fwd_n": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _f, _f, _i, _p, _p, _p, _p]),
    "fmmt_batchnorm1d_bwd_n": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "fmmt_select_frames_fwd_n": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p]),
}

# include/fmmt_eval_collect.h, one to one: a fourth table and header for the same reason
# (tests/test_eval_collect_cpu.py::test_eval_collect_header_signatures_and_library_agree holds table, header and library together)
EVAL_COLLECT_SIGNATURES = {
    "fmmt_eval_accumulate_at": (_i, [_i, _i, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, C.c_int64, _p]),
}

# include/fmmt_pool_head_rows.h, one to one: a fifth table and header for the same reason -- the pooling head's pair with the row count added behind
# `keep` (tests/test_pad_rows_cpu.py::test_pool_head_rows_header_signatures_and_library_agree holds table, header and library together)
POOL_HEAD_ROWS_SIGNATURES = {
    "fmmt_pool_head_fwd_rows": (_i, [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f, _u64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "fmmt_pool_head_bwd_rows": (_i, [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
}

# include/fmmt_guard.h, one to one: a sixth table and header for the same reason -- the update that is skipped on a non-finite gradient norm and
# the counters beside it (tests/test_guard_cpu.py::test_guard_header_signatures_and_library_agree holds table, header and library together)
GUARD_SIGNATURES = {
    "fmmt_adamw_batch_guarded": (_i, [_i, _i, _p, _p, _p, _p, _f, _f, _f, _f, _f, _i, _p]),
    "fmmt_guard_commit": (_i, [_p, _p, _p, _p]),
    "fmmt_monitor_loss": (_i, [_p, _f, _p, _p]),
}
# the layout of `words` (include/fmmt_guard.h FMMT_GUARD_*): the one place Python states it; train_step.TrainMonitor reads through these
GUARD_LOSS_SUM, GUARD_MICRO_STEPS, GUARD_NONFINITE_LOSSES, GUARD_APPLIED, GUARD_SKIPPED, GUARD_LAST_NORM, GUARD_WORDS = 0, 1, 2, 3, 4, 5, 6

# include/fmmt_digest.h, one to one: a seventh table and header for the same reason -- the replica digest over fmmt_adamw_batch's descriptor
# table (tests/test_digest_cpu.py::test_digest_header_signatures_and_library_agree holds table, header and library together)
DIGEST_SIGNATURES = {
    "fmmt_param_digest": (_i, [_i, _i, _p, _p, _p, _p]),
}
DIGEST_WORDS = 6          # (S1, S2) of the parameters, the first moments, the second moments

# include/fmmt_eval_shard.h, one to one: an eighth table and header for the same reason -- the collecting metric update with a device-held row count
# and the merge of the ranks' shards (tests/test_eval_shard_cpu.py::test_eval_shard_header_signatures_and_library_agree holds table, header and library together)
EVAL_SHARD_SIGNATURES = {
    "fmmt_eval_accumulate_rows": (_i, [_i, _i, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, C.c_int64, _p]),
    "fmmt_eval_merge": (_i, [_i, _i, C.c_int64, C.c_int64, _p, _p, _p, _p, _p, _p, _p]),
}

# include/fmmt_jitter.h, one to one: a ninth table and header for the same reason -- the uint8 pre-step pair with the per-frame ColorJitter table and
# the contrast statistic's scratch behind `lut_dev` (tests/test_color_jitter_cpu.py::test_jitter_header_signatures_and_library_agree holds table, header and library together)
JITTER_SIGNATURES = {
    "fmmt_jitter_table_check": (_i, [_p, _i]),
    "fmmt_patch_embed_u8_jitter": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "fmmt_patch_embed_u8_jitter_ln_fwd": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p]),
}
# the record layout (include/fmmt_jitter.h FMMT_JITTER_*): the one place Python states it; augment.ColorJitter builds tables through these
JITTER_WORDS, JITTER_BANDS = 8, 56
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE, JITTER_NONE = 0, 1, 2, 3, 4

# include/fmmt_aug.h, one to one: a tenth table and header -- the uint8 pre-step pair with the Aff-Wild2 chain's per-frame record, the byte workspace
# of the frame behind `partial` and the host check of a record (tests/test_aff_augment_cpu.py holds table, header and library together)
AUG_SIGNATURES = {
    "fmmt_aug_table_check": (_i, [_p, _i]),
    "fmmt_aug_workspace_bytes": (C.c_size_t, [_i]),
    "fmmt_patch_embed_u8_aug": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p, _p, C.c_size_t, _p, _p]),
    "fmmt_patch_embed_u8_aug_ln_fwd": (_i, [_i, _i, _i, _i, _p, _p, _p, _p, _p, _p, C.c_size_t, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p]),
}
# the record layout (include/fmmt_aug.h FMMT_AUG_*): words 0-7 a jitter record, 8 flags, 9-11 blur r / ww / fw, 12-15 top / left / h / w, 16-17 noise key
AUG_WORDS, AUG_FLAG_GRAY, AUG_MAX_RADIUS, AUG_HALO = 20, 1, 1, 6

# include/fmmt_groups.h, one to one: an eleventh table and header -- fmmt_adamw_batch and its guarded twin with the learning rate, betas, eps and
# weight decay read per record from a group table (tests/test_param_groups_cpu.py holds table, header and library together)
GROUPS_SIGNATURES = {
    "fmmt_adamw_groups": (_i, [_i, _i, _p, _i, _p, _p, _p, _p, _f, _i, _p]),
    "fmmt_adamw_groups_guarded": (_i, [_i, _i, _p, _i, _p, _p, _p, _p, _f, _i, _p]),
}
# the group record (include/fmmt_groups.h fmmt_adamw_group): the one place Python states it; train_step.FusedClipAdamW builds tables through this
ADAMW_GROUP_BYTES = 32
ADAMW_GROUP_FIELDS = [("lr", "<u8"), ("beta1", "<f4"), ("beta2", "<f4"), ("eps", "<f4"), ("weight_decay", "<f4"), ("pad", "<u4", (2,))]

# include/fmmt_stats.h, one to one: a twelfth table and header -- per-record statistics of one field of fmmt_adamw_batch's descriptor table and the
# snapshot of a bad update (tests/test_grad_report_cpu.py holds table, header and library together)
STATS_SIGNATURES = {
    "fmmt_table_stats": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
}
# the field selector and the 16-byte record (include/fmmt_stats.h FMMT_STATS_*): the one place Python states them; train_step.GradReport reads through these
STATS_G, STATS_P, STATS_M, STATS_V = 0, 1, 2, 3
STATS_BYTES, STATS_BAD_WORDS = 16, 2
STATS_FIELDS = [("sumsq", "<f4"), ("max_abs", "<f4"), ("nonfinite", "<i4"), ("reserved", "<i4")]

# include/fmmt_tokens.h, one to one: a thirteenth table and header -- the text encoder on real tokens only: the token layout of a padding mask, the
# unpack of packed rows, the attention core's ragged mode, the sublayer tails with a row map (tests/test_tokens_cpu.py holds table, header and library together)
TOKENS_SIGNATURES = {
    "fmmt_token_layout": (_i, [_i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "fmmt_unpack_rows": (_i, [_i, _i, _i, _sz, _p, _p, _p, _p]),
    "fmmt_mha_fwd_ragged": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _i, _f, _f, _u64, _p, _p, _i, _p, _p]),
    "fmmt_mha_bwd_ragged": (_i, [_i, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _i, _f, _f, _u64, _p, _p, _p, _i, _p, _p, _i, _p, _p, _i, _p]),
    "fmmt_dropadd_ln_fwd_map": (_i, [_i, _i, _i, _f, _p, _p, _p, _p, _f, _u64, _p, _u64, _p, _p, _p, _p]),
    "fmmt_dropadd_ln_bwd_map": (_i, [_i, _i, _i, _f, _p, _p, _p, _f, _u64, _p, _u64, _p, _p, _p, _p, _p, _p, _sz, _p, _p]),
}
# include/fmmt_loss.h, one to one: a fourteenth table and header -- the class-weighted, label-smoothed cross-entropy of (B, NL) logits, one launch per
# direction, and the pooling head's _rows pair with that loss (a float `den` word for the int row count) (tests/test_criterion_cpu.py holds table, header and library together)
LOSS_SIGNATURES = {
    "fmmt_ce_fwd": (_i, [_i, _i, _i, _p, _i, _p, _p, _f, _p, _p, _p]),
    "fmmt_ce_bwd": (_i, [_i, _i, _i, _p, _i, _p, _p, _f, _p, _p, _p, _i, _p]),
    "fmmt_pool_head_fwd_crit": (_i, [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f, _u64, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _sz, _p]),
    "fmmt_pool_head_bwd_crit": (_i, [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
}
# include/fmmt_route.h, one to one: a fifteenth table and header -- which kernel family a GEMM launch takes, answered on the host by the dispatch itself
# (tests/test_gemm_routes_cpu.py holds table, header, the ROUTE_* values below and the library together)
ROUTE_SIGNATURES = {
    "fmmt_linear_fwd_route": (_i, [_i] * 17),
    "fmmt_linear_wgrad_route": (_i, [_i] * 10),
}
ROUTE_MODE_FWD, ROUTE_MODE_SEG3_N, ROUTE_MODE_SEG3_K, ROUTE_MODE_SPLITK = 0, 1, 2, 3
CE_MAXNL, CE_MAXB = 8, 65536          # include/fmmt_loss.h: the limits of fmmt_ce_fwd / _bwd
RAGGED = 0x800          # include/fmmt_tokens.h FMMT_RAGGED: the dtype flag fmmt_mha_fwd_ragged / _bwd_ragged ask for

FMMT_EINVAL, FMMT_EALIGN, FMMT_EWORKSPACE = -1, -2, -3
_ERR = {-1: "FMMT_EINVAL (bad shape / unsupported size)", -2: "FMMT_EALIGN (pointer or leading dimension not 16-byte aligned)",
        -3: "FMMT_EWORKSPACE (workspace too small)"}

_lib = None


class FmmtError(RuntimeError):
    pass


def load():
    """Load the shared library (once).  Raises FmmtError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FmmtError(f"{LIB_PATH} is missing: build it with `python -m facialmmt_amd.build` "
                        f"(or __graft_entry__.build()); there is no CPU / PyTorch fallback for the hot path")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(POOL_HEAD_SIGNATURES.items()) + list(RAGGED_SIGNATURES.items()) + list(EVAL_COLLECT_SIGNATURES.items()) + list(POOL_HEAD_ROWS_SIGNATURES.items()) + list(GUARD_SIGNATURES.items()) + list(DIGEST_SIGNATURES.items()) + list(EVAL_SHARD_SIGNATURES.items()) + list(JITTER_SIGNATURES.items()) + list(AUG_SIGNATURES.items()) + list(GROUPS_SIGNATURES.items()) + list(STATS_SIGNATURES.items()) + list(TOKENS_SIGNATURES.items()) + list(LOSS_SIGNATURES.items()) + list(ROUTE_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = _ERR.get(rc, f"hipError_t {rc}")
        raise FmmtError(f"{what} failed: {msg}")


def dtype_code(t) -> int:
    import torch
    if t == torch.float32:
        return F32
    if t == torch.bfloat16:
        return BF16
    raise FmmtError(f"unsupported activation dtype {t}: the HIP path computes in float32 (parity) or bfloat16 (throughput)")
