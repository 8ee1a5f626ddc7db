/* libfmmt_hip -- the pooling head's entry points; included by fmmt.h (same ABI rules: plain C, caller-owned buffers, asynchronous on `stream`,
 * 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_POOL_HEAD_H
#define FMMT_POOL_HEAD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Additive-attention pooling -> dropout -> classifier -> cross-entropy: the tail of the V-only classifier (and, by its shapes, of the multimodal one) behind
 * the pooling's one GEMM, as two launches per direction.  Replaces modules/Transformer.py:24-45 (AdditiveAttention.forward behind `self.P(inputs)`:
 * tanh, the 1-column `value` Linear, masked_fill, softmax, bmm), src/models.py:183-188 / :219-221 (Dropout, classifier) and the cross_entropy of
 * train.py:258 with their backwards.  The caller keeps ph = P h + b_P (B L x H x H) and the one-row qq = Q query_vector + b_Q on fmmt_linear_fwd.
 *   h, ph [B][L][H] in `dtype`; qq, value_w [H], value_b [1], mask [B][L] (0 = masked), cls_w [NL][H], cls_b [NL] fp32; labels [B] int64 in [0, NL)
 *   (a label outside adds nothing to the loss and gets no gradient); dropout probability p in [0, 1), its seed an integer or, when seed_dev is
 *   non-NULL, a device word read at run time (a replayed graph then draws fresh masks) -- the element generator of the fused sublayer tails.
 *   score_t = value_w . tanh(ph_t + qq) + value_b, -inf where mask == 0; alpha = softmax_t (fp32, log2 domain); pooled = sum_t alpha_t h_t;
 *   logits = cls_w (keep * pooled) + cls_b; loss = mean over the B rows of logsumexp(logits) - logits[label], summed in a fixed order.
 *   Outputs, all fp32: logits [B][NL], loss [1], and what the backward reads: alpha [B][L], pooled [B][H] (before dropout), keep [B][H] (0 or
 *   1 / (1 - p) as realised).  tanh is recomputed.  A row whose mask is all zero yields NaN, as the reference's softmax over -inf does.
 * fmmt_pool_head_bwd: dloss [1] fp32 (device) ->  dh [B][L][H] = alpha_t d(pooled) (the pooling's share of h's gradient: the caller adds what flows
 *   through ph), dph [B][L][H] = d(score_t) value_w (1 - tanh^2), both in `dtype`; dqq [H] = sum of dph over rows and tokens, dv [H], dvb [1],
 *   dW [NL][H], db [NL] fp32.  Every reduction over B and L runs in a fixed order without atomics: two runs give the same bits.
 * workspace: fmmt_pool_head_bwd_workspace(B, L, H) bytes serve EITHER direction (flash-style per-workgroup partials: a row's tokens are split over
 *   up to 32 workgroups; 0 for shapes outside the limits).  2 <= L <= 1024, H % 8 == 0, H <= 1024, NL <= 8, B <= 1024, else FMMT_EINVAL;
 *   h, ph, dh, dph, qq, value_w and the workspace 16-byte aligned, else FMMT_EALIGN.  FMMT_BF16: bf16 h / ph / dh / dph, all arithmetic fp32;
 *   FMMT_F32: the same template, nothing rounded. */
size_t fmmt_pool_head_bwd_workspace(int B, int L, int H);
int fmmt_pool_head_fwd(int dtype, int B, int L, int H, int NL, const void* h, const void* ph, const float* qq, const float* value_w,
                       const float* value_b, const float* mask, const float* cls_w, const float* cls_b, const int64_t* labels, float p, uint64_t seed,
                       const uint64_t* seed_dev, float* logits, float* loss, float* alpha, float* pooled, float* keep, void* workspace,
                       size_t workspace_bytes, void* stream);
int fmmt_pool_head_bwd(int dtype, int B, int L, int H, int NL, const float* dloss, const void* h, const void* ph, const float* qq,
                       const float* value_w, const float* cls_w, const int64_t* labels, const float* logits, const float* alpha, const float* pooled,
                       const float* keep, void* dh, void* dph, float* dqq, float* dv, float* dvb, float* dW, float* db, void* workspace,
                       size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
