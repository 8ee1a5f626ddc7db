/* libfmmt_hip -- the training loss as a value a run chooses: class-weighted, label-smoothed cross-entropy; included by fmmt.h (same ABI rules:
 * plain C, caller-owned buffers, asynchronous on `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_LOSS_H
#define FMMT_LOSS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reference hands its loops a criterion (train.py:295, taken at train.py:26,135,256); torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps,
 * reduction='mean') is the edit a run on MELD's lopsided labels makes there.  With valid_i = (0 <= labels[i] < NL), p = softmax(x_i), w_c = 1 when
 * class_w == NULL:
 *     t_ic  = valid_i * ((1 - eps) * w[y_i] * [c == y_i] + (eps / NL) * w_c)
 *     num   = - sum_i sum_c t_ic * log p_ic            den = sum_i valid_i * w[y_i]            loss = num / den
 *     dx_ic = dloss * (p_ic * sum_c' t_ic' - t_ic) / den
 * A row of a class whose weight is 0 keeps its smoothing term (torch's rule).  A label outside [0, NL) -- -100, a padded row -- is ignored: it adds
 * nothing to num or den and its gradient row is zero.  DEPARTURE from torch: den == 0 gives loss = 0 and a zero gradient where torch gives NaN, the
 * rule of fmmt_pool_head_fwd_rows for a batch without a labelled row.
 *
 * fmmt_ce_fwd: logits [B][ld] (dtype FMMT_F32 / FMMT_BF16, ld >= NL elements between rows), labels [B] int64, class_w [NL] fp32 (finite, >= 0) or
 *   NULL, smoothing = eps in [0, 1).  Writes loss[0] and den[0], fp32 DEVICE words, with ordinary stores.  ONE launch of one 1024-thread workgroup:
 *   leaf `tid` adds its rows tid, tid + 1024, ... in that order, the 1024 leaves meet in a fixed 10-level tree (the tree of fmmt_eval_accumulate);
 *   no atomics, two calls give the same bits.  All arithmetic fp32.
 * fmmt_ce_bwd: the same operands plus dloss[0] and den[0] (the word the forward wrote), both READ ON THE DEVICE -- never on the host, so both
 *   launches sit inside a captured graph and follow the labels and the weights they are replayed on.  Writes dlogits [B][ld_d] (ld_d >= NL) in the
 *   logits' dtype, columns [0, NL) of every row (zeros for an ignored row); a thread per row, one launch.
 * Limits: 1 <= NL <= 8, 1 <= B <= 65536.  FMMT_EINVAL, before anything is launched: another dtype, B / NL / ld / ld_d outside these, smoothing
 * outside [0, 1) (NaN included), NULL logits / labels / loss / den / dloss / dlogits. */
int fmmt_ce_fwd(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, const float* class_w, float smoothing, float* loss,
                float* den, void* stream);
int fmmt_ce_bwd(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, const float* class_w, float smoothing,
                const float* dloss, const float* den, void* dlogits, int ld_d, void* stream);

/* The pooling head (fmmt_pool_head.h, fmmt_pool_head_rows.h) with that loss behind its classifier: the _rows pair -- every argument, limit,
 * alignment rule, return code and the workspace of fmmt_pool_head_bwd_workspace(B, L, H) bytes -- with three changes: class_w [NL] (NULL-able) and
 * smoothing as above, and den [1], a FLOAT device word (sum of w[label] over the labelled rows) where _rows has the int32 row count.  The same
 * four kernels, instantiated with the row loss and d(logits) of the formulas above; the forward writes den, the backward reads it on the device.
 * class_w == NULL and smoothing == 0: every output and every gradient has the BITS of fmmt_pool_head_fwd_rows / _bwd_rows (the divisor is the same
 * count held as a float, exact for B <= 1024).  den == 0: loss 0, every gradient zero.  den == NULL, smoothing outside [0, 1): FMMT_EINVAL. */
int fmmt_pool_head_fwd_crit(int dtype, int B, int L, int H, int NL, const void* h, const void* ph, const float* qq, const float* value_w,
                            const float* value_b, const float* mask, const float* cls_w, const float* cls_b, const int64_t* labels, float p,
                            uint64_t seed, const uint64_t* seed_dev, float* logits, float* loss, float* alpha, float* pooled, float* keep,
                            const float* class_w, float smoothing, float* den, void* workspace, size_t workspace_bytes, void* stream);
int fmmt_pool_head_bwd_crit(int dtype, int B, int L, int H, int NL, const float* dloss, const void* h, const void* ph, const float* qq,
                            const float* value_w, const float* cls_w, const int64_t* labels, const float* logits, const float* alpha,
                            const float* pooled, const float* keep, const float* class_w, float smoothing, const float* den, void* dh, void* dph,
                            float* dqq, float* dv, float* dvb, float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
