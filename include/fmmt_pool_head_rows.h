/* libfmmt_hip -- the pooling head's loss as a mean over the rows that have a label; included by fmmt.h (same ABI rules: plain C, caller-owned
 * buffers, asynchronous on `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_POOL_HEAD_ROWS_H
#define FMMT_POOL_HEAD_ROWS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A captured training graph has one batch shape, and an epoch ends on a batch with fewer rows.  Such a batch is padded to the captured shape with
 * rows whose label is -100; the loss then has to be what the reference computes on the compact batch (train.py:256-258 on a short batch: the model,
 * then F.cross_entropy, whose mean runs over the rows it was given) -- a mean over the LABELLED rows, not over B as fmmt_pool_head_fwd takes it.
 *
 * fmmt_pool_head_fwd_rows: fmmt_pool_head_fwd (fmmt_pool_head.h: every argument, limit, alignment rule and return code, the same workspace of
 *   fmmt_pool_head_bwd_workspace(B, L, H) bytes) plus n_rows [1] int32, a DEVICE output: the number of rows b with 0 <= labels[b] < NL, counted by the
 *   finishing launch and written with an ordinary store.  loss = (sum over the rows, in the same fixed order, of logsumexp(logits) - logits[label])
 *   / n_rows; a row without a label adds an exact 0 to the sum; n_rows == 0: loss = 0.  Stands for train.py:256-258 on a short batch (cross_entropy
 *   with its default ignore_index = -100 over the padded rows).  logits, alpha, pooled and keep are written for EVERY row, labelled or not.
 * fmmt_pool_head_bwd_rows: fmmt_pool_head_bwd plus n_rows, the word the forward wrote, READ ON THE DEVICE -- never on the host, so a replayed graph
 *   follows the batch it is given.  d(logits)_b = dloss / n_rows (softmax - onehot) for a labelled row (the backward of train.py:258 / :262 on a short
 *   batch); a row without a label gets exact zeros in d(logits), dh and dph and adds exact zeros to dqq, dv, dvb, dW and db (its h, ph, alpha and
 *   pooled must be finite: zero times them is the zero written).  n_rows == 0: every gradient is zero.
 * One kernel body serves both families (the divisor is B or the device word, as bn1d_core.h serves the masked and the unmasked BatchNorm): when every
 * label is valid n_rows == B and every output has the bits of fmmt_pool_head_fwd / _bwd.  n_rows == NULL: FMMT_EINVAL. */
int fmmt_pool_head_fwd_rows(int dtype, int B, int L, int H, int NL, const void* h, const void* ph, const float* qq, const float* value_w,
                            const float* value_b, const float* mask, const float* cls_w, const float* cls_b, const int64_t* labels, float p,
                            uint64_t seed, const uint64_t* seed_dev, float* logits, float* loss, float* alpha, float* pooled, float* keep,
                            int32_t* n_rows, void* workspace, size_t workspace_bytes, void* stream);
int fmmt_pool_head_bwd_rows(int dtype, int B, int L, int H, int NL, const float* dloss, const void* h, const void* ph, const float* qq,
                            const float* value_w, const float* cls_w, const int64_t* labels, const float* logits, const float* alpha,
                            const float* pooled, const float* keep, const int32_t* n_rows, void* dh, void* dph, float* dqq, float* dv, float* dvb,
                            float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
