/* libfmmt_hip -- the metric update of an evaluation split that also COLLECTS the split, at a row index held on the device; included by fmmt.h (same
 * ABI rules: plain C, caller-owned buffers, asynchronous on `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_EVAL_COLLECT_H
#define FMMT_EVAL_COLLECT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* multimodal_evaluate keeps every batch's logits and labels and concatenates them at the end of the split (train.py:231-234, :240-241), because
 * eval_meld wants the whole split (utils/eval_metrics.py:16-28).  fmmt_eval_accumulate (fmmt.h) can store a batch's logits at rows
 * [out_offset, out_offset + B), but out_offset is a launch argument: a captured HIP graph freezes it.  This entry point reads the row index from
 * device memory instead, so ONE captured launch, replayed per batch, fills the split's buffers front to back.
 *
 * fmmt_eval_accumulate_at: fmmt_eval_accumulate -- same logits / labels / accumulators, same kernel body, the same bits in *loss_sum (double), *count
 *   and confusion for the same rows -- plus:
 *   cursor [1] int64 on the device: with c = *cursor as the launch finds it, row i < B of the batch is stored at logits_out [c + i][NL] (fp32),
 *     labels_out [c + i] (int64, the label as it came: a negative one too) and, when pred_out is non-NULL, pred_out [c + i] (int32 argmax);
 *   out_capacity: the rows the three buffers hold.  A row with c + i >= out_capacity (or < 0) is stored nowhere; its loss, count and confusion
 *     contributions are accumulated all the same.  A batch may straddle the end: the rows that fit are stored.
 *   Behind the last row the kernel writes *cursor = c + B, also when rows were dropped: *cursor > out_capacity at the end of the split tells the
 *     caller that it overflowed (as counts[1] > F_cap does for fmmt_pack_frames).  The caller zeroes *cursor at the start of a split.
 *   One workgroup of 1024 threads; every thread reads *cursor before a barrier and thread 0 stores the new value behind the body, with an ordinary
 *   vector store; launches on one stream are ordered.  1 <= B <= 1024, 1 <= NL <= 8, ld >= NL, out_capacity >= 0, cursor / logits_out / labels_out
 *   non-NULL, else FMMT_EINVAL; loss_sum, count, confusion, labels, cursor, labels_out 8-byte aligned, else FMMT_EALIGN. */
int fmmt_eval_accumulate_at(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, double* loss_sum, int64_t* count,
                            int64_t* confusion, int64_t* cursor, float* logits_out, int64_t* labels_out, int32_t* pred_out, int64_t out_capacity,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
