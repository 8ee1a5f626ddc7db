/* libfmmt_hip -- an evaluation split SHARDED over ranks: the collecting metric update with a device-held row count (a short last batch padded to a
 * captured shape) and the merge of the ranks' gathered accumulators and rows into one split; included by fmmt.h (same ABI rules: plain C,
 * caller-owned buffers, asynchronous on `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_EVAL_SHARD_H
#define FMMT_EVAL_SHARD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* fmmt_eval_accumulate_at (fmmt_eval_collect.h) advances its cursor by the launch argument B and stores every row of the batch: a short batch padded
 * to a captured graph's B would leave holes in the collected split.  A captured graph freezes B; a word in memory it re-reads on every replay.
 *
 * fmmt_eval_accumulate_rows: fmmt_eval_accumulate_at -- same arguments, same kernel body -- plus
 *   n_rows [1] int32 on the device: with b = min(max(*n_rows, 0), B) as the launch finds it, only batch rows i < b exist.  Rows i >= b are neither
 *     stored nor counted, WHATEVER their label (a valid one too), and their logits are not read; *cursor advances by b.
 *   With *n_rows == B every accumulator, every stored row and the cursor get the bits fmmt_eval_accumulate_at leaves; with b == 0 nothing changes
 *     (the loss sum has +0.0 added).  Overflow is reported as there: a row at or behind out_capacity is counted and kept nowhere, *cursor > out_capacity.
 *   One workgroup of 1024 threads; every thread reads *n_rows and *cursor before the first barrier, thread 0 stores the new cursor behind the body.
 *   fmmt_eval_accumulate_at's argument rules, and n_rows non-NULL (FMMT_EINVAL) and 4-byte aligned (FMMT_EALIGN). */
int fmmt_eval_accumulate_rows(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, double* loss_sum, int64_t* count,
                              int64_t* confusion, int64_t* cursor, const int32_t* n_rows, float* logits_out, int64_t* labels_out, int32_t* pred_out,
                              int64_t out_capacity, void* stream);

/* fmmt_eval_merge: W shards of one split, as an all-gather leaves them, become the split.  Rank r evaluated a contiguous block of the dataset with
 * accumulators and buffers of its own; blocks in rank order are the dataset's order.
 *   words   [W][2 + NL*NL + 1] int64: per rank the loss sum (the bits of a double), the row count, the confusion matrix [label][argmax] and the cursor
 *           (the rows that went through the rank's updates) -- the accumulators and the cursor as fmmt_eval_accumulate_at / _rows keep them, adjacent;
 *   results [W][cap][NL] fp32, truths [W][cap] int64: the ranks' collected rows; every rank with the same cap.
 *   words_out [2 + NL*NL + 1], results_out [out_cap][NL], truths_out [out_cap]: the same layout for the whole split.
 * With n_r = min(max(cursor_r, 0), cap) and start_r = n_0 + ... + n_(r-1): row i < n_r of rank r goes to row start_r + i when that is below out_cap,
 * nowhere otherwise; rows of the outputs at or behind n_0 + ... + n_(W-1) are not written, and nothing is read at or behind row n_r of any rank.
 *   loss sum: the ranks' doubles added in rank order by one thread, ((l_0 + l_1) + l_2) ...: the bits are fixed.  Count, confusion: int64 sums.
 *   A rank with cursor_r <= 0 (an empty shard) contributes nothing, to the sums either.
 *   cursor_out = n_0 + ... + n_(W-1) when every cursor_r <= cap and that total is <= out_cap; otherwise out_cap + (rows that went through a rank's
 *   updates and are not in the outputs), which is > out_cap: the overflow report of fmmt_eval_accumulate_at, for the merged split.
 * One launch, no atomics: every workgroup recomputes the W-entry prefix from the gathered cursors; a grid-stride copy; workgroup 0 writes words_out.
 * The outputs must not overlap the inputs.  1 <= W <= 64, 1 <= NL <= 8, cap >= 0, out_cap >= 0, all six pointers non-NULL, else FMMT_EINVAL; words,
 * truths, words_out, truths_out 8-byte aligned, results and results_out 4-byte aligned, else FMMT_EALIGN.  Checked before anything is launched. */
int fmmt_eval_merge(int W, int NL, int64_t cap, int64_t out_cap, const int64_t* words, const float* results, const int64_t* truths, int64_t* words_out,
                    float* results_out, int64_t* truths_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
