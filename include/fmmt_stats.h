/* libfmmt_hip -- per-tensor statistics over the fused optimizer's descriptor table: which tensor holds the NaN, how large each tensor's gradient
 * is; included by fmmt.h (same ABI rules: plain C, caller-owned buffers, asynchronous on `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_STATS_H
#define FMMT_STATS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* After loss.backward() in the reference (train.py:135-143) every p.grad is there to inspect, between clip_grad_norm_ (train.py:140) and
 * optimizer.step() (train.py:141).  A captured step has no such moment: the leaves' .grad are None, the flat fp32 buffers are zeroed behind
 * every update, and a skipped update (fmmt_guard.h) reports a NaN norm without saying which of ~700 tensors it came from.  fmmt_table_stats is
 * that moment on the device: launched between the clip norm and the update, it reduces ONE field of every record of the descriptor table of
 * fmmt_adamw_batch (fmmt.h: records {p, g, m, v, low, n, first block, g_is_bf16} in blocks of 4096 elements; n_blocks is that table's block
 * count) to three numbers per record.
 *
 * which: the field that is read */
#define FMMT_STATS_G 0   /* the gradient field (honours g_is_bf16) */
#define FMMT_STATS_P 1
#define FMMT_STATS_M 2
#define FMMT_STATS_V 3
/* stats: n_desc records { float sumsq; float max_abs; int32 nonfinite; int32 reserved (0); }  (16 bytes), record j of the table in stats[j].
 * Over the n elements x of the field (a bf16 gradient is converted to fp32 first, which is exact):
 *   sumsq     the fp32 sum of x * x.  NaN and inf propagate; two finite 3e19 entries give inf -- the overflow the guarded update skips on.
 *   max_abs   the largest |x| over the elements that are not NaN: 0 when there is none, inf when an inf is present.
 *   nonfinite how many elements have every exponent bit set (NaN, +-inf): the bit test of the guarded update.
 * Two launches on `stream`:
 *   1. one workgroup per 4096-element block finds its record by the binary search of fmmt_adamw_batch and reads its elements once -- 16-byte
 *      loads where the address allows it (16-byte alignment for fp32, 8 for a bf16 gradient: fmmt_adamw_batch's rule), element by element
 *      otherwise and in a record's last partial quad -- and writes one 16-byte triple into partial[block].
 *   2. one workgroup per record reduces that record's triples and writes stats[j].
 * Every reduction runs in an order the table alone fixes (lane, wave, workgroup, block); there are no atomics: two calls give the same bits,
 * and the call is capture-safe.
 *   partial: 16 * n_blocks bytes of scratch, written then read by this call.
 *
 * norm, bad_stats, bad_words: the snapshot of a bad update; all three may be NULL (statistics on demand).  norm is the device word the guarded
 * update decides on (fmmt_adamw_batch_guarded's total_norm).  When it is given, launch 2 tests *norm after it wrote stats; when its exponent bits
 * are all set (NaN or +-inf),
 *   bad_stats (n_desc records, the layout of stats; may be NULL) receives a copy of stats,
 *   bad_words[0] += 1 (bad_words: two int64 words, zeroed by the caller at the start of what it counts; may be NULL),
 *   bad_words[1] = the index of the first record with nonfinite > 0 or a non-finite sumsq, -1 when there is none (a norm that overflowed over
 *     records that are each finite).
 * On a finite norm bad_stats and bad_words are not touched, so they keep the last bad update until the caller zeroes them.  Each word has a
 * single writer (ordinary vector stores, ordered by the stream), as in fmmt_guard_commit.
 *
 * Checked before anything is launched: NULL desc / partial / stats, n_desc < 1, n_blocks < 1, which outside 0..3, bad_stats or bad_words without
 * norm: FMMT_EINVAL; partial, stats or bad_stats not 16-byte aligned, bad_words not 8-byte aligned: FMMT_EALIGN.
 * The field is read once: 4 bytes per element (2 for a bf16 gradient) of HBM traffic, nothing else of that size. */
int fmmt_table_stats(int which, int n_desc, int n_blocks, const void* desc, void* partial, void* stats, const float* norm, void* bad_stats,
                     int64_t* bad_words, void* stream);

#ifdef __cplusplus
}
#endif
#endif
