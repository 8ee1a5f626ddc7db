/* libfmmt_hip -- the optimizer update that is SKIPPED when the gradient norm is not finite, and the run's counters kept on the device; included
 * by fmmt.h (same ABI rules: plain C, caller-owned buffers, asynchronous on `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_GUARD_H
#define FMMT_GUARD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reference trains its T+A+V configuration under native AMP (main.py:152-160): GradScaler leaves optimizer.step() out when a gradient holds
 * an inf or a NaN, and scheduler.step() still runs (train.py:139-143).  fmmt_adamw_batch has no such protection: a NaN norm gives a clip
 * coefficient of 1, an infinite norm 0 and inf * 0 = NaN, and either way the moments, the parameters and the bf16 twins are NaN from then on.
 * The three entry points below are that protection for captured steps, where no norm or loss reaches the host: the decision is taken on the
 * device from the norm word, and what happened is counted in `words`.
 *
 * words: ONE contiguous int64 device array of FMMT_GUARD_WORDS entries, 8-byte aligned, zeroed by the caller at the start of what it counts: */
#define FMMT_GUARD_LOSS_SUM 0          /* double bits: sum of the finite losses fmmt_monitor_loss saw */
#define FMMT_GUARD_MICRO_STEPS 1       /* how many losses that sum holds */
#define FMMT_GUARD_NONFINITE_LOSSES 2  /* losses that were NaN or +-inf (not summed) */
#define FMMT_GUARD_APPLIED 3           /* updates applied (fmmt_guard_commit found a finite norm) */
#define FMMT_GUARD_SKIPPED 4           /* updates skipped (the norm was NaN or +-inf) */
#define FMMT_GUARD_LAST_NORM 5         /* float bits of the norm fmmt_guard_commit saw last, zero-extended */
#define FMMT_GUARD_WORDS 6

/* fmmt_adamw_batch_guarded: fmmt_adamw_batch -- the same descriptor table, the same arguments, the same kernel body -- with two differences.
 *   total_norm is required (NULL: FMMT_EINVAL).  Every block reads *total_norm first; when it is NaN or +-inf the block returns before it touches
 *     anything: p, m, v and the bf16 twins keep their bits.
 *   *step is the update count BEFORE this update: the kernel uses t = *step + 1.0f and never writes step (fmmt_guard_commit does, behind it).
 *   On a finite norm the result has the bits of fmmt_adamw_batch called with the step word holding *step + 1. */
int fmmt_adamw_batch_guarded(int n_desc, int n_blocks, const void* desc, const float* lr, const float* step, const float* total_norm,
                             float beta1, float beta2, float eps, float weight_decay, float max_norm, int hf_semantics, void* stream);

/* fmmt_guard_commit: one workgroup, launched BEHIND fmmt_adamw_batch_guarded on the same stream -- stream order is what lets it write the word the
 * update's blocks only read.  Finite *total_norm: *step += 1 and words[APPLIED] += 1; otherwise step is unchanged and words[SKIPPED] += 1; in
 * both cases words[LAST_NORM] = the norm's bits.  One thread, ordinary vector stores.  NULL pointer: FMMT_EINVAL; words not 8-byte aligned:
 * FMMT_EALIGN. */
int fmmt_guard_commit(const float* total_norm, float* step, int64_t* words, void* stream);

/* fmmt_monitor_loss: one workgroup, once per micro-step, behind the loss.  x = *loss * scale (one fp32 product); finite: words[LOSS_SUM] (a
 * double) += (double)x and words[MICRO_STEPS] += 1; otherwise words[NONFINITE_LOSSES] += 1.  `scale` is the accumulation factor the step divided
 * its loss by, so the sum is of the undivided batch means, the number the reference logs (train.py:144-150).  NULL pointer: FMMT_EINVAL; words
 * not 8-byte aligned: FMMT_EALIGN. */
int fmmt_monitor_loss(const float* loss, float scale, int64_t* words, void* stream);

#ifdef __cplusplus
}
#endif
#endif
