// The optimizer update that leaves everything alone when the gradient norm is not finite (include/fmmt_guard.h), for steps that run as captured
// graphs: no norm or loss reaches the host there, so the decision GradScaler takes on the host in the reference (train.py:139-143) is taken on
// the device, and what happened is counted in six int64 words the host reads when it likes.
//
// fmmt_adamw_batch_guarded: adamw_batch_body (adamw_core.h, the body of fmmt_adamw_batch) behind one scalar load and a block-uniform branch.  The
//   step word holds the update count BEFORE the update and is only read: all blocks of the launch must see the same t, so the one writer of the
//   word is the kernel behind it.
// fmmt_guard_commit: that kernel -- one thread advances the step word when the norm was finite and counts the update as applied or skipped.
// fmmt_monitor_loss: one thread adds a finite loss into a double and counts it, or counts a non-finite one.
// Launches on a stream are ordered and each kernel has a single writer: ordinary loads and stores, no atomics.
#include "fmmt_common.h"
#include "adamw_core.h"
#include "../../include/fmmt.h"

namespace {

__global__ __launch_bounds__(256) void adamw_batch_guarded_kernel(const AdamDesc* __restrict__ desc, int n_desc, const float* __restrict__ lr_p,
                                                                  const float* __restrict__ step_p, const float* __restrict__ norm_p,
                                                                  float beta1, float beta2, float eps, float wd, float max_norm, int hf) {
    if (!finite_bits(*norm_p)) return;                       // block-uniform: nothing of p, m, v or the twins is read or written
    const int r = adamw_find_record(desc, n_desc);
    adamw_batch_body<true>(desc[r], AdamHyper{*lr_p, beta1, beta2, eps, wd}, step_p, norm_p, max_norm, hf);
}

__global__ __launch_bounds__(64) void guard_commit_kernel(const float* __restrict__ norm_p, float* __restrict__ step, long long* __restrict__ words) {
    if (threadIdx.x != 0) return;
    const float norm = *norm_p;
    if (finite_bits(norm)) {
        *step += 1.0f;
        words[FMMT_GUARD_APPLIED] += 1;
    } else {
        words[FMMT_GUARD_SKIPPED] += 1;
    }
    words[FMMT_GUARD_LAST_NORM] = (long long)__float_as_uint(norm);
}

__global__ __launch_bounds__(64) void monitor_loss_kernel(const float* __restrict__ loss, float scale, long long* __restrict__ words) {
    if (threadIdx.x != 0) return;
    const float x = *loss * scale;
    if (finite_bits(x)) {
        double* sum = reinterpret_cast<double*>(words + FMMT_GUARD_LOSS_SUM);
        *sum += (double)x;
        words[FMMT_GUARD_MICRO_STEPS] += 1;
    } else {
        words[FMMT_GUARD_NONFINITE_LOSSES] += 1;
    }
}

}  // namespace

extern "C" int fmmt_adamw_batch_guarded(int n_desc, int n_blocks, const void* desc, const float* lr, const float* step, const float* total_norm,
                                        float beta1, float beta2, float eps, float weight_decay, float max_norm, int hf_semantics, void* stream) {
    if (n_desc <= 0 || n_blocks <= 0 || !desc || !lr || !step || !total_norm) return FMMT_EINVAL;
    hipLaunchKernelGGL(adamw_batch_guarded_kernel, dim3((unsigned)n_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const AdamDesc*>(desc), n_desc, lr, step, total_norm, beta1, beta2, eps, weight_decay, max_norm, hf_semantics);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_guard_commit(const float* total_norm, float* step, int64_t* words, void* stream) {
    if (!total_norm || !step || !words) return FMMT_EINVAL;
    if (reinterpret_cast<uintptr_t>(words) & 7) return FMMT_EALIGN;
    hipLaunchKernelGGL(guard_commit_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), total_norm, step,
                       reinterpret_cast<long long*>(words));
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_monitor_loss(const float* loss, float scale, int64_t* words, void* stream) {
    if (!loss || !words) return FMMT_EINVAL;
    if (reinterpret_cast<uintptr_t>(words) & 7) return FMMT_EALIGN;
    hipLaunchKernelGGL(monitor_loss_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), loss, scale,
                       reinterpret_cast<long long*>(words));
    FMMT_CHECK_LAUNCH();
    return 0;
}
