// Clip + AdamW + bf16 twins over a descriptor table whose records belong to parameter groups (include/fmmt_groups.h): adamw_batch_body
// (adamw_core.h, the body of fmmt_adamw_batch and fmmt_adamw_batch_guarded) with the learning rate, betas, eps and weight decay read per RECORD
// instead of per launch.  Nothing of the arithmetic, the 4096-element block map, the alignment fallbacks or the bf16 twins is restated here.
//
// What a block adds to the one-group kernel: behind the binary search that finds its record, one int32 (group_of[record]), one 32-byte group
// record and the group's lr word.  All three addresses are block-uniform and the memory is only read, so they are scalar loads; a streaming
// kernel of 28-30 bytes per element over 4096 elements per block does not see 40 bytes more.
#include "fmmt_common.h"
#include "adamw_core.h"
#include "../../include/fmmt.h"

namespace {

static_assert(sizeof(fmmt_adamw_group) == FMMT_ADAMW_GROUP_BYTES && FMMT_ADAMW_GROUP_BYTES % 16 == 0, "the group record of include/fmmt_groups.h");

template <bool GUARDED>
__device__ __forceinline__ void adamw_groups_block(const AdamDesc* __restrict__ desc, int n_desc, const int* __restrict__ group_of,
                                                   const fmmt_adamw_group* __restrict__ groups, const float* __restrict__ step_p,
                                                   const float* __restrict__ norm_p, float max_norm, int hf) {
    const int r = adamw_find_record(desc, n_desc);
    const fmmt_adamw_group g = groups[group_of[r]];
    // a pointer that comes out of memory is a generic one to the compiler, and a generic load is a per-lane flat load; the record holds a device
    // (global-memory) address by contract, and said so the uniform load of the word is a scalar one like the three in front of it
    const float lr = *(const __attribute__((address_space(1))) float*)g.lr;
    adamw_batch_body<GUARDED>(desc[r], AdamHyper{lr, g.beta1, g.beta2, g.eps, g.weight_decay}, step_p, norm_p, max_norm, hf);
}

__global__ __launch_bounds__(256) void adamw_groups_kernel(const AdamDesc* __restrict__ desc, int n_desc, const int* __restrict__ group_of,
                                                           const fmmt_adamw_group* __restrict__ groups, const float* __restrict__ step_p,
                                                           const float* __restrict__ norm_p, float max_norm, int hf) {
    adamw_groups_block<false>(desc, n_desc, group_of, groups, step_p, norm_p, max_norm, hf);
}

__global__ __launch_bounds__(256) void adamw_groups_guarded_kernel(const AdamDesc* __restrict__ desc, int n_desc, const int* __restrict__ group_of,
                                                                   const fmmt_adamw_group* __restrict__ groups, const float* __restrict__ step_p,
                                                                   const float* __restrict__ norm_p, float max_norm, int hf) {
    if (!finite_bits(*norm_p)) return;                       // block-uniform: nothing of p, m, v or the twins is read or written
    adamw_groups_block<true>(desc, n_desc, group_of, groups, step_p, norm_p, max_norm, hf);
}

}  // namespace

extern "C" int fmmt_adamw_groups(int n_desc, int n_blocks, const void* desc, int n_groups, const int32_t* group_of, const void* groups,
                                 const float* step, const float* total_norm, float max_norm, int hf_semantics, void* stream) {
    if (n_groups <= 0 || n_desc <= 0 || n_blocks <= 0 || !desc || !group_of || !groups || !step) return FMMT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(groups) & 7) || (reinterpret_cast<uintptr_t>(group_of) & 3)) return FMMT_EALIGN;
    hipLaunchKernelGGL(adamw_groups_kernel, dim3((unsigned)n_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const AdamDesc*>(desc), n_desc, reinterpret_cast<const int*>(group_of),
                       reinterpret_cast<const fmmt_adamw_group*>(groups), step, total_norm, max_norm, hf_semantics);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_adamw_groups_guarded(int n_desc, int n_blocks, const void* desc, int n_groups, const int32_t* group_of, const void* groups,
                                         const float* step, const float* total_norm, float max_norm, int hf_semantics, void* stream) {
    if (n_groups <= 0 || n_desc <= 0 || n_blocks <= 0 || !desc || !group_of || !groups || !step || !total_norm) return FMMT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(groups) & 7) || (reinterpret_cast<uintptr_t>(group_of) & 3)) return FMMT_EALIGN;
    hipLaunchKernelGGL(adamw_groups_guarded_kernel, dim3((unsigned)n_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const AdamDesc*>(desc), n_desc, reinterpret_cast<const int*>(group_of),
                       reinterpret_cast<const fmmt_adamw_group*>(groups), step, total_norm, max_norm, hf_semantics);
    FMMT_CHECK_LAUNCH();
    return 0;
}
