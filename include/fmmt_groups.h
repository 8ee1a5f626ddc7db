/* libfmmt_hip -- clip + AdamW + bf16 twins over a descriptor table whose records belong to PARAMETER GROUPS, each with its own learning rate, betas,
 * eps and weight decay; included by fmmt.h (same ABI rules: plain C, caller-owned buffers, asynchronous on `stream`, 0 / hipError_t / FMMT_E*
 * return codes). */
#ifndef FMMT_GROUPS_H
#define FMMT_GROUPS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* fmmt_adamw_batch takes one lr word and one beta1 / beta2 / eps / weight_decay per LAUNCH: one parameter group.  An optimizer with several groups
 * (no decay on biases and LayerNorm weights, a smaller or layer-wise decayed learning rate for the text encoder, a group held still with lr = 0)
 * is one launch too: the two entry points below read those five values per RECORD, from a small device table.
 *
 * The descriptor table is fmmt_adamw_batch's, byte for byte (56-byte records, include/fmmt.h; fmmt_param_digest reads the same table).  The group
 * of a record travels beside it:
 *   group_of: n_desc int32 on the device, group_of[i] in [0, n_groups) = the group of record i.  The kernel does not range-check it -- a value
 *             outside the range reads outside `groups`; the caller checks before upload (train_step.group_plan does).
 *   groups:   n_groups records of FMMT_ADAMW_GROUP_BYTES (32) bytes on the device, 8-byte aligned: */
typedef struct fmmt_adamw_group {
    const float* lr;    /* byte  0: DEVICE pointer to the group's learning-rate word (a 0-dim fp32 tensor a scheduler fills); groups may share one */
    float beta1;        /* byte  8 */
    float beta2;        /* byte 12 */
    float eps;          /* byte 16 */
    float weight_decay; /* byte 20 */
    uint32_t pad[2];    /* byte 24: zero; pads the record to a 16-byte multiple */
} fmmt_adamw_group;
#define FMMT_ADAMW_GROUP_BYTES 32

/* fmmt_adamw_groups: fmmt_adamw_batch with (lr, beta1, beta2, eps, weight_decay) = groups[group_of[record]] -- the same block map (one workgroup per
 *   4096 elements of one record), the same kernel body, the same alignment fallbacks and bf16 twins.  step, total_norm, max_norm and hf_semantics
 *   stay per launch: ONE update count and ONE clip coefficient for all groups, as clip_grad_norm_(model.parameters()) gives.  The result has the
 *   bits of one fmmt_adamw_batch call per group over that group's records with the same step and norm words.  total_norm may be NULL (no clip).
 *   n_groups < 1, n_desc < 1, n_blocks < 1, or a NULL desc / group_of / groups / step: FMMT_EINVAL; groups not 8-byte or group_of not 4-byte
 *   aligned: FMMT_EALIGN; nothing launched in either case. */
int fmmt_adamw_groups(int n_desc, int n_blocks, const void* desc, int n_groups, const int32_t* group_of, const void* groups, const float* step,
                      const float* total_norm, float max_norm, int hf_semantics, void* stream);

/* fmmt_adamw_groups_guarded: to fmmt_adamw_groups what fmmt_adamw_batch_guarded (fmmt_guard.h) is to fmmt_adamw_batch.  total_norm is required
 *   (NULL: FMMT_EINVAL); every block reads it first and returns before it touches anything when it is NaN or +-inf.  *step is the update count
 *   BEFORE this update (t = *step + 1.0f) and is never written: fmmt_guard_commit runs behind it on the same stream, unchanged. */
int fmmt_adamw_groups_guarded(int n_desc, int n_blocks, const void* desc, int n_groups, const int32_t* group_of, const void* groups,
                              const float* step, const float* total_norm, float max_norm, int hf_semantics, void* stream);

#ifdef __cplusplus
}
#endif
#endif
