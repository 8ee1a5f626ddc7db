/* libfmmt_hip -- ragged frame counts behind one fixed shape; included by fmmt.h (same ABI rules: plain C, caller-owned buffers, asynchronous on
 * `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_RAGGED_H
#define FMMT_RAGGED_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A MELD batch has a different number of face frames in every utterance: the loader hands over (B, Lv, ...) zero-padded frames and the real count per
 * utterance (utils/dataset.py:275-292) and the reference concatenates the real ones on the host (train.py:60-71), so the tensor Swin sees changes its
 * first dimension with every batch -- which a captured HIP graph cannot follow.  These entry points keep ONE shape: the batch is packed on the device
 * into a buffer of F_cap rows, the real frames in the reference's concatenation order at the front, zeros behind, and a DEVICE word n_valid says how
 * many rows are real.  Every op of Swin is per frame except the three below; nothing else has to know about n_valid.
 *
 * fmmt_pack_frames: src [B][Lv][row_bytes] (any element type: it moves bytes -- 37 632 per 112x112x3 uint8 crop, 301 056 / 602 112 per bf16 / fp32
 *   3x224x224 frame), num_imgs [B] int64 on the device -> dst [F_cap][row_bytes].  With n_u = clamp(num_imgs[u], 0, Lv) and total = sum n_u, row r < total
 *   of dst is frame k of utterance u, r = n_0 + ... + n_{u-1} + k (torch.cat([src[u, :n_u] for u])); rows >= total are zero-filled; rows of the
 *   concatenation at or behind F_cap are DROPPED (nothing is written out of bounds).  counts [2] int32: counts[0] = min(total, F_cap) -- the n_valid
 *   of the calls below --, counts[1] = total (> F_cap tells the caller that frames were dropped).  16-byte vector loads and stores, one launch.
 *   B <= 256 (the prefix sum lives in LDS, as in fmmt_select_frames_fwd), F_cap <= 65535, else FMMT_EINVAL; row_bytes % 16 != 0 or src / dst not
 *   16-byte aligned: FMMT_EALIGN.
 *
 * fmmt_batchnorm1d_fwd_n / _bwd_n: fmmt_batchnorm1d_fwd / _bwd (Swin_Transformer.py:434-541, the embedding head's nn.BatchNorm1d) over the first
 *   *n_valid rows of buffers that hold n_cap rows (n_valid: device word, clamped to [0, n_cap], read once per workgroup; n_cap sizes the launch).
 *   Training mode: batch statistics, the running-statistics update (unbiased variance over n_valid rows) and, backward, dgamma / dbeta and the two
 *   column sums run over those rows only.  y and dx of rows >= n_valid are written as ZEROS; x and dy there are never read.  (The unmasked backward
 *   gives a row with dy = 0 the value -k (sum(dy) / n + xhat sum(dy xhat) / n): the one path by which padded frames would reach every Swin weight
 *   gradient.)  Same kernel body, same summation order (16 row groups added in group order): n_valid == n_cap gives the bits of the unmasked
 *   entry points.  n_valid == 1: variance 0, running variance updated with 0, dx = 0 -- what the reference's duplicate-the-sample rule computes
 *   (Swin_Transformer.forward, ref :535-538); the one output row is evaluated centred, (x - mean) invstd gamma + beta = beta exactly, because the
 *   folded offset beta - mean gamma invstd of the general path is rounded at the magnitude of mean gamma / sqrt(eps) (1.5e-5 off beta, measured).  n_valid == 0: zeros, running statistics untouched.  One launch each, as the unmasked pair.
 *
 * fmmt_select_frames_fwd_n: fmmt_select_frames_fwd (fmmt.h; train.py:75-114) on preds [nF = F_cap][NL] whose rows >= *n_valid are padding: the
 *   "did any face of the batch pass the threshold" decision (train.py:80,84) looks at the rows g < *n_valid only -- a padded row above the threshold
 *   must not move the batch from the keep-everything branch to the selection branch.  (Ownership needs no change: an owned face lies below
 *   the largest utterance boundary max_u (sum_{i<=u} num_imgs_i - u) <= sum(num_imgs) = n_valid.)  n_valid == NULL: fmmt_select_frames_fwd.  The backward is fmmt_select_frames_bwd: a gather through
 *   src_face, which never names a padded row. */
int fmmt_pack_frames(int B, int Lv, int F_cap, size_t row_bytes, const void* src, const int64_t* num_imgs, void* dst, int32_t* counts, void* stream);
int fmmt_batchnorm1d_fwd_n(int dtype, int n_cap, int C, const int32_t* n_valid, const void* x, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, int training, void* y, float* save_mean,
                           float* save_invstd, void* stream);
int fmmt_batchnorm1d_bwd_n(int dtype, int n_cap, int C, const int32_t* n_valid, const void* dy, const void* x, const float* gamma,
                           const float* save_mean, const float* save_invstd, int training, void* dx, float* dgamma, float* dbeta, void* stream);
int fmmt_select_frames_fwd_n(int dtype, int nF, int NL, int B, int Lv, int D, const float* preds, const void* vision_inputs,
                             const float* vision_mask, const int64_t* num_imgs, float threshold, void* out, float* new_mask, int32_t* src_face,
                             const int32_t* n_valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif
