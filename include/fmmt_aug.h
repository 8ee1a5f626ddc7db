/* libfmmt_hip -- the Aff-Wild2 training augmentation of the auxiliary task inside the uint8 pre-step; included by fmmt.h (same ABI rules: plain C,
 * caller-owned buffers, asynchronous on `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_AUG_H
#define FMMT_AUG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reference trains the auxiliary task on Aff-Wild2 crops put through (utils/util.py:22-60, utils/random_erasing.py), after Resize(224, BICUBIC):
 *   RandomApply(Grayscale(3))            applied with probability 0.8 (the reference's RandomApply applies when random() > prob, prob = 0.2)
 *   RandomApply(ColorJitter(.4,.4,.4,.4))                        0.2
 *   RandomApply(GaussianBlur, sigma ~ U(0.1, 2.0))               0.5
 *   ToTensor, Normalize(.5, .5)
 *   RandomErasing(prob = 0.25, mode = 'pixel', max_count = 1)    on the normalised tensor
 * The two entry points below are fmmt_patch_embed_u8 / fmmt_patch_embed_u8_ln_fwd (fmmt.h) with that chain between the resize's bytes and the patch
 * gather.  Grayscale, jitter and blur are integer or exactly rounded and BIT-EXACT with Pillow (tests/support_aff_augment.py restates them in numpy
 * and is held to Pillow itself); the erased rectangle is filled with N(0, 1) values of the counter-based generator stated below.
 *
 * The random draws are an INPUT: aug_dev is a DEVICE table of one record per frame, FMMT_AUG_WORDS 32-bit words each:
 *   words 0-7    a ColorJitter record (fmmt_jitter.h; four FMMT_JITTER_NONE codes: not jittered)
 *   word  8      flags; bit FMMT_AUG_FLAG_GRAY: Grayscale(3) in front of the jitter
 *   words 9-11   the box blur: r (-1: no blur; 0 or 1), ww, fw
 *   words 12-15  the erased rectangle: top, left, h, w in the 224 x 224 frame (h = 0: none)
 *   words 16-17  the noise key k0, k1
 *   words 18-19  zero
 * On the device a blur radius other than 0 or 1 counts as "no blur", the jitter codes as in fmmt_jitter.h, and the rectangle is intersected with the
 * frame; fmmt_aug_table_check refuses such records where the table is on the host.
 *
 * Grayscale: R = G = B = L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Pillow's convert("L")).  Contrast's whole-frame mean is taken behind it.
 * Blur: PIL.ImageFilter.GaussianBlur(radius = sigma) is three box passes along x, then three along y, on every channel.  In double, then float32:
 *   s2 = sigma^2 / 3, L = sqrt(12 s2 + 1), l = floor((L - 1) / 2), fr = l + (2l + 1)(l(l + 1) - 3 s2) / (6 (s2 - (l + 1)^2))
 *   r = (int)fr, ww = (uint32)((float)(1 << 24) / (fr * 2 + 1)), fw = ((1 << 24) - (2r + 1) ww) / 2
 * and one pass at position i, in uint32, indices clamped to the image:
 *   out = (ww * sum_{d = -r..r} in[i + d] + fw * (in[i - r - 1] + in[i + r + 1]) + (1 << 23)) >> 24
 * fr <= 1.375 over sigma in [0.1, 2.0], so r <= FMMT_AUG_MAX_RADIUS = 1: a pass reaches 2 pixels, the six passes FMMT_AUG_HALO = 6 rows.
 * Noise: element (channel c, row y, column x) of a frame has the counter n = (c * 224 + y) * 224 + x.  With mix32a / mix32b
 *   mix32a(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   mix32b(x): x ^= x >> 17; x *= 0xed5ad4bb; x ^= x >> 11; x *= 0xac4c1b51; x ^= x >> 15
 *   ka = mix32a(k0 ^ 0x9e3779b9), kb = mix32b(k1 ^ 0x7f4a7c15)                    (the key enters hashed: no key is a shifted counter)
 *   h1 = mix32a(mix32b(n ^ ka) + kb),  h2 = mix32b(mix32a(n + kb) ^ ka)           (all in uint32)
 *   u1 = ((h1 >> 8) + 1) * 2^-24, u2 = (h2 >> 8) * 2^-24,  z = sqrt(-2 ln u1) * cos(2 pi u2)   in float32
 * with the library's logf, sqrtf and sinf, the cosine taken as sin(pi (1/2 - min(x, 2 - x))), x = 2 u2: both reductions are exact in float32, so z
 * keeps its relative accuracy at the cosine's zero crossings (no fast intrinsics).  |z| <= 5.77.  The blur never sees the noise: it runs on bytes, the rectangle is filled behind the Normalize table.
 *
 * Three launches on `stream`, on the same grid (56 bands x n_img): the contrast statistic with the grayscale in front (fmmt_jitter.h; frames
 * without contrast leave at once), the resize + grayscale + jitter of a band written as bytes to frames_ws, and the finish, which stages a band's
 * rows with the blur's halo from frames_ws in LDS, blurs, applies the table and the rectangle and gathers (and projects + normalises).
 * partial: n_img * FMMT_JITTER_BANDS int32 words; frames_ws: n_img * 224 * 224 * 3 bytes (fmmt_aug_workspace_bytes), 16-byte aligned; both are
 * written then read by the call (nothing to zero, no atomics: capture-safe).
 *
 * Arguments as in fmmt_patch_embed_u8_jitter / _jitter_ln_fwd, with frames_ws and its size behind partial.  NULL aug_dev / partial / frames_ws:
 * FMMT_EINVAL; frames_ws smaller than fmmt_aug_workspace_bytes: FMMT_EWORKSPACE; misaligned: FMMT_EALIGN.  FMMT_BF16 / FMMT_F32. */
#define FMMT_AUG_WORDS 20
#define FMMT_AUG_FLAG_GRAY 1
#define FMMT_AUG_MAX_RADIUS 1
#define FMMT_AUG_HALO 6

/* HOST: 0 if every record of table[n_img][20] passes fmmt_jitter_table_check on its first 8 words, has no flag but FMMT_AUG_FLAG_GRAY, r in -1..1
 * with (for r >= 0) ww > 0 and fw == ((1 << 24) - (2r + 1) ww) / 2 >= 0, a rectangle with h = 0 or 1 <= h, w < 224 inside the frame, and zero in
 * words 18-19; else FMMT_EINVAL. */
int fmmt_aug_table_check(const int32_t* table, int n_img);
size_t fmmt_aug_workspace_bytes(int n_img);
int fmmt_patch_embed_u8_aug(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev, const float* lut_dev,
                            const int32_t* aug_dev, int32_t* partial, void* frames_ws, size_t ws_bytes, void* cols, void* stream);
int fmmt_patch_embed_u8_aug_ln_fwd(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev, const float* lut_dev,
                                   const int32_t* aug_dev, int32_t* partial, void* frames_ws, size_t ws_bytes, const void* w, const float* bias,
                                   const float* ln_gamma, const float* ln_beta, float eps, void* cols, void* x_pre, void* y, float* mean, float* rstd,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
