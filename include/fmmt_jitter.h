/* libfmmt_hip -- the MELD training ColorJitter inside the uint8 pre-step; included by fmmt.h (same ABI rules: plain C, caller-owned buffers,
 * asynchronous on `stream`, 0 / hipError_t / FMMT_E* return codes). */
#ifndef FMMT_JITTER_H
#define FMMT_JITTER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reference puts every face frame of the MELD TRAIN split through torchvision's ColorJitter(brightness=.5, contrast=.5, saturation=.5, hue=.5)
 * (utils/dataset.py:35-39,62-63), after the cv2 resize and before ToTensor / Normalize; validation and test frames are not jittered.  On a PIL image
 * that transform is four Pillow operations on the uint8 RGB image, in a random order per image, each rounding to uint8 before the next.  The two
 * entry points below are fmmt_patch_embed_u8 / fmmt_patch_embed_u8_ln_fwd (fmmt.h) with those operations between the resize's bytes and the
 * ToTensor / Normalize table: resize (either flavour) -> the frame's operations in the frame's order -> table -> patch gather (-> projection +
 * LayerNorm).  Bit-exact with Pillow (tests/support_color_jitter.py restates the arithmetic in numpy and is held to Pillow itself).
 *
 * The random draws are an INPUT, as the Gumbel noise of fmmt_emotion_head_fwd is: jitter_dev is a DEVICE table of one record per frame,
 * FMMT_JITTER_WORDS 32-bit words each:
 *   words 0-2  the brightness, contrast and saturation factors (float32 bits)
 *   word  3    the hue shift byte: int(hue_factor * 255) truncated toward zero, mod 256 (torchvision adds it to the uint8 H plane)
 *   words 4-7  the operation applied 1st .. 4th: FMMT_JITTER_BRIGHTNESS / _CONTRAST / _SATURATION / _HUE / _NONE
 * _NONE in all four: the frame is not jittered (the bits of fmmt_patch_embed_u8).  On the device any other code, and a second contrast in one
 * record, count as _NONE; fmmt_jitter_table_check refuses them where the table is on the host.
 *
 * The operations, on a pixel's (R, G, B) bytes.  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
 *   blend(d, f, x) = t <= 0 ? 0 : t >= 255 ? 255 : (int)t,  t = d + f * (x - d) in float32, the product rounded before the sum (Image.blend)
 *   brightness: d = 0.   saturation: d = L of the pixel.
 *   contrast:   d = (2 * sum(L) + N) / (2 * N) in integers, N = 224 * 224, the sum over the whole frame AS IT IS when contrast is applied
 *               (after the operations that precede it in this frame's order) -- Pillow's int(mean + 0.5).
 *   hue:        Pillow's RGB -> HSV, H = (H + shift) & 255, HSV -> RGB (libImaging/Convert.c), float / double mixed as there.
 *
 * partial: n_img * FMMT_JITTER_BANDS int32 words of scratch for the contrast statistic, written then read by the call (nothing to zero, no
 * atomics: capture-safe).  Two launches on `stream`, on the same grid (56 bands x n_img): the first resizes, applies what precedes contrast and
 * writes each band's integer sum of L (frames without contrast leave at once), the second sums a frame's 56 integers and does the rest.  The
 * 224 x 224 image is never materialised; the crops are read twice.
 *
 * Arguments as in fmmt_patch_embed_u8 / fmmt_patch_embed_u8_ln_fwd, with jitter_dev and partial behind lut_dev.  NULL jitter_dev / partial:
 * FMMT_EINVAL; either not 4-byte aligned: FMMT_EALIGN.  FMMT_BF16 / FMMT_F32 (the parity instantiation of the same template). */
#define FMMT_JITTER_WORDS 8
#define FMMT_JITTER_BANDS 56
#define FMMT_JITTER_BRIGHTNESS 0
#define FMMT_JITTER_CONTRAST 1
#define FMMT_JITTER_SATURATION 2
#define FMMT_JITTER_HUE 3
#define FMMT_JITTER_NONE 4

/* HOST: 0 if every record of table[n_img][8] holds codes 0..4 with no operation but _NONE twice and a shift byte in 0..255, else FMMT_EINVAL. */
int fmmt_jitter_table_check(const int32_t* table, int n_img);
int fmmt_patch_embed_u8_jitter(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev, const float* lut_dev,
                               const int32_t* jitter_dev, int32_t* partial, void* cols, void* stream);
int fmmt_patch_embed_u8_jitter_ln_fwd(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev,
                                      const float* lut_dev, const int32_t* jitter_dev, int32_t* partial, const void* w, const float* bias,
                                      const float* ln_gamma, const float* ln_beta, float eps, void* cols, void* x_pre, void* y, float* mean,
                                      float* rstd, void* stream);

#ifdef __cplusplus
}
#endif
#endif
