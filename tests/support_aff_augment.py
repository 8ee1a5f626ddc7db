"""The reference's Aff-Wild2 train transform behind Resize(224, BICUBIC) (utils/util.py:22-60, utils/random_erasing.py) restated in numpy: Grayscale(3),
ColorJitter (tests/support_color_jitter.py), Pillow's GaussianBlur, and RandomErasing's noise rectangle on the normalised tensor.
tests/test_aff_augment_cpu.py holds the byte stages to Pillow itself (np.array_equal) and to tests/golden/aff_augment.npz; the GPU tests use
`apply_table` and `erase` as the oracle of fmmt_patch_embed_u8_aug.

A table is what the kernel reads (include/fmmt_aug.h): one record of 20 int32 words per frame -- words 0-7 a ColorJitter record, 8 flags (bit 0:
grayscale), 9-11 the blur's box radius r (-1: none) and weights ww, fw, 12-15 the erased rectangle top, left, h, w (h = 0: none), 16-17 the noise key,
18-19 zero."""
import math

import numpy as np

from tests import support_color_jitter as J

WORDS, FLAG_GRAY, MAX_RADIUS, HALO, SIZE = 20, 1, 1, 6, 224


def gray(img):
    """Grayscale(3): Pillow's convert("L") copied to three channels"""
    return np.repeat(J.luma(img)[..., None], 3, axis=-1)


def box_radius(sigma, passes=3):
    """Pillow's _gaussian_blur_radius (libImaging/BoxBlur.c), in double"""
    s2 = sigma * sigma / passes
    big = math.sqrt(12.0 * s2 + 1.0)
    lo = math.floor((big - 1.0) / 2.0)
    return lo + (2 * lo + 1) * (lo * (lo + 1) - 3 * s2) / (6 * (s2 - (lo + 1) * (lo + 1)))


def box_weights(sigma):
    """(r, ww, fw): the radius handed on as a float32, the weights 24-bit fixed point (ImagingLineBoxBlur)"""
    fr = np.float32(box_radius(float(sigma)))
    r = int(fr)
    ww = int(np.uint32(np.float32(1 << 24) / (fr * np.float32(2) + np.float32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def line_pass(a, r, ww, fw):
    """one box pass along the last axis of a uint8 array, indices clamped to the line, in uint32: windowed sums, no running accumulator"""
    n = a.shape[-1]
    idx = np.arange(n)
    acc = np.zeros(a.shape, np.int64)
    for d in range(-r, r + 1):
        acc += a[..., np.clip(idx + d, 0, n - 1)]
    far = a[..., np.clip(idx - r - 1, 0, n - 1)].astype(np.int64) + a[..., np.clip(idx + r + 1, 0, n - 1)]
    bulk = (acc * ww + far * fw) & 0xFFFFFFFF
    return (((bulk + (1 << 23)) & 0xFFFFFFFF) >> 24).astype(np.uint8)


def box_blur(img, r, ww, fw):
    """(H, W, 3) uint8: three passes along x, then three along y, on every channel"""
    x = np.moveaxis(img, 2, 0)
    for _ in range(3):
        x = line_pass(x, r, ww, fw)
    x = np.swapaxes(x, 1, 2)
    for _ in range(3):
        x = line_pass(x, r, ww, fw)
    return np.ascontiguousarray(np.moveaxis(np.swapaxes(x, 1, 2), 0, 2))


def gaussian_blur(img, sigma):
    """PIL.ImageFilter.GaussianBlur(radius=sigma) on an RGB image"""
    return box_blur(img, *box_weights(sigma))


# ---- the noise generator of include/fmmt_aug.h
def _u32(x):
    return np.asarray(x).astype(np.uint64) & np.uint64(0xFFFFFFFF)


def mix32a(x):
    x = _u32(x)
    x ^= x >> np.uint64(16)
    x = _u32(x * np.uint64(0x7FEB352D))
    x ^= x >> np.uint64(15)
    x = _u32(x * np.uint64(0x846CA68B))
    x ^= x >> np.uint64(16)
    return x


def mix32b(x):
    x = _u32(x)
    x ^= x >> np.uint64(17)
    x = _u32(x * np.uint64(0xED5AD4BB))
    x ^= x >> np.uint64(11)
    x = _u32(x * np.uint64(0xAC4C1B51))
    x ^= x >> np.uint64(15)
    return x


def noise_words(counter, k0, k1):
    """the two 32-bit hashes h1, h2 of the counters under the key (k0, k1)"""
    n = _u32(counter)
    ka, kb = mix32a(_u32(int(k0) & 0xFFFFFFFF) ^ np.uint64(0x9E3779B9)), mix32b(_u32(int(k1) & 0xFFFFFFFF) ^ np.uint64(0x7F4A7C15))
    return mix32a(_u32(mix32b(n ^ ka) + kb)), mix32b(mix32a(_u32(n + kb)) ^ ka)


def noise(counter, k0, k1):
    """N(0, 1) of the counters, float64: Box-Muller on two 24-bit uniforms, u1 in (0, 1]"""
    h1, h2 = noise_words(counter, k0, k1)
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    x = (h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -23                             # 2 u2, exact, in [0, 2)
    x = np.minimum(x, 2.0 - x)                                                            # cos(pi x) = cos(pi (2 - x)) = sin(pi (1/2 - x)): exact reductions,
    return np.sqrt(-2.0 * np.log(u1)) * np.sin(np.pi * (0.5 - x))                         # so the zero crossings keep their relative accuracy


def counters(size=SIZE):
    """(3, size, size): element (c, y, x) has the counter (c * size + y) * size + x"""
    return np.arange(3 * size * size, dtype=np.int64).reshape(3, size, size)


def make_table(gray_flags, jitter=None, sigma=None, rect=None, key=None):
    """(n,) flags, (n, 8) jitter table or None, (n,) sigmas (None / 0: no blur), (n, 4) rectangles, (n, 2) keys -> the (n, 20) int32 table"""
    n = len(gray_flags)
    t = np.zeros((n, WORDS), np.int32)
    t[:, :3] = np.ones((n, 3), np.float32).view(np.int32)
    t[:, 4:8] = J.NONE
    if jitter is not None:
        t[:, :8] = jitter
    t[:, 8] = [FLAG_GRAY if g else 0 for g in gray_flags]
    t[:, 9] = -1
    for i, s in enumerate(sigma if sigma is not None else []):
        if s:
            t[i, 9:12] = box_weights(s)
    if rect is not None:
        t[:, 12:16] = np.asarray(rect, np.int32).reshape(n, 4)
    if key is not None:
        t[:, 16:18] = (np.asarray(key, np.int64).reshape(n, 2) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return t


def apply_table(frames, table):
    """the byte stages: (n, H, W, 3) uint8 frames, (n, 20) int32 table -> grayscale, jitter (contrast's mean behind the grayscale), blur"""
    table = np.ascontiguousarray(np.asarray(table, np.int32))
    out = []
    for i in range(frames.shape[0]):
        img = frames[i]
        if table[i, 8] & FLAG_GRAY:
            img = gray(img)
        img = J.apply_table(img[None], table[i:i + 1, :8])[0]
        if table[i, 9] >= 0:
            img = box_blur(img, int(table[i, 9]), int(table[i, 10]) & 0xFFFFFFFF, int(table[i, 11]) & 0xFFFFFFFF)
        out.append(img)
    return np.stack(out)


def erase(chw, table):
    """RandomErasing on the normalised tensors: (n, 3, S, S) float -> float64 with each frame's rectangle overwritten by its noise; and the mask"""
    table = np.asarray(table, np.int32)
    out = chw.astype(np.float64).copy()
    mask = np.zeros(chw.shape, bool)
    ctr = counters(chw.shape[-1])
    for i in range(chw.shape[0]):
        top, left, h, w = (int(v) for v in table[i, 12:16])
        if h > 0:
            mask[i, :, top:top + h, left:left + w] = True
            out[i][mask[i]] = noise(ctr[mask[i]], int(table[i, 16]), int(table[i, 17]))
    return out, mask


# ---- Pillow's own; imported lazily: the GPU machine needs none of it
def pil_gray(img):
    from PIL import Image
    return np.array(Image.fromarray(img, "RGB").convert("L").convert("RGB"))


def pil_blur(img, sigma):
    from PIL import Image, ImageFilter
    return np.array(Image.fromarray(img, "RGB").filter(ImageFilter.GaussianBlur(radius=float(sigma))))


def pil_chain(frames, gray_flags, jitter, sigma):
    """the reference's order on PIL images: Grayscale(3), the jitter record's operations, GaussianBlur"""
    out = []
    for i in range(frames.shape[0]):
        img = frames[i]
        if gray_flags[i]:
            img = pil_gray(img)
        if jitter is not None:
            img = J.pil_apply_table(img[None], jitter[i:i + 1])[0]
        if sigma[i]:
            img = pil_blur(img, sigma[i])
        out.append(img)
    return np.stack(out)
