"""torchvision's ColorJitter on a PIL image (the MELD train transform, utils/dataset.py:35-39,62-63) restated in numpy on uint8 RGB arrays: the four
Pillow operations it is made of, each rounding to uint8 before the next.  tests/test_color_jitter_cpu.py holds every function here to Pillow itself
(np.array_equal) and to tests/golden/color_jitter.npz; the GPU tests use `apply_table` as the oracle of fmmt_patch_embed_u8_jitter.

A table is what the kernel reads (include/fmmt_jitter.h): one record of 8 int32 words per frame -- words 0-2 the float32 bits of the brightness,
contrast and saturation factors, word 3 the hue shift byte, words 4-7 the operation applied 1st..4th (0 brightness, 1 contrast, 2 saturation,
3 hue, 4 none)."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE, NONE = 0, 1, 2, 3, 4


def luma(img):
    """Pillow's RGB -> L (ImagingConvert rgb2l): integer, rounded"""
    a = img.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """Image.blend(degenerate, image, f): float32, the product rounded before the sum, clipped, truncated"""
    d, x, f = deg.astype(np.float32), img.astype(np.float32), np.float32(f)
    t = d + f * (x - d)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.float32)
    return out.astype(np.int32).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast_mean(img):
    """ImageEnhance.Contrast's int(mean(L) + 0.5), in integers"""
    L = luma(img)
    n = L.size
    return int((2 * int(L.sum(dtype=np.int64)) + n) // (2 * n))


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, f)


def rgb2hsv(img):
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(np.float32)
        s = cr / mx.astype(np.float32)
        rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (r, g, b))
        h = np.where(r == mx, bc - gc,
                     np.where(g == mx, (2.0 + rc.astype(np.float64) - bc).astype(np.float32), (4.0 + gc.astype(np.float64) - rc).astype(np.float32)))
        h = np.fmod(h.astype(np.float32).astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
        H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H, S = np.where(grey, 0, H), np.where(grey, 0, S)
    return np.stack([H, S, mx], axis=-1).astype(np.uint8)


def _round_away(x):
    """C round(): half away from zero (x - trunc(x) is exact)"""
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def hsv2rgb(hsv):
    H, S, V = (hsv[..., k] for k in range(3))
    fh = H.astype(np.float32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(fh)
    f = (fh - i.astype(np.float32)).astype(np.float32).astype(np.float64)
    fs = (S.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)
    v = V.astype(np.float64)
    p = np.clip(_round_away(v * (1.0 - fs)), 0, 255).astype(np.uint8)
    q = np.clip(_round_away(v * (1.0 - fs * f)), 0, 255).astype(np.uint8)
    t = np.clip(_round_away(v * (1.0 - fs * (1.0 - f))), 0, 255).astype(np.uint8)
    k = i.astype(np.int64) % 6
    R = np.choose(k, [V, q, p, p, t, V])
    G = np.choose(k, [t, V, V, q, p, p])
    B = np.choose(k, [p, p, t, V, V, q])
    out = np.stack([R, G, B], axis=-1).astype(np.uint8)
    return np.where((S == 0)[..., None], np.repeat(V[..., None], 3, axis=-1), out).astype(np.uint8)


def hue_byte(hue_factor):
    """torchvision adjust_hue: np.uint8(hue_factor * 255) added to the uint8 H plane"""
    return int(hue_factor * 255) % 256


def hue(img, shift_byte):
    hsv = rgb2hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift_byte)) & 255
    return hsv2rgb(hsv)


def apply_ops(img, order, fb, fc, fs, shift_byte):
    """one frame (H, W, 3) uint8 through the operations `order` names (codes above; anything else: none), in order"""
    for code in order:
        if code == BRIGHTNESS:
            img = brightness(img, fb)
        elif code == CONTRAST:
            img = contrast(img, fc)
        elif code == SATURATION:
            img = saturation(img, fs)
        elif code == HUE:
            img = hue(img, shift_byte)
    return img


def make_table(orders, factors, hue_bytes):
    """(n, 4) codes, (n, 3) factors, (n,) shift bytes -> the (n, 8) int32 table"""
    orders = np.asarray(orders, np.int32).reshape(-1, 4)
    n = orders.shape[0]
    t = np.empty((n, 8), np.int32)
    t[:, :3] = np.asarray(factors, np.float32).reshape(n, 3).view(np.int32)
    t[:, 3] = np.asarray(hue_bytes, np.int64).reshape(n) & 255
    t[:, 4:] = orders
    return t


def apply_table(frames, table):
    """(n, H, W, 3) uint8 frames, (n, 8) int32 table -> the jittered frames"""
    table = np.ascontiguousarray(np.asarray(table, np.int32))
    fac = table[:, :3].copy().view(np.float32)
    return np.stack([apply_ops(frames[i], [int(c) for c in table[i, 4:]], fac[i, 0], fac[i, 1], fac[i, 2], int(table[i, 3]) & 255)
                     for i in range(frames.shape[0])])


# ---- Pillow's own (what torchvision's ColorJitter calls on a PIL image); imported lazily: the GPU machine needs none of it
def pil_op(img, code, factor_or_byte):
    from PIL import Image, ImageEnhance
    im = Image.fromarray(img, "RGB")
    if code == BRIGHTNESS:
        return np.array(ImageEnhance.Brightness(im).enhance(float(factor_or_byte)))
    if code == CONTRAST:
        return np.array(ImageEnhance.Contrast(im).enhance(float(factor_or_byte)))
    if code == SATURATION:
        return np.array(ImageEnhance.Color(im).enhance(float(factor_or_byte)))
    if code == HUE:                                   # torchvision.transforms._functional_pil.adjust_hue, with the byte already formed
        h, s, v = im.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h += np.uint8(factor_or_byte)
        return np.array(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
    return img


def pil_apply_table(frames, table):
    table = np.ascontiguousarray(np.asarray(table, np.int32))
    fac = table[:, :3].copy().view(np.float32)
    out = []
    for i in range(frames.shape[0]):
        img = frames[i]
        for c in table[i, 4:]:
            c = int(c)
            img = pil_op(img, c, int(table[i, 3]) & 255 if c == HUE else (fac[i, c] if c < 3 else 0))
        out.append(img)
    return np.stack(out)
