"""On-device draws for the MELD training ColorJitter (the reference: utils/dataset.py:35-39,62-63 -- torchvision's
ColorJitter(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.5) on every face frame of the TRAIN split, between the resize and ToTensor).

The arithmetic runs inside the uint8 pre-step (ops.patch_embed_u8(..., jitter=table), include/fmmt_jitter.h); this module only makes the per-frame
parameter table that kernel reads: one record of 8 int32 words per frame -- the float32 bits of the brightness, contrast and saturation factors, the
hue shift byte, and the operation applied 1st .. 4th (0 brightness, 1 contrast, 2 saturation, 3 hue, 4 none).  The table is threaded explicitly
(PatchEmbed.forward_u8 / SwinTransformer.forward / SwinForAffwildClassification.forward / the target steps' color_jitter=): there is no module-level
switch, because the auxiliary step shares the Swin model and is not jittered by this transform."""
from __future__ import annotations

import ctypes
import math
import numbers

import numpy as np
import torch

from . import _lib


def _range(value, name, center, bound, clip_first_on_zero):
    """torchvision.transforms.ColorJitter._check_input"""
    if value is None:
        return None
    if isinstance(value, numbers.Number):
        if value < 0:
            raise ValueError(f"If {name} is a single number, it must be non negative.")
        value = [center - float(value), center + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        value = [float(value[0]), float(value[1])]
    else:
        raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
    if not bound[0] <= value[0] <= value[1] <= bound[1]:
        raise ValueError(f"{name} values should be between {bound}, but got {value}.")
    return None if value[0] == value[1] == center else (value[0], value[1])


def hue_byte(hue_factor: float) -> int:
    """what torchvision's adjust_hue adds to the uint8 H plane: int(hue_factor * 255) truncated toward zero, mod 256"""
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError(f"hue_factor ({hue_factor}) is not in [-0.5, 0.5].")
    return int(hue_factor * 255) % 256


class ColorJitter:
    """torchvision.transforms.ColorJitter's parameters and draws; the defaults are the reference's amounts.  An amount of 0 or None switches the
    operation off (code 4 in every record), as torchvision skips it."""

    def __init__(self, brightness=0.5, contrast=0.5, saturation=0.5, hue=0.5):
        inf = float("inf")
        self.brightness = _range(brightness, "brightness", 1.0, (0.0, inf), True)
        self.contrast = _range(contrast, "contrast", 1.0, (0.0, inf), True)
        self.saturation = _range(saturation, "saturation", 1.0, (0.0, inf), True)
        self.hue = _range(hue, "hue", 0.0, (-0.5, 0.5), False)

    def __repr__(self):
        return f"ColorJitter(brightness={self.brightness}, contrast={self.contrast}, saturation={self.saturation}, hue={self.hue})"

    def draw(self, n: int, device) -> torch.Tensor:
        """The (n, 8) int32 table of n frames from `device`'s CURRENT generator: one torch.rand and elementwise device ops, no host value and no
        synchronisation -- it can sit inside a captured graph, and a saved generator state replays the same tables.  Factors are U(lo, hi), the
        hue factor U(lo, hi) turned into its shift byte, the order a uniform random permutation (the ranks of four uniforms, ties to the lower code)."""
        u = torch.rand((n, 8), device=device, dtype=torch.float32)
        t = torch.empty((n, _lib.JITTER_WORDS), dtype=torch.int32, device=device)
        for c, rng in enumerate((self.brightness, self.contrast, self.saturation)):
            lo, hi = rng if rng is not None else (1.0, 1.0)
            t[:, c] = (u[:, c] * (hi - lo) + lo).view(torch.int32)
        lo, hi = self.hue if self.hue is not None else (0.0, 0.0)
        t[:, 3] = ((u[:, 3] * (hi - lo) + lo).clamp(-0.5, 0.5) * 255.0).to(torch.int32) & 255        # .to(int32) truncates toward zero
        k = u[:, 4:8]
        idx = torch.arange(4, device=device)
        first = (k.unsqueeze(2) > k.unsqueeze(1)) | ((k.unsqueeze(2) == k.unsqueeze(1)) & (idx.view(1, 4, 1) > idx.view(1, 1, 4)))
        rank = first.sum(2)                                                                          # position of operation i in the frame's order
        order = ((rank.unsqueeze(2) == idx.view(1, 1, 4)) * idx.view(1, 4, 1)).sum(1)                # operation at position k
        for c, rng in enumerate((self.brightness, self.contrast, self.saturation, self.hue)):
            if rng is None:
                order = torch.where(order == c, _lib.JITTER_NONE, order)
        t[:, 4:] = order.to(torch.int32)
        return t

    @staticmethod
    def table(orders, factors, hue, device=None) -> torch.Tensor:
        """A table from explicit values: orders (n, 4) operation codes (4: none), factors (n, 3) brightness / contrast / saturation factors, hue (n,)
        hue FACTORS in [-0.5, 0.5] (converted to shift bytes here).  Checked on the host by the library (fmmt_jitter_table_check): an unknown code or
        an operation named twice in a record is a ValueError."""
        orders = torch.as_tensor(orders, dtype=torch.int32).reshape(-1, 4)
        n = orders.shape[0]
        factors = torch.as_tensor(factors, dtype=torch.float32).reshape(-1, 3)
        hue = [float(h) for h in torch.as_tensor(hue, dtype=torch.float64).reshape(-1).tolist()]
        if n < 1 or factors.shape[0] != n or len(hue) != n:
            raise ValueError(f"ColorJitter.table: {n} orders, {factors.shape[0]} factor rows, {len(hue)} hue factors")
        t = torch.empty((n, _lib.JITTER_WORDS), dtype=torch.int32)
        t[:, :3] = factors.view(torch.int32)
        t[:, 3] = torch.tensor([hue_byte(h) for h in hue], dtype=torch.int32)
        t[:, 4:] = orders
        t = t.contiguous()
        if _lib.load().fmmt_jitter_table_check(ctypes.c_void_p(t.data_ptr()), n) != 0:
            raise ValueError("ColorJitter.table: operation codes are 0 brightness, 1 contrast, 2 saturation, 3 hue, 4 none, each operation at most once per frame")
        return t if device is None else t.to(device)


# ------------------------------------------------------------------------------------------------ the Aff-Wild2 chain of the auxiliary task
def box_radius(sigma: float) -> float:
    """Pillow's _gaussian_blur_radius for three passes (libImaging/BoxBlur.c), in double: the fractional box radius GaussianBlur(radius=sigma) runs"""
    s2 = float(sigma) * float(sigma) / 3.0
    big = math.sqrt(12.0 * s2 + 1.0)
    lo = math.floor((big - 1.0) / 2.0)
    return lo + (2 * lo + 1) * (lo * (lo + 1) - 3 * s2) / (6 * (s2 - (lo + 1) * (lo + 1)))


def box_weights(sigma: float):
    """(r, ww, fw) of one box pass of GaussianBlur(radius=sigma): the radius handed on as a float32, the weights 24-bit fixed point (include/fmmt_aug.h)"""
    fr = np.float32(box_radius(sigma))
    r = int(fr)
    ww = int(np.uint32(np.float32(1 << 24) / (fr * np.float32(2) + np.float32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


class AffWildAugment:
    """The reference's Aff-Wild2 TRAIN transform behind Resize(224, BICUBIC) (utils/util.py:22-60, utils/random_erasing.py), as per-frame draws for the
    uint8 pre-step (ops.patch_embed_u8(..., augment=table), include/fmmt_aug.h): Grayscale(3), ColorJitter(.4, .4, .4, .4), GaussianBlur with
    sigma ~ U(0.1, 2.0), ToTensor / Normalize, RandomErasing(mode='pixel', max_count=1).

    The probabilities are the EFFECTIVE ones: the reference's RandomApply applies its transform when random() > prob (utils/util.py:22-33), so its
    Grayscale prob=0.2 is applied to 0.8 of the frames, its ColorJitter prob=0.8 to 0.2 and its blur prob=0.5 to 0.5; RandomErasing(prob=0.25) erases
    0.25 of them.  A probability of 0 switches a stage off.  An erase makes up to `erase_attempts` draws of a rectangle -- area fraction
    U(erase_area) of the frame, aspect exp(U(ln a, ln 1/a)) with a = erase_min_aspect, h = round(sqrt(area * aspect)), w = round(sqrt(area / aspect)) --
    and takes the first with h < 224 and w < 224, at top ~ randint(0, 224 - h), left ~ randint(0, 224 - w) inclusive; none accepted: nothing erased.

    One record of 20 int32 words per frame: words 0-7 a ColorJitter record (four codes 4: not jittered), 8 flags (bit 0 grayscale), 9-11 the blur's box
    radius r (-1: none) and weights ww, fw, 12-15 the rectangle top, left, h, w (h = 0: none), 16-17 the noise key, 18-19 zero."""
    SIZE = 224

    def __init__(self, grayscale_p=0.8, jitter_p=0.2, jitter=None, blur_p=0.5, sigma=(0.1, 2.0), erase_p=0.25, erase_area=(0.02, 1 / 3),
                 erase_min_aspect=0.3, erase_attempts=10):
        for name, p in (("grayscale_p", grayscale_p), ("jitter_p", jitter_p), ("blur_p", blur_p), ("erase_p", erase_p)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"{name} is a probability, got {p}")
        self.grayscale_p, self.jitter_p, self.blur_p, self.erase_p = float(grayscale_p), float(jitter_p), float(blur_p), float(erase_p)
        self.jitter = ColorJitter(0.4, 0.4, 0.4, 0.4) if jitter is None else jitter
        if not isinstance(self.jitter, ColorJitter):
            raise TypeError(f"jitter: an augment.ColorJitter, got {type(jitter).__name__}")
        self.sigma = (float(sigma[0]), float(sigma[1]))
        if not 0.0 < self.sigma[0] <= self.sigma[1]:
            raise ValueError(f"sigma: a range 0 < lo <= hi, got {sigma}")
        if int(np.float32(box_radius(self.sigma[1]))) > _lib.AUG_MAX_RADIUS:     # the box radius grows with sigma
            raise ValueError(f"sigma up to {self.sigma[1]} needs a box radius of {int(np.float32(box_radius(self.sigma[1])))}: the kernel's halo is sized "
                             f"for r <= {_lib.AUG_MAX_RADIUS}")
        self.erase_area = (float(erase_area[0]), float(erase_area[1]))
        if not 0.0 < self.erase_area[0] <= self.erase_area[1] <= 1.0:
            raise ValueError(f"erase_area: fractions of the frame, 0 < lo <= hi <= 1, got {erase_area}")
        self.erase_min_aspect = float(erase_min_aspect)
        if not 0.0 < self.erase_min_aspect <= 1.0:
            raise ValueError(f"erase_min_aspect in (0, 1], got {erase_min_aspect}")
        self.erase_attempts = int(erase_attempts)
        if self.erase_attempts < 1:
            raise ValueError(f"erase_attempts >= 1, got {erase_attempts}")

    def __repr__(self):
        return (f"AffWildAugment(grayscale_p={self.grayscale_p}, jitter_p={self.jitter_p}, jitter={self.jitter}, blur_p={self.blur_p}, sigma={self.sigma}, "
                f"erase_p={self.erase_p}, erase_area={self.erase_area}, erase_min_aspect={self.erase_min_aspect}, erase_attempts={self.erase_attempts})")

    @staticmethod
    def rectangles(u_area, u_aspect, u_top, u_left, area, min_aspect, size=224):
        """(n, A) uniforms -> per attempt h, w, top, left (int32) and whether the attempt is accepted (1 <= h, w < size): elementwise, any device"""
        a = (u_area * (area[1] - area[0]) + area[0]) * float(size * size)
        la = math.log(min_aspect)
        aspect = torch.exp(u_aspect * (-2.0 * la) + la)
        h = torch.round(torch.sqrt(a * aspect)).to(torch.int32)
        w = torch.round(torch.sqrt(a / aspect)).to(torch.int32)
        ok = (h < size) & (w < size) & (h >= 1) & (w >= 1)
        top = torch.minimum((u_top * (size + 1 - h)).to(torch.int32), size - h)        # randint(0, size - h) inclusive; a uniform below 1 may round up to it
        left = torch.minimum((u_left * (size + 1 - w)).to(torch.int32), size - w)
        return h, w, top, left, ok

    def draw(self, n: int, device) -> torch.Tensor:
        """The (n, 20) int32 table of n frames from `device`'s CURRENT generator: one torch.rand of (n, 5 + 4 * attempts) uniforms -- columns 0-4 decide
        grayscale, jitter, blur, the blur's sigma and erase, then `attempts` columns each of area, aspect, top and left --, ColorJitter.draw's, one
        torch.randint for the noise keys, and elementwise device ops (a cumulative sum picks the first accepted attempt): no host value and no
        synchronisation -- it can sit inside a captured graph, and a saved generator state replays the same tables."""
        A, S = self.erase_attempts, self.SIZE
        u = torch.rand((n, 5 + 4 * A), device=device, dtype=torch.float32)
        jit = self.jitter.draw(n, device)
        key = torch.randint(0, 1 << 32, (n, 2), device=device, dtype=torch.int64)
        t = torch.zeros((n, _lib.AUG_WORDS), dtype=torch.int32, device=device)
        t[:, :8] = jit
        t[:, 4:8] = torch.where((u[:, 1] < self.jitter_p).unsqueeze(1), jit[:, 4:8], _lib.JITTER_NONE)
        t[:, 8] = (u[:, 0] < self.grayscale_p).to(torch.int32) * _lib.AUG_FLAG_GRAY
        # Pillow's radius formula in double, the radius handed on as a float32, the weights in integers (box_weights above, on the device)
        sigma = (u[:, 3] * (self.sigma[1] - self.sigma[0]) + self.sigma[0]).double()
        s2 = sigma * sigma / 3.0
        lo = torch.floor((torch.sqrt(12.0 * s2 + 1.0) - 1.0) / 2.0)
        fr = (lo + (2 * lo + 1) * (lo * (lo + 1) - 3 * s2) / (6 * (s2 - (lo + 1) * (lo + 1)))).float()
        r = fr.to(torch.int64)
        ww = (16777216.0 / (fr * 2 + 1).double()).float().to(torch.int64)                  # float32 / float32 through double: the same rounding
        fw = torch.div((1 << 24) - (2 * r + 1) * ww, 2, rounding_mode="floor")
        blur = u[:, 2] < self.blur_p
        t[:, 9] = torch.where(blur, r, -1).to(torch.int32)
        t[:, 10] = torch.where(blur, ww, 0).to(torch.int32)
        t[:, 11] = torch.where(blur, fw, 0).to(torch.int32)
        h, w, top, left, ok = self.rectangles(u[:, 5:5 + A], u[:, 5 + A:5 + 2 * A], u[:, 5 + 2 * A:5 + 3 * A], u[:, 5 + 3 * A:5 + 4 * A],
                                              self.erase_area, self.erase_min_aspect, S)
        first = (ok & (torch.cumsum(ok.to(torch.int32), 1) == 1) & (u[:, 4] < self.erase_p).unsqueeze(1)).to(torch.int32)   # at most one per row
        for c, v in enumerate((top, left, h, w)):
            t[:, 12 + c] = (v * first).sum(1)
        t[:, 16:18] = (key - ((key >> 31) << 32)).to(torch.int32)                          # the 32 bits, as a signed word
        return t

    @staticmethod
    def table(gray, jitter=None, sigma=None, rect=None, key=None, device=None) -> torch.Tensor:
        """A table from explicit values, n = len(gray) frames: gray (n,) bools; jitter None or an (n, 8) ColorJitter table (ColorJitter.table);
        sigma None or (n,) GaussianBlur radii (0 or None per frame: no blur), turned into box weights by Pillow's double-precision formula here;
        rect None or (n, 4) top, left, h, w (h = 0: nothing erased); key None or (n, 2) 32-bit noise keys.  Checked on the host by the library
        (fmmt_aug_table_check): a bad jitter record, a box radius above 1, a rectangle outside the frame or with h or w >= 224 is a ValueError."""
        gray = [bool(g) for g in gray]
        n = len(gray)
        if n < 1:
            raise ValueError("AffWildAugment.table: no frames")
        t = torch.zeros((n, _lib.AUG_WORDS), dtype=torch.int32)
        t[:, 4:8] = _lib.JITTER_NONE
        t[:, :3] = torch.ones((n, 3), dtype=torch.float32).view(torch.int32)
        if jitter is not None:
            jitter = torch.as_tensor(jitter).cpu()
            if jitter.dtype != torch.int32 or tuple(jitter.shape) != (n, _lib.JITTER_WORDS):
                raise ValueError(f"AffWildAugment.table: the jitter table is ({n}, {_lib.JITTER_WORDS}) int32, got {tuple(jitter.shape)} {jitter.dtype}")
            t[:, :8] = jitter
        t[:, 8] = torch.tensor([_lib.AUG_FLAG_GRAY if g else 0 for g in gray], dtype=torch.int32)
        t[:, 9] = -1
        if sigma is not None:
            sigma = list(sigma)
            if len(sigma) != n:
                raise ValueError(f"AffWildAugment.table: {n} frames, {len(sigma)} sigmas")
            for i, s in enumerate(sigma):
                if s is None or float(s) == 0.0:
                    continue
                if float(s) < 0.0:
                    raise ValueError(f"AffWildAugment.table: sigma {s} of frame {i} is negative")
                r, ww, fw = box_weights(float(s))
                if ww >= 1 << 31:
                    raise ValueError(f"AffWildAugment.table: sigma {s} of frame {i} is too small for a box weight")
                t[i, 9], t[i, 10], t[i, 11] = r, ww, fw
        if rect is not None:
            rect = torch.as_tensor(rect, dtype=torch.int32).reshape(-1, 4)
            if rect.shape[0] != n:
                raise ValueError(f"AffWildAugment.table: {n} frames, {rect.shape[0]} rectangles")
            t[:, 12:16] = rect
        if key is not None:
            key = torch.as_tensor(key, dtype=torch.int64).reshape(-1, 2)
            if key.shape[0] != n:
                raise ValueError(f"AffWildAugment.table: {n} frames, {key.shape[0]} keys")
            key = key & 0xFFFFFFFF
            t[:, 16:18] = (key - ((key >> 31) << 32)).to(torch.int32)
        t = t.contiguous()
        if _lib.load().fmmt_aug_table_check(ctypes.c_void_p(t.data_ptr()), n) != 0:
            raise ValueError("AffWildAugment.table: a jitter record ColorJitter.table refuses, a blur whose box radius exceeds 1, or a "
                             "rectangle that is not inside the 224 x 224 frame with 1 <= h, w < 224")
        return t if device is None else t.to(device)
