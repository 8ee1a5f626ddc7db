"""On-device draws for the MELD training ColorJitter (the reference: utils/dataset.py:35-39,62-63 -- torchvision's
ColorJitter(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.5) on every face frame of the TRAIN split, between the resize and ToTensor).

The arithmetic runs inside the uint8 pre-step (ops.patch_embed_u8(..., jitter=table), include/fmmt_jitter.h); this module only makes the per-frame
parameter table that kernel reads: one record of 8 int32 words per frame -- the float32 bits of the brightness, contrast and saturation factors, the
hue shift byte, and the operation applied 1st .. 4th (0 brightness, 1 contrast, 2 saturation, 3 hue, 4 none).  The table is threaded explicitly
(PatchEmbed.forward_u8 / SwinTransformer.forward / SwinForAffwildClassification.forward / the target steps' color_jitter=): there is no module-level
switch, because the auxiliary step shares the Swin model and is not jittered by this transform."""
from __future__ import annotations

import ctypes
import numbers

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
