"""Writes tests/golden/aff_augment.npz: Pillow's OWN output of the byte stages of the Aff-Wild2 train transform (Grayscale(3), the ColorJitter
operations, GaussianBlur) for 3 frames of 224 x 224 with the table that was applied, and of GaussianBlur alone on a 17 x 17 frame at the sigmas of
fixture_sigmas().  The inputs are not stored: fixture_frames() / fixture_small() rebuild them from synth.randint.
Needs Pillow; run from the repository root:  python -m tests.gen_aff_augment_golden"""
import math
import os

import numpy as np

from facialmmt_amd import synth
from tests import support_aff_augment as A
from tests import support_color_jitter as J

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aff_augment.npz")


def last_sigma_with_r0():
    """the largest float32 sigma whose box radius is still below 1 (fr = 1 at sigma = sqrt(2)), and the next float32 above it"""
    s = np.float32(math.sqrt(2.0))
    while int(np.float32(A.box_radius(float(s)))) >= 1:
        s = np.nextafter(s, np.float32(0))
    return float(s), float(np.nextafter(s, np.float32(4)))


def fixture_sigmas():
    """0.1, 1.0, 2.0, the last sigma with r = 0 and the first with r = 1"""
    lo, hi = last_sigma_with_r0()
    return [0.1, 1.0, 2.0, lo, hi]


def fixture_frames():
    """frame 0: random bytes; 1: low contrast; 2: random with a saturated top, a black bottom and one white pixel in a black block at a band seam"""
    f = synth.randint("aff_augment_golden", (3, 224, 224, 3), 0, 256, seed=5).astype(np.uint8)
    f[1] = (100 + f[1] % 40).astype(np.uint8)
    f[2, :5] = 255
    f[2, -5:] = 0
    f[2, 90:110, 90:110] = 0
    f[2, 100, 100] = 255
    return f


def fixture_small():
    return synth.randint("aff_augment_golden_small", (17, 17, 3), 0, 256, seed=6).astype(np.uint8)


def fixture_table():
    jit = J.make_table([[J.CONTRAST, J.NONE, J.NONE, J.NONE], [J.HUE, J.CONTRAST, J.BRIGHTNESS, J.SATURATION], [J.NONE] * 4],
                       [[1.0, 1.37, 1.0], [0.71, 0.64, 1.4], [1, 1, 1]], [0, J.hue_byte(-0.33), 0])
    return A.make_table([1, 0, 0], jit, [1.7, 0.8, 2.0])


if __name__ == "__main__":
    import PIL
    frames, table = fixture_frames(), fixture_table()
    out = A.pil_chain(frames, [1, 0, 0], table[:, :8], [1.7, 0.8, 2.0])
    small = np.stack([A.pil_blur(fixture_small(), s) for s in fixture_sigmas()])
    np.savez_compressed(PATH, table=table, pil_out=out, small_out=small, sigmas=np.array(fixture_sigmas()), pillow_version=np.array(PIL.__version__))
    print(PATH, os.path.getsize(PATH), "bytes")
