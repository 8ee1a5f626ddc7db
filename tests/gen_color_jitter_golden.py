"""Writes tests/golden/color_jitter.npz: Pillow's OWN output of the four ColorJitter operations (what torchvision's ColorJitter calls on a PIL
image) for 4 frames of 224 x 224, with the tables that were applied.  The inputs are not stored: fixture_frames() rebuilds them from synth.randint.
Needs Pillow; run from the repository root:  python -m tests.gen_color_jitter_golden"""
import os

import numpy as np

from facialmmt_amd import synth
from tests import support_color_jitter as J

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter.npz")


def fixture_frames():
    """frame 0, 1: random bytes; 2: low contrast (a 40-wide band: contrast and saturation clip on neither side at small factors, the mean matters);
    3: random with a saturated top, a black bottom and a grey (R = G = B) stripe"""
    f = synth.randint("color_jitter_golden", (4, 224, 224, 3), 0, 256, seed=3).astype(np.uint8)
    f[2] = (100 + f[2] % 40).astype(np.uint8)
    f[3, :5] = 255
    f[3, -5:] = 0
    f[3, 100:110] = f[3, 100:110, :, :1]
    return f


def fixture_table():
    orders = [[J.HUE, J.CONTRAST, J.BRIGHTNESS, J.SATURATION], [J.CONTRAST, J.SATURATION, J.HUE, J.BRIGHTNESS],
              [J.SATURATION, J.BRIGHTNESS, J.CONTRAST, J.HUE], [J.BRIGHTNESS, J.HUE, J.SATURATION, J.CONTRAST]]
    factors = [[0.62, 1.41, 0.55], [1.37, 0.71, 1.49], [1.12, 1.5, 1.33], [0.5, 0.93, 0.8]]
    return J.make_table(orders, factors, [J.hue_byte(h) for h in (0.31, -0.5, -0.07, 0.5)])


if __name__ == "__main__":
    import PIL
    frames, table = fixture_frames(), fixture_table()
    out = J.pil_apply_table(frames, table)
    np.savez_compressed(PATH, table=table, pil_out=out, pillow_version=np.array(PIL.__version__))
    print(PATH, os.path.getsize(PATH), "bytes")
