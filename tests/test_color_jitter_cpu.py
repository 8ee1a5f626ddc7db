"""CPU tests of the MELD training ColorJitter: the numpy restatement the GPU tests use as their oracle (tests/support_color_jitter.py) held to Pillow
itself and to Pillow's recorded output (tests/golden/color_jitter.npz, written by tests/gen_color_jitter_golden.py), the parameter tables of
facialmmt_amd.augment.ColorJitter, and the ABI surface of include/fmmt_jitter.h (header == _lib.JITTER_SIGNATURES == the built library)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import support_color_jitter as J
from tests.gen_color_jitter_golden import fixture_frames, fixture_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow():
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        pytest.skip("Pillow is not installed: the restatement is still held to Pillow's recorded output (tests/golden/color_jitter.npz)")


def _frames():
    rng = np.random.default_rng(11)
    rand = rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    low = rng.integers(100, 140, (224, 224, 3), dtype=np.uint8)        # within a 40-wide band
    return rand, low


@pytest.mark.parametrize("code", [J.BRIGHTNESS, J.CONTRAST, J.SATURATION])
def test_each_blend_equals_pillow(code):
    _pillow()
    for img in _frames():
        for f in (0.5, 0.77, 1.0, 1.23, 1.5):
            f = np.float32(f)
            assert np.array_equal(J.apply_ops(img, [code], f, f, f, 0), J.pil_op(img, code, f)), (code, f)


def test_hue_equals_pillow():
    _pillow()
    for img in _frames():
        for b in (0, 1, 127, 128, 255):
            assert np.array_equal(J.hue(img, b), J.pil_op(img, J.HUE, b)), b


def test_hsv_conversions_equal_pillow_over_all_colours():
    _pillow()
    from PIL import Image
    a = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([a >> 16, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    assert np.array_equal(J.rgb2hsv(img), np.array(Image.fromarray(img, "RGB").convert("HSV")))
    assert np.array_equal(J.hsv2rgb(img), np.array(Image.frombytes("HSV", (4096, 4096), img.tobytes()).convert("RGB")))


def test_all_24_orders_equal_pillow():
    """random and low-contrast frame: the amounts make contrast and saturation clip on both sides, and contrast's mean is the mean of the frame as
    the operations in front of it left it"""
    _pillow()
    frames = np.stack(_frames())
    for k, order in enumerate(itertools.permutations(range(4))):
        fac = [[0.5 + 0.04 * k, 1.5 - 0.03 * k, 0.55 + 0.035 * k], [1.5 - 0.04 * k, 0.5 + 0.04 * k, 1.45 - 0.03 * k]]
        table = J.make_table([order, order], fac, [(37 * k + 5) & 255, (91 * k + 128) & 255])
        assert np.array_equal(J.apply_table(frames, table), J.pil_apply_table(frames, table)), order


def test_restatement_equals_the_pillow_fixture(golden):
    z = golden.files["color_jitter"]
    assert np.array_equal(z["table"], fixture_table())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "color_jitter.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "preproc.npz"))
    got = J.apply_table(fixture_frames(), z["table"])
    assert got.shape == (4, 224, 224, 3) and np.array_equal(got, z["pil_out"])
    assert not np.array_equal(z["pil_out"], fixture_frames())


def test_none_code_and_partial_orders():
    img = _frames()[0]
    assert np.array_equal(J.apply_ops(img, [4, 4, 4, 4], 0.5, 0.5, 0.5, 77), img)
    one = J.apply_ops(img, [4, J.SATURATION, 4, 4], 0.5, 0.5, np.float32(0.6), 77)
    assert np.array_equal(one, J.saturation(img, np.float32(0.6))) and not np.array_equal(one, img)
    assert np.array_equal(J.hue(img, 0)[img.max(-1) == img.min(-1)], img[img.max(-1) == img.min(-1)])          # grey pixels survive any hue
    assert J.contrast_mean(np.full((224, 224, 3), 255, np.uint8)) == 255 and J.contrast_mean(np.zeros((224, 224, 3), np.uint8)) == 0


# ------------------------------------------------------------------------------------------------ augment.ColorJitter
def test_range_checks_are_torchvisions():
    from facialmmt_amd.augment import ColorJitter
    cj = ColorJitter()
    assert cj.brightness == cj.contrast == cj.saturation == (0.5, 1.5) and cj.hue == (-0.5, 0.5)
    assert ColorJitter(brightness=2.0).brightness == (0.0, 3.0)                      # clipped at zero
    assert ColorJitter(0, None, (1, 1), 0).__dict__ == dict(brightness=None, contrast=None, saturation=None, hue=None)
    assert ColorJitter(contrast=(0.2, 0.9)).contrast == (0.2, 0.9)
    for bad in (dict(brightness=-0.1), dict(hue=0.6), dict(hue=(-0.7, 0.1)), dict(saturation=(1.2, 0.8)), dict(contrast=(-1, 1))):
        with pytest.raises(ValueError):
            ColorJitter(**bad)
    with pytest.raises(TypeError):
        ColorJitter(brightness="a lot")
    with pytest.raises(TypeError):
        ColorJitter(hue=(0.1, 0.2, 0.3))


def test_draw_on_the_cpu_generator():
    from facialmmt_amd.augment import ColorJitter
    torch.manual_seed(5)
    state = torch.get_rng_state()
    t = ColorJitter().draw(2000, "cpu")
    assert t.shape == (2000, 8) and t.dtype == torch.int32
    fac = t[:, :3].contiguous().view(torch.float32)
    assert (fac >= 0.5).all() and (fac <= 1.5).all() and fac.std(0).min() > 0.2
    assert (t[:, 3] >= 0).all() and (t[:, 3] <= 255).all() and len(set(t[:, 3].tolist())) > 200
    assert (t[:, 4:].sort(1).values == torch.arange(4, dtype=torch.int32)).all()       # every row a permutation
    assert len(set(map(tuple, t[:, 4:].tolist()))) == 24                               # and all of them occur
    torch.set_rng_state(state)
    assert torch.equal(ColorJitter().draw(2000, "cpu"), t)                             # the generator is the only state
    assert not torch.equal(ColorJitter().draw(2000, "cpu"), t)
    # a narrow hue range: the shift bytes of U(-0.1, 0.1) * 255 truncated toward zero, mod 256
    h = ColorJitter(hue=0.1).draw(500, "cpu")[:, 3]
    assert set(h.tolist()) <= set(range(0, 26)) | set(range(231, 256))
    # switched-off operations: code 4 in their place, the rest still a random order of what is left
    t = ColorJitter(brightness=0, contrast=None, saturation=0.3, hue=0.2).draw(300, "cpu")
    assert (t[:, 4:].sort(1).values == torch.tensor([2, 3, 4, 4], dtype=torch.int32)).all()
    assert (t[:, :2].contiguous().view(torch.float32) == 1.0).all()
    assert (ColorJitter(0, 0, 0, 0).draw(4, "cpu")[:, 4:] == 4).all()


def test_table_from_explicit_values():
    from facialmmt_amd.augment import ColorJitter, hue_byte
    t = ColorJitter.table([[3, 1, 4, 0], [4, 4, 4, 4]], [[0.5, 1.0, 1.5], [1, 1, 1]], [0.5, -0.5])
    assert t.dtype == torch.int32 and t.shape == (2, 8)
    assert np.array_equal(t.numpy(), J.make_table([[3, 1, 4, 0], [4, 4, 4, 4]], [[0.5, 1.0, 1.5], [1, 1, 1]], [127, 129]))
    hs = (0.0, 0.5, -0.5, 0.004, -0.004, 0.499, -0.003)                              # truncation toward zero: -0.765 -> 0
    assert [hue_byte(h) for h in hs] == [0, 127, 129, 1, 255, 127, 0] == [J.hue_byte(h) for h in hs]
    for orders in ([[5, 0, 1, 2]], [[-1, 4, 4, 4]], [[1, 1, 4, 4]], [[0, 3, 2, 3]]):
        with pytest.raises(ValueError):
            ColorJitter.table(orders, [[1, 1, 1]], [0.0])
    with pytest.raises(ValueError):
        ColorJitter.table([[0, 1, 2, 3]], [[1, 1, 1]], [0.6])
    with pytest.raises(ValueError):
        ColorJitter.table([[0, 1, 2, 3]], [[1, 1, 1], [1, 1, 1]], [0.1])


# ------------------------------------------------------------------------------------------------ ABI surface
def _lib_built():
    from facialmmt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_jitter_header_signatures_and_library_agree():
    """include/fmmt_jitter.h (included by fmmt.h) == _lib.JITTER_SIGNATURES == the symbols of the built library: names, every argument's type and the
    return type, as tests/test_eval_shard_cpu.py does for its header; the table is disjoint from the eight that exist"""
    from facialmmt_amd import _lib, build
    assert "color_jitter.hip" in build.SOURCES and "preproc.hip" in build.SOURCES
    assert '#include "fmmt_jitter.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    raw = open(os.path.join(ROOT, "include", "fmmt_jitter.h")).read()
    assert "utils/dataset.py:35-39,62-63" in raw
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.JITTER_SIGNATURES) == ["fmmt_jitter_table_check", "fmmt_patch_embed_u8_jitter", "fmmt_patch_embed_u8_jitter_ln_fwd"]
    for other in (_lib.SIGNATURES, _lib.POOL_HEAD_SIGNATURES, _lib.RAGGED_SIGNATURES, _lib.EVAL_COLLECT_SIGNATURES, _lib.POOL_HEAD_ROWS_SIGNATURES,
                  _lib.GUARD_SIGNATURES, _lib.DIGEST_SIGNATURES, _lib.EVAL_SHARD_SIGNATURES):
        assert not set(_lib.JITTER_SIGNATURES) & set(other)

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}[base]
    for name, args in protos.items():
        res, got = _lib.JITTER_SIGNATURES[name]
        assert got == [ctype_of(a) for a in args.split(",") if a.strip()], name
        assert res is C.c_int and re.search(r"\bint\s+" + name + r"\s*\(", src), name
    # the existing pre-step pair with the table and the scratch put in behind lut_dev
    for new, old in (("fmmt_patch_embed_u8_jitter", "fmmt_patch_embed_u8"), ("fmmt_patch_embed_u8_jitter_ln_fwd", "fmmt_patch_embed_u8_ln_fwd")):
        a = list(_lib.JITTER_SIGNATURES[new][1])
        assert a[7:9] == [C.c_void_p, C.c_void_p] and a[:7] + a[9:] == _lib.SIGNATURES[old][1]
    defines = dict(re.findall(r"#define\s+(FMMT_JITTER_\w+)\s+(\d+)", src))
    assert {k: int(v) for k, v in defines.items()} == dict(FMMT_JITTER_WORDS=_lib.JITTER_WORDS, FMMT_JITTER_BANDS=_lib.JITTER_BANDS,
                                                           FMMT_JITTER_BRIGHTNESS=J.BRIGHTNESS, FMMT_JITTER_CONTRAST=J.CONTRAST,
                                                           FMMT_JITTER_SATURATION=J.SATURATION, FMMT_JITTER_HUE=J.HUE, FMMT_JITTER_NONE=J.NONE)
    assert (_lib.JITTER_BRIGHTNESS, _lib.JITTER_CONTRAST, _lib.JITTER_SATURATION, _lib.JITTER_HUE, _lib.JITTER_NONE) == (0, 1, 2, 3, 4)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in _lib.JITTER_SIGNATURES) and "fmmt_jitter.h" in text and "color_jitter=" in text
    lib = _lib_built()
    assert all(hasattr(lib, name) for name in _lib.JITTER_SIGNATURES)


def test_arguments_are_validated_before_any_launch():
    from facialmmt_amd import _lib
    lib = _lib_built()
    buf = (C.c_char * 512)()
    p = C.addressof(buf)
    p += -p % 16

    def plain(dtype=1, mode=0, n=2, S=160, img=p, tab=p, lut=p, jit=p, partial=p, cols=p):
        return lib.fmmt_patch_embed_u8_jitter(dtype, mode, n, S, img, tab, lut, jit, partial, cols, None)
    for bad in (dict(dtype=2), dict(mode=2), dict(n=0), dict(n=65536), dict(S=3), dict(S=225), dict(img=None), dict(tab=None), dict(lut=None), dict(jit=None),
                dict(partial=None), dict(cols=None)):
        assert plain(**bad) == _lib.FMMT_EINVAL, bad
    for bad in (dict(tab=p + 4), dict(cols=p + 8), dict(jit=p + 2), dict(partial=p + 1)):
        assert plain(**bad) == _lib.FMMT_EALIGN, bad

    def fused(dtype=1, mode=1, n=2, S=160, jit=p, partial=p, w=p, y=p, mean=p, rstd=p, cols=None):
        return lib.fmmt_patch_embed_u8_jitter_ln_fwd(dtype, mode, n, S, p, p, p, jit, partial, w, None, p, p, 1e-5, cols, None, y, mean, rstd, None)
    for bad in (dict(dtype=3), dict(mode=-1), dict(n=0), dict(S=300), dict(jit=None), dict(partial=None), dict(w=None), dict(y=None), dict(mean=None)):
        assert fused(**bad) == _lib.FMMT_EINVAL, bad
    for bad in (dict(jit=p + 2), dict(partial=p + 3), dict(w=p + 8), dict(cols=p + 8)):
        assert fused(**bad) == _lib.FMMT_EALIGN, bad
    # the host check of a table
    ok = J.make_table([[3, 1, 4, 0], [4, 4, 4, 4]], [[0.5, 1, 1.5], [1, 1, 1]], [127, 0])
    assert lib.fmmt_jitter_table_check(ok.ctypes.data, 2) == 0
    assert lib.fmmt_jitter_table_check(None, 2) == lib.fmmt_jitter_table_check(ok.ctypes.data, 0) == _lib.FMMT_EINVAL
    for word, value in ((4, 5), (7, -1), (5, 3), (3, 256), (3, -1)):
        t = ok.copy()
        t[0, word] = value
        assert lib.fmmt_jitter_table_check(t.ctypes.data, 2) == _lib.FMMT_EINVAL, (word, value)


def test_front_ends_refuse_cpu_tensors_and_float_frames_with_a_table():
    from facialmmt_amd import _lib, ops
    from facialmmt_amd.augment import ColorJitter
    t = ColorJitter.table([[0, 1, 2, 3]] * 2, [[1, 1, 1]] * 2, [0.0, 0.0])
    with pytest.raises(_lib.FmmtError):
        ops.patch_embed_u8(torch.zeros(2, 112, 112, 3, dtype=torch.uint8), "cv2", torch.float32, jitter=t)       # no CPU or PyTorch fall-back
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as SW

    class _Swin(SW.SwinTransformer):                                     # forward_features' guard alone: no parameters needed
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.pos_drop = torch.nn.Dropout(0.0)
    with pytest.raises(ValueError, match="uint8"):
        _Swin().forward_features(torch.zeros(2, 3, 224, 224), jitter=t)
