"""CPU tests of the Aff-Wild2 training augmentation: the numpy restatement the GPU tests use as their oracle (tests/support_aff_augment.py) held to
Pillow itself and to Pillow's recorded output (tests/golden/aff_augment.npz, written by tests/gen_aff_augment_golden.py), the draws and tables of
facialmmt_amd.augment.AffWildAugment, the noise generator's statistics, and the ABI surface of include/fmmt_aug.h (header == _lib.AUG_SIGNATURES ==
the built library)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import support_aff_augment as A
from tests import support_color_jitter as J
from tests.gen_aff_augment_golden import fixture_frames, fixture_sigmas, fixture_small, fixture_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow():
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        pytest.skip("Pillow is not installed: the restatement is still held to Pillow's recorded output (tests/golden/aff_augment.npz)")


def _frames(S):
    rng = np.random.default_rng(S)
    return rng.integers(0, 256, (S, S, 3), dtype=np.uint8), rng.integers(100, 140, (S, S, 3), dtype=np.uint8)


def test_grayscale_equals_pillow():
    _pillow()
    for S in (224, 17):
        for img in _frames(S):
            assert np.array_equal(A.gray(img), A.pil_gray(img))


@pytest.mark.parametrize("S", [224, 17])
def test_gaussian_blur_equals_pillow(S):
    """sigma 0.1, 1.0, 2.0, the last float32 sigma with box radius 0 and the first with 1, and 30 random sigmas of the reference's range"""
    _pillow()
    sig = fixture_sigmas()
    assert [A.box_weights(s)[0] for s in sig] == [0, 0, 1, 0, 1] and np.float32(sig[3]) < np.float32(sig[4]) == np.nextafter(np.float32(sig[3]), np.float32(2))
    img = _frames(S)[0]
    for s in sig + list(np.random.default_rng(3).uniform(0.1, 2.0, 30)):
        assert np.array_equal(A.gaussian_blur(img, float(s)), A.pil_blur(img, s)), s
    assert A.box_radius(2.0) == 1.375 and max(A.box_weights(s)[0] for s in np.linspace(0.1, 2.0, 200)) == 1


def test_the_stages_composed_in_the_chains_order_equal_pillow():
    _pillow()
    rand, low = _frames(224)
    frames = np.stack([rand, low, rand, low])
    jit = J.make_table([[J.CONTRAST, J.SATURATION, J.NONE, J.HUE], [J.BRIGHTNESS, J.CONTRAST, J.NONE, J.NONE], [J.NONE] * 4, [J.HUE, J.NONE, J.CONTRAST, J.NONE]],
                       [[1, 1.4, 0.6], [0.7, 1.35, 1], [1, 1, 1], [1, 0.62, 1]], [77, 0, 0, 200])
    flags, sigma = [1, 1, 1, 0], [1.9, 0.0, 0.45, 1.2]
    table = A.make_table(flags, jit, sigma)
    got = A.apply_table(frames, table)
    assert np.array_equal(got, A.pil_chain(frames, flags, jit, sigma))
    assert (got[0][..., 0] == got[0][..., 1]).all() and not np.array_equal(got[0], A.gaussian_blur(A.gray(rand), 1.9))     # grey stays grey; contrast moved it
    assert (got[3][..., 0] != got[3][..., 1]).any()
    assert np.array_equal(got[2], A.gaussian_blur(A.gray(rand), 0.45))
    # contrast's mean is the grey frame's
    assert J.contrast_mean(A.gray(low)) == int(A.gray(low)[..., 0].astype(np.float64).mean() + 0.5)


def test_restatement_equals_the_pillow_fixture(golden):
    z = golden.files["aff_augment"]
    assert np.array_equal(z["table"], fixture_table()) and np.array_equal(z["sigmas"], np.array(fixture_sigmas()))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "aff_augment.npz")) < 1 << 19
    got = A.apply_table(fixture_frames(), z["table"])
    assert got.shape == (3, 224, 224, 3) and np.array_equal(got, z["pil_out"]) and not np.array_equal(z["pil_out"], fixture_frames())
    for i, s in enumerate(fixture_sigmas()):
        assert np.array_equal(A.gaussian_blur(fixture_small(), s), z["small_out"][i]), s


# ------------------------------------------------------------------------------------------------ augment.AffWildAugment
N = 20000


def _within(count, p, n=N):
    return abs(count - n * p) <= 4.0 * math.sqrt(n * p * (1 - p)) + 1e-9


def test_draw_on_the_cpu_generator():
    from facialmmt_amd import _lib
    from facialmmt_amd.augment import AffWildAugment
    aug = AffWildAugment()
    torch.manual_seed(5)
    state = torch.get_rng_state()
    t = aug.draw(N, "cpu")
    assert t.shape == (N, 20) and t.dtype == torch.int32 and (t[:, 18:] == 0).all()
    gray, jit, blur, erase = (t[:, 8] & 1) == 1, (t[:, 4:8] != 4).any(1), t[:, 9] >= 0, t[:, 14] > 0
    # 0.5 % of the attempts are rejected and an erase has ten: the erase frequency is erase_p to 1e-23
    for name, got, p in (("gray", gray, 0.8), ("jitter", jit, 0.2), ("blur", blur, 0.5), ("erase", erase, 0.25)):
        assert _within(int(got.sum()), p), (name, int(got.sum()))
    assert ((t[:, 8] & ~1) == 0).all()
    fac = t[:, :3].contiguous().view(torch.float32)
    assert (fac >= 0.6).all() and (fac <= 1.4).all() and (t[:, 3] >= 0).all() and (t[:, 3] <= 255).all()
    assert set(t[:, 3].tolist()) <= set(range(0, 103)) | set(range(154, 256))             # |hue| <= 0.4: shift bytes of +-102
    assert (t[jit][:, 4:8].sort(1).values == torch.arange(4, dtype=torch.int32)).all() and (t[~jit][:, 4:8] == 4).all()
    assert set(t[:, 9].tolist()) == {-1, 0, 1} and (t[~blur][:, 10:12] == 0).all()
    r, ww, fw = t[blur][:, 9].long(), t[blur][:, 10].long(), t[blur][:, 11].long()
    assert (ww > 0).all() and (fw == ((1 << 24) - (2 * r + 1) * ww) // 2).all() and (fw >= 0).all()
    lo, hi = A.box_weights(0.1), A.box_weights(2.0)
    assert int(ww.max()) <= lo[1] and int(ww.min()) >= hi[1]                              # the weights of sigma within [0.1, 2.0]
    top, left, h, w = (t[erase][:, 12 + c] for c in range(4))
    assert (h >= 1).all() and (h < 224).all() and (w >= 1).all() and (w < 224).all() and (top >= 0).all() and (left >= 0).all()
    assert (top + h <= 224).all() and (left + w <= 224).all() and (t[~erase][:, 12:16] == 0).all()
    assert int(h.min()) >= 17 and int(h.max()) > 200 and int((top + h).max()) == 224 and int(top.min()) == 0
    assert len(set(t[:, 16].tolist())) > N - 10 and (t[:, 16] < 0).any() and (t[:, 17] < 0).any()      # 32-bit keys, the sign bit in use
    assert _lib.load().fmmt_aug_table_check(C.c_void_p(t.contiguous().data_ptr()), N) == 0
    torch.set_rng_state(state)
    assert torch.equal(aug.draw(N, "cpu"), t)                                             # the generator is the only state
    assert not torch.equal(aug.draw(N, "cpu"), t)
    # the selected attempt is the first accepted one: a restatement of the selection on the same uniforms (the per-attempt values are rectangles()')
    torch.set_rng_state(state)
    u = torch.rand((N, 45), dtype=torch.float32)
    h, w, top, left, ok = (v.tolist() for v in AffWildAugment.rectangles(u[:, 5:15], u[:, 15:25], u[:, 25:35], u[:, 35:45], (0.02, 1 / 3), 0.3))
    apply, rejected = (u[:, 4] < 0.25).tolist(), 0
    for i in range(N):
        want = [0, 0, 0, 0]
        for a in range(10 if apply[i] else 0):
            assert ok[i][a] == (1 <= h[i][a] < 224 and 1 <= w[i][a] < 224)
            if ok[i][a]:
                want = [top[i][a], left[i][a], h[i][a], w[i][a]]
                break
            rejected += 1
        assert t[i, 12:16].tolist() == want, i
    assert rejected > 0                                                                   # and some first attempts were rejected


def test_probabilities_zero_and_one_and_the_argument_checks():
    from facialmmt_amd.augment import AffWildAugment, ColorJitter
    torch.manual_seed(1)
    t = AffWildAugment(grayscale_p=0, jitter_p=0, blur_p=0, erase_p=0).draw(500, "cpu")
    assert (t[:, 8] == 0).all() and (t[:, 4:8] == 4).all() and (t[:, 9] == -1).all() and (t[:, 10:16] == 0).all()
    t = AffWildAugment(grayscale_p=1, jitter_p=1, blur_p=1, erase_p=1).draw(500, "cpu")
    assert (t[:, 8] == 1).all() and (t[:, 4:8] != 4).all() and (t[:, 9] >= 0).all() and (t[:, 14] > 0).all()
    t = AffWildAugment(jitter_p=1, jitter=ColorJitter(0, 0.3, 0, 0)).draw(50, "cpu")
    assert (t[:, 4:8].sort(1).values == torch.tensor([1, 4, 4, 4], dtype=torch.int32)).all()
    # an area no attempt can fit: nothing is erased
    t = AffWildAugment(erase_p=1, erase_area=(1.0, 1.0), erase_min_aspect=1.0).draw(50, "cpu")
    assert (t[:, 12:16] == 0).all()
    AffWildAugment(sigma=(0.1, 2.44))
    with pytest.raises(ValueError, match="radius"):
        AffWildAugment(sigma=(0.1, 2.45))                                                 # sigma = sqrt(6): box radius 2, beyond the kernel's halo
    for bad in (dict(grayscale_p=1.5), dict(erase_p=-0.1), dict(sigma=(0.0, 1.0)), dict(sigma=(1.0, 0.5)), dict(erase_area=(0.5, 0.2)),
                dict(erase_min_aspect=0.0), dict(erase_attempts=0)):
        with pytest.raises(ValueError):
            AffWildAugment(**bad)
    with pytest.raises(TypeError):
        AffWildAugment(jitter=dict(brightness=0.4))
    assert "utils/util.py" in AffWildAugment.__doc__ and "EFFECTIVE" in AffWildAugment.__doc__


def test_table_from_explicit_values():
    from facialmmt_amd.augment import AffWildAugment, ColorJitter, box_weights
    jit = ColorJitter.table([[3, 1, 4, 0], [4, 4, 4, 4]], [[0.5, 1.0, 1.5], [1, 1, 1]], [0.5, 0.0])
    t = AffWildAugment.table([True, False], jitter=jit, sigma=[1.7, None], rect=[[3, 5, 6, 7], [0, 0, 0, 0]], key=[[1, 0xFFFFFFFF], [7, 8]])
    want = A.make_table([1, 0], jit.numpy(), [1.7, 0], [[3, 5, 6, 7], [0, 0, 0, 0]], [[1, 0xFFFFFFFF], [7, 8]])
    assert t.dtype == torch.int32 and np.array_equal(t.numpy(), want)
    for s in fixture_sigmas() + [0.33, 1.5]:
        assert box_weights(s) == A.box_weights(s)
    for bad in (dict(sigma=[2.6, 0]), dict(rect=[[0, 0, 224, 10], [0, 0, 0, 0]]), dict(rect=[[2, 0, 223, 10], [0, 0, 0, 0]]), dict(rect=[[0, 218, 10, 7], [0, 0, 0, 0]]),
                dict(rect=[[-1, 0, 10, 10], [0, 0, 0, 0]]), dict(rect=[[0, 0, 10, 0], [0, 0, 0, 0]]), dict(sigma=[-1.0, 0]), dict(sigma=[1.0]),
                dict(jitter=torch.tensor([[0, 0, 0, 0, 1, 1, 4, 4], [0, 0, 0, 0, 4, 4, 4, 4]], dtype=torch.int32))):
        with pytest.raises(ValueError):
            AffWildAugment.table([True, False], **bad)
    AffWildAugment.table([False], rect=[[1, 1, 223, 223]])


# ------------------------------------------------------------------------------------------------ the noise generator
def test_noise_statistics_and_key_separation():
    """a 223 x 223 x 3 block under a fixed key: n = 149 187 values"""
    ctr = A.counters()[:, :223, :223].reshape(-1)
    n = ctr.size
    assert n == 149187
    k0, k1 = 0x1234ABCD, 0x0BADF00D
    z = A.noise(ctr, k0, k1)
    assert np.abs(z).max() <= 5.77 and abs(z.mean()) <= 4 / math.sqrt(n) and abs(z.var() - 1) <= 4 * math.sqrt(2 / n)
    for other in ((k0 ^ 1, k1), (k0, k1 ^ (1 << 31)), (k0 ^ (1 << 17), k1)):             # one key bit
        y = A.noise(ctr, *other)
        assert abs(np.corrcoef(z, y)[0, 1]) < 4 / math.sqrt(n), other
    # the key shifted by one against the counter shifted by one: no window of one key's sequence is another key's
    h1, h2 = A.noise_words(ctr, k0, k1)
    for dk0, dk1 in ((1, 0), (0, 1), (1, 1), (-1, 0), (0, -1), (-1, -1)):
        for dc in (1, -1):
            g1, g2 = A.noise_words(ctr + dc, k0 + dk0, k1 + dk1)
            assert (g1 == h1).sum() <= 2 and (g2 == h2).sum() <= 2, (dk0, dk1, dc)       # chance: n / 2^32
        for x in (1, 2, 224):
            g1, g2 = A.noise_words(ctr ^ x, k0 ^ (x if dk0 else 0), k1 ^ (x if dk1 else 0))
            assert (g1 == h1).sum() <= 2 and (g2 == h2).sum() <= 2, (dk0, dk1, x)
    assert (h1 == h2).sum() <= 2
    # the two words of one element are not each other's neighbours either, and u1 never reaches 0
    assert len(np.unique(h1)) > n - 10 and len(np.unique(h2)) > n - 10


# ------------------------------------------------------------------------------------------------ ABI surface
def _lib_built():
    from facialmmt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_aug_header_signatures_and_library_agree():
    """include/fmmt_aug.h (included by fmmt.h) == _lib.AUG_SIGNATURES == the symbols of the built library, as tests/test_color_jitter_cpu.py does for
    its header; the table is disjoint from the nine that exist"""
    from facialmmt_amd import _lib, build
    assert "aff_augment.hip" in build.SOURCES and "color_jitter.hip" in build.SOURCES
    assert '#include "fmmt_aug.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    assert os.path.exists(os.path.join(ROOT, "facialmmt_amd", "csrc", "jitter_core.h"))
    raw = open(os.path.join(ROOT, "include", "fmmt_aug.h")).read()
    assert "utils/util.py:22-60" in raw and "mix32a" in raw
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {m.group(1): (m.group(0).split()[0], m.group(2)) for m in re.finditer(r"\b\w+\s+(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.AUG_SIGNATURES) == ["fmmt_aug_table_check", "fmmt_aug_workspace_bytes", "fmmt_patch_embed_u8_aug",
                                                             "fmmt_patch_embed_u8_aug_ln_fwd"]
    for other in (_lib.SIGNATURES, _lib.POOL_HEAD_SIGNATURES, _lib.RAGGED_SIGNATURES, _lib.EVAL_COLLECT_SIGNATURES, _lib.POOL_HEAD_ROWS_SIGNATURES,
                  _lib.GUARD_SIGNATURES, _lib.DIGEST_SIGNATURES, _lib.EVAL_SHARD_SIGNATURES, _lib.JITTER_SIGNATURES):
        assert not set(_lib.AUG_SIGNATURES) & set(other)
    base = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        return base[" ".join(decl.replace("const", " ").split()[:-1])]                   # drop the parameter's name
    for name, (ret, args) in protos.items():
        res, got = _lib.AUG_SIGNATURES[name]
        assert got == [ctype_of(a) for a in args.split(",") if a.strip()], name
        assert res is base[ret], name
    # the jitter pair with the byte workspace and its size put in behind `partial`
    for new, old in (("fmmt_patch_embed_u8_aug", "fmmt_patch_embed_u8_jitter"), ("fmmt_patch_embed_u8_aug_ln_fwd", "fmmt_patch_embed_u8_jitter_ln_fwd")):
        a = list(_lib.AUG_SIGNATURES[new][1])
        assert a[9:11] == [C.c_void_p, C.c_size_t] and a[:9] + a[11:] == _lib.JITTER_SIGNATURES[old][1]
    defines = dict(re.findall(r"#define\s+(FMMT_AUG_\w+)\s+(\d+)", src))
    assert {k: int(v) for k, v in defines.items()} == dict(FMMT_AUG_WORDS=_lib.AUG_WORDS, FMMT_AUG_FLAG_GRAY=_lib.AUG_FLAG_GRAY,
                                                           FMMT_AUG_MAX_RADIUS=_lib.AUG_MAX_RADIUS, FMMT_AUG_HALO=_lib.AUG_HALO)
    assert (_lib.AUG_WORDS, _lib.AUG_FLAG_GRAY, _lib.AUG_MAX_RADIUS, _lib.AUG_HALO) == (A.WORDS, A.FLAG_GRAY, A.MAX_RADIUS, A.HALO) == (20, 1, 1, 6)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in _lib.AUG_SIGNATURES) and "fmmt_aug.h" in text and "augment=" in text
    lib = _lib_built()
    assert all(hasattr(lib, name) for name in _lib.AUG_SIGNATURES)
    assert lib.fmmt_aug_workspace_bytes(3) == 3 * 224 * 224 * 3 and lib.fmmt_aug_workspace_bytes(0) == 0


def test_arguments_are_validated_before_any_launch():
    from facialmmt_amd import _lib
    lib = _lib_built()
    buf = (C.c_char * 512)()
    p = C.addressof(buf)
    p += -p % 16
    big = 2 * 224 * 224 * 3

    def plain(dtype=1, mode=0, n=2, S=160, img=p, tab=p, lut=p, aug=p, partial=p, ws=p, nbytes=big, cols=p):
        return lib.fmmt_patch_embed_u8_aug(dtype, mode, n, S, img, tab, lut, aug, partial, ws, nbytes, cols, None)
    for bad in (dict(dtype=2), dict(mode=2), dict(n=0), dict(n=65536), dict(S=3), dict(S=225), dict(img=None), dict(tab=None), dict(lut=None), dict(aug=None),
                dict(partial=None), dict(ws=None), dict(cols=None)):
        assert plain(**bad) == _lib.FMMT_EINVAL, bad
    for bad in (dict(nbytes=big - 1), dict(nbytes=0)):
        assert plain(**bad) == _lib.FMMT_EWORKSPACE, bad
    for bad in (dict(tab=p + 4), dict(cols=p + 8), dict(aug=p + 2), dict(partial=p + 1), dict(ws=p + 4)):
        assert plain(**bad) == _lib.FMMT_EALIGN, bad

    def fused(dtype=1, mode=0, n=2, S=160, aug=p, partial=p, ws=p, nbytes=big, w=p, y=p, mean=p, rstd=p, cols=None):
        return lib.fmmt_patch_embed_u8_aug_ln_fwd(dtype, mode, n, S, p, p, p, aug, partial, ws, nbytes, w, None, p, p, 1e-5, cols, None, y, mean, rstd, None)
    for bad in (dict(dtype=3), dict(mode=-1), dict(n=0), dict(S=300), dict(aug=None), dict(partial=None), dict(ws=None), dict(w=None), dict(y=None), dict(mean=None)):
        assert fused(**bad) == _lib.FMMT_EINVAL, bad
    assert fused(nbytes=big - 1) == _lib.FMMT_EWORKSPACE
    for bad in (dict(aug=p + 2), dict(partial=p + 3), dict(ws=p + 8), dict(w=p + 8), dict(cols=p + 8)):
        assert fused(**bad) == _lib.FMMT_EALIGN, bad
    # the host check of a table
    jit = J.make_table([[3, 1, 4, 0], [4, 4, 4, 4]], [[0.5, 1, 1.5], [1, 1, 1]], [127, 0])
    ok = A.make_table([1, 0], jit, [1.7, 0.4], [[207, 207, 17, 17], [0, 0, 0, 0]], [[5, 6], [7, 8]])
    assert lib.fmmt_aug_table_check(ok.ctypes.data, 2) == 0
    assert lib.fmmt_aug_table_check(None, 2) == lib.fmmt_aug_table_check(ok.ctypes.data, 0) == _lib.FMMT_EINVAL
    r, ww, fw = A.box_weights(1.7)
    for word, value in ((4, 5), (5, 3), (3, 256),                                         # what fmmt_jitter_table_check refuses
                        (8, 2), (8, 3), (9, 2), (9, -2), (10, ww + 1), (11, fw + 1), (10, 0), (10, -5),
                        (14, 224), (15, 224), (14, 18), (15, 18), (12, -1), (13, 208), (14, -3), (15, 0), (18, 1), (19, -1)):
        t = ok.copy()
        t[0, word] = value
        assert lib.fmmt_aug_table_check(t.ctypes.data, 2) == _lib.FMMT_EINVAL, (word, value)
    t = ok.copy()
    t[1, 9:12] = (2, (1 << 24) // 5, 0)                                                   # weights that sum to 1 << 24 with r = 2: the radius is refused
    assert lib.fmmt_aug_table_check(t.ctypes.data, 2) == _lib.FMMT_EINVAL
    t = ok.copy()
    t[0, 12:16] = (1, 1, 223, 223)
    assert lib.fmmt_aug_table_check(t.ctypes.data, 2) == 0


def test_front_ends_refuse_bad_arguments():
    from facialmmt_amd import _lib, ops
    from facialmmt_amd.augment import AffWildAugment, ColorJitter
    from facialmmt_amd.train_step import AuxStep, GraphedAuxStep
    t = AffWildAugment.table([True, False])
    x = torch.zeros(2, 112, 112, 3, dtype=torch.uint8)
    with pytest.raises(_lib.FmmtError):
        ops.patch_embed_u8(x, "pil", torch.float32, augment=t)                            # no CPU or PyTorch fall-back
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as SW

    class _Swin(SW.SwinTransformer):                                                      # forward_features' guards alone: no parameters needed
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.pos_drop = torch.nn.Dropout(0.0)
    with pytest.raises(ValueError, match="uint8"):
        _Swin().forward_features(torch.zeros(2, 3, 224, 224), augment=t)
    jit = ColorJitter.table([[0, 1, 2, 3]] * 2, [[1, 1, 1]] * 2, [0.0, 0.0])
    with pytest.raises(ValueError, match="exclude"):
        _Swin().forward_features(x, jitter=jit, augment=t)
    with pytest.raises(ValueError, match="exclude"):
        ops._augment_table(t, jit, x, "patch_embed_u8")
    for bad in (t[:1], t[:, :8], t.float(), t.view(-1), [[0] * 20] * 2):
        with pytest.raises(ValueError):
            ops._augment_table(bad, None, x, "patch_embed_u8")
    with pytest.raises(TypeError):
        AuxStep(None, None, None, None, augment=ColorJitter())
    with pytest.raises(TypeError):
        GraphedAuxStep(None, None, None, None, x, torch.zeros(2, dtype=torch.long), augment=dict(blur_p=0.5))
    with pytest.raises(ValueError, match="uint8"):
        GraphedAuxStep(None, None, None, None, torch.zeros(2, 3, 224, 224), torch.zeros(2, dtype=torch.long), augment=AffWildAugment())
    step = AuxStep(None, None, None, None, augment=AffWildAugment())
    with pytest.raises(ValueError, match="uint8"):
        step(torch.zeros(2, 3, 224, 224), torch.zeros(2, dtype=torch.long))
    assert step.last_augment is None
