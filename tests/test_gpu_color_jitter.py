"""GPU tests of the MELD training ColorJitter inside the uint8 pre-step (csrc/color_jitter.hip, include/fmmt_jitter.h): integer and exactly rounded
work, so everything is BIT-EXACT -- against the numpy restatement (tests/support_color_jitter.py, itself held to Pillow by tests/test_color_jitter_cpu.py)
applied to the oracle's resize, against Pillow's recorded output (tests/golden/color_jitter.npz), against the plain pre-step where the table says
"none", and between the fused and the two-launch form."""
import numpy as np
import pytest
import torch

from facialmmt_amd import ops, synth
from facialmmt_amd.augment import ColorJitter
from oracle import preproc as P
from tests import support_color_jitter as J
from tests.gen_color_jitter_golden import fixture_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _crops(name, n, S, seed):
    return synth.randint(name, (n, S, S, 3), 0, 256, seed=seed).astype(np.uint8)


def _want(jittered_224):
    """(n, 224, 224, 3) uint8 -> the patch matrix of Normalize(ToTensor(.))"""
    return P.patch_cols(np.ascontiguousarray(P.normalize_lut()[jittered_224].transpose(0, 3, 1, 2)))


# every operation first, in the middle and last; hue shifts 0, 1, 127, 128, 255; factors 0.5, 1.0, 1.5
ORDERS = [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [2, 0, 3, 1], [1, 0, 2, 3], [3, 1, 2, 0], [2, 1, 3, 0], [0, 3, 1, 2]]
FACTORS = [[0.5, 0.5, 0.5], [1.5, 1.5, 1.5], [1.0, 1.5, 0.5], [1.5, 0.5, 1.0], [1.5, 1.5, 0.5], [0.5, 1.5, 1.5], [1.0, 1.0, 1.0], [0.73, 1.31, 1.18]]
SHIFTS = [1, 127, 128, 255, 0, 128, 0, 201]


def _case_frames(S, seed):
    img = _crops("jitter_gpu", 8, S, seed)
    img[0, :3] = 255                                          # saturated and black borders: the resize's overshoot must clip in front of the jitter
    img[0, -3:] = 0
    img[2] = (100 + img[2] % 40).astype(np.uint8)             # low contrast: the blends clip on neither side, the mean decides
    img[3] = 0                                                # all black
    img[4] = 255                                              # all 255
    img[5] = img[5][..., :1]                                  # grey: max == min everywhere
    return img


@pytest.mark.parametrize("mode", ["pil", "cv2"])
@pytest.mark.parametrize("S", [224, 160, 57])
def test_jittered_patch_matrix_bit_exact(dev, mode, S):
    img = _case_frames(S, seed=S + (3 if mode == "pil" else 5))
    table = J.make_table(ORDERS, FACTORS, SHIFTS)
    resized = P.resize_u8(img, mode)
    if S == 224:
        assert np.array_equal(resized, img)                   # the resize is the identity: the jitter alone
    want = _want(J.apply_table(resized, table))
    x, t = torch.from_numpy(img).to(dev), torch.from_numpy(table).to(dev)
    got = ops.patch_embed_u8(x, mode, torch.float32, jitter=t)
    assert got.shape == (8 * 3136, 48)
    bad = np.flatnonzero((got.cpu().numpy() != want).any(1))
    assert bad.size == 0, f"frames {sorted(set((bad // 3136).tolist()))} differ, first patch row {bad[0]}"
    got16 = ops.patch_embed_u8(x, mode, torch.bfloat16, jitter=t)
    assert torch.equal(got16.cpu(), torch.from_numpy(want).bfloat16())
    assert not np.array_equal(want, P.patch_cols_from_u8(img, mode))


def test_hue_round_trip_on_a_sweep_of_colours(dev):
    """600 000 colours spread over the 2^24 (every 27th, 12 frames), hue alone with three shifts: the float / double mix of the two HSV conversions"""
    a = (np.arange(12 * 224 * 224, dtype=np.int64) * 27 + 11) & 0xFFFFFF
    img = np.stack([a >> 16, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(12, 224, 224, 3)
    for shift in (0, 77, 255):
        table = J.make_table([[4, 3, 4, 4]] * 12, [[1, 1, 1]] * 12, [shift] * 12)
        got = ops.patch_embed_u8(torch.from_numpy(img).to(dev), "cv2", torch.float32, jitter=torch.from_numpy(table).to(dev))
        assert np.array_equal(got.cpu().numpy(), _want(J.hue(img, shift))), shift


@pytest.mark.parametrize("mode", ["pil", "cv2"])
def test_against_the_pillow_fixture(golden, dev, mode):
    z = golden.files["color_jitter"]
    x, t = torch.from_numpy(fixture_frames()).to(dev), torch.from_numpy(z["table"]).to(dev)
    got = ops.patch_embed_u8(x, mode, torch.float32, jitter=t)            # S = 224: both resizes are the identity
    assert np.array_equal(got.cpu().numpy(), _want(z["pil_out"]))          # Pillow's own bytes


def _patch_embed(dev):
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as SW
    pe = SW.PatchEmbed(224, 4, 3, 96, torch.nn.LayerNorm)
    synth.fill_state_dict(pe, seed=31, prefix="pe.")
    return pe.to(dev)


@pytest.mark.parametrize("mode,S,dtype", [("cv2", 160, torch.bfloat16), ("pil", 57, torch.float32)])
def test_a_table_of_none_gives_the_plain_pre_step(dev, mode, S, dtype):
    x = torch.from_numpy(_crops("jitter_none", 3, S, seed=S)).to(dev)
    none = ColorJitter.table([[4, 4, 4, 4]] * 3, [[0.5, 1.5, 0.7]] * 3, [0.3] * 3, device=dev)        # factors and shift without an operation: unused
    assert torch.equal(ops.patch_embed_u8(x, mode, dtype, jitter=none), ops.patch_embed_u8(x, mode, dtype))
    pe = _patch_embed(dev)
    with torch.no_grad():
        assert torch.equal(pe.forward_u8(x, mode, dtype, jitter=none), pe.forward_u8(x, mode, dtype))
    drawn = ColorJitter(0, None, 0, 0).draw(3, dev)                       # every amount off: what draw() emits is such a table
    assert (drawn[:, 4:] == 4).all() and torch.equal(ops.patch_embed_u8(x, mode, dtype, jitter=drawn), ops.patch_embed_u8(x, mode, dtype))


@pytest.mark.parametrize("mode,S,dtype", [("cv2", 160, torch.bfloat16), ("pil", 57, torch.float32), ("cv2", 224, torch.float32)])
def test_fused_form_equals_two_launches_on_the_same_table(dev, monkeypatch, mode, S, dtype):
    """fmmt_patch_embed_u8_jitter_ln_fwd against fmmt_patch_embed_u8_jitter + fmmt_patch_embed_ln_fwd: cols, y, x_pre, mean, rstd bit for bit; the
    module's forward and parameter gradients the same through either"""
    from facialmmt_amd import _lib
    lib = _lib.load()
    img = _case_frames(S, seed=S + 9)[:3]
    x = torch.from_numpy(img).to(dev)
    t = torch.from_numpy(J.make_table(ORDERS[:3], FACTORS[:3], SHIFTS[:3])).to(dev)
    pe = _patch_embed(dev)
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "_PATCH_U8_LN", fused)
        y = pe.forward_u8(x, mode, dtype, jitter=t)
        w = torch.randn(y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(9)).to(dtype)
        outs.append((y.detach(), torch.autograd.grad(y, list(pe.parameters()), w)))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)
    with torch.no_grad():
        assert not torch.equal(pe.forward_u8(x, mode, dtype), outs[0][0])                     # and the table did something
    # the raw entry points
    code, tab, lut = ops.resize_tables(mode, S, dev)
    M, dt = 3 * 3136, (_lib.BF16 if dtype == torch.bfloat16 else _lib.F32)
    w2d = pe.proj.weight.detach().view(96, 48).to(dtype).contiguous()
    bias, g, b = pe.proj.bias.detach().float(), pe.norm.weight.detach().float(), pe.norm.bias.detach().float()
    st = torch.cuda.current_stream().cuda_stream
    partial = torch.empty(3, 56, dtype=torch.int32, device=dev)
    f = dict(cols=torch.empty(M, 48, dtype=dtype, device=dev), x_pre=torch.empty(M, 96, dtype=dtype, device=dev), y=torch.empty(M, 96, dtype=dtype, device=dev),
             mean=torch.empty(M, device=dev), rstd=torch.empty(M, device=dev))
    rc = lib.fmmt_patch_embed_u8_jitter_ln_fwd(dt, code, 3, S, x.data_ptr(), tab.data_ptr(), lut.data_ptr(), t.data_ptr(), partial.data_ptr(), w2d.data_ptr(),
                                               bias.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-5, f["cols"].data_ptr(), f["x_pre"].data_ptr(), f["y"].data_ptr(),
                                               f["mean"].data_ptr(), f["rstd"].data_ptr(), st)
    assert rc == 0
    two = dict(cols=ops.patch_embed_u8(x, mode, dtype, jitter=t), x_pre=torch.empty(M, 96, dtype=dtype, device=dev), y=torch.empty(M, 96, dtype=dtype, device=dev),
               mean=torch.empty(M, device=dev), rstd=torch.empty(M, device=dev))
    rc = lib.fmmt_patch_embed_ln_fwd(dt, M, 96, 48, two["cols"].data_ptr(), w2d.data_ptr(), bias.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-5,
                                     two["x_pre"].data_ptr(), two["y"].data_ptr(), two["mean"].data_ptr(), two["rstd"].data_ptr(), st)
    assert rc == 0
    for k in f:
        assert torch.equal(f[k], two[k]), k
    assert torch.equal(f["y"].view_as(outs[0][0]), outs[0][0])
    want = torch.from_numpy(_want(J.apply_table(P.resize_u8(img, mode), t.cpu().numpy())))
    assert torch.equal(f["cols"].cpu(), want.to(dtype))
    # inference: no patch matrix, the same y
    y2 = torch.empty_like(f["y"])
    rc = lib.fmmt_patch_embed_u8_jitter_ln_fwd(dt, code, 3, S, x.data_ptr(), tab.data_ptr(), lut.data_ptr(), t.data_ptr(), partial.data_ptr(), w2d.data_ptr(),
                                               bias.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-5, None, None, y2.data_ptr(), None, None, st)
    assert rc == 0 and torch.equal(y2, f["y"])


def test_frames_with_different_orders_do_not_disturb_each_other(dev):
    """one launch, eight records: each frame's rows are what the frame gives alone, and permuting frames together with their records permutes the rows"""
    S = 160
    x = torch.from_numpy(_case_frames(S, seed=77)).to(dev)
    t = torch.from_numpy(J.make_table(ORDERS, FACTORS, SHIFTS)).to(dev)
    full = ops.patch_embed_u8(x, "cv2", torch.bfloat16, jitter=t).view(8, 3136, 48)
    for i in (0, 2, 7):
        assert torch.equal(ops.patch_embed_u8(x[i:i + 1], "cv2", torch.bfloat16, jitter=t[i:i + 1]).view(3136, 48), full[i]), i
    perm = torch.tensor([5, 0, 7, 2, 1, 6, 3, 4], device=dev)
    assert torch.equal(ops.patch_embed_u8(x[perm], "cv2", torch.bfloat16, jitter=t[perm]).view(8, 3136, 48), full[perm])
    assert not torch.equal(ops.patch_embed_u8(x, "cv2", torch.bfloat16, jitter=t[perm]).view(8, 3136, 48), full)      # the records belong to their frames


def test_torch_op_and_swin_forward_take_the_table(dev):
    import os
    from facialmmt_amd import torch_ops  # noqa: F401
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as SW
    from facialmmt_amd.modules.SwinTransformer.backbone_def import BackboneFactory
    img = _crops("jitter_swin", 3, 112, seed=5)
    x = torch.from_numpy(img).to(dev)
    t = ColorJitter.table(ORDERS[:3], FACTORS[:3], [0.2, -0.4, 0.0], device=dev)
    assert torch.equal(torch.ops.fmmt.patch_embed_u8_jitter(x, "cv2", True, t), ops.patch_embed_u8(x, "cv2", torch.bfloat16, jitter=t))
    torch.library.opcheck(torch.ops.fmmt.patch_embed_u8_jitter.default, (x, "pil", True, t), test_utils=("test_schema", "test_faketensor"))
    m = BackboneFactory("SwinTransformer", os.path.join(os.path.dirname(SW.__file__), "swin_conf.yaml")).get_backbone()
    synth.fill_state_dict(m, seed=100)
    m.to(dev).eval()
    m.input_resize = "cv2"
    jittered = J.apply_table(P.resize_u8(img, "cv2"), t.cpu().numpy())
    frames = torch.from_numpy(np.ascontiguousarray(P.normalize_lut()[jittered].transpose(0, 3, 1, 2))).to(dev)
    with torch.no_grad():
        a, b, plain = m(x, jitter=t), m(frames), m(x)
        one = m(x[:1], jitter=t[:1])                                       # the single-frame path duplicates the record with the frame
    assert torch.equal(a, b) and not torch.equal(a, plain) and one.shape == (1, a.shape[1])


def test_errors(dev):
    x = torch.zeros(3, 112, 112, 3, dtype=torch.uint8, device=dev)
    good = ColorJitter.table([[0, 1, 2, 3]] * 3, [[1, 1, 1]] * 3, [0.0] * 3, device=dev)
    for bad in (good[:2], good[:, :7], good.float(), good.long(), good.view(-1), good.cpu(), [[0] * 8] * 3):
        with pytest.raises(ValueError):
            ops.patch_embed_u8(x, "cv2", torch.bfloat16, jitter=bad)
    pe = _patch_embed(dev)
    with pytest.raises(ValueError):
        pe.forward_u8(x, "cv2", torch.bfloat16, jitter=good[:2])
    import os
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as SW
    from facialmmt_amd.modules.SwinTransformer.backbone_def import BackboneFactory
    m = BackboneFactory("SwinTransformer", os.path.join(os.path.dirname(SW.__file__), "swin_conf.yaml")).get_backbone().to(dev)
    with pytest.raises(ValueError, match="uint8"):
        m(torch.zeros(3, 3, 224, 224, device=dev), jitter=good)           # a table with float frames
