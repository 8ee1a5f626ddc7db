"""The references of tests/support_unimodal_oracle.py have to be trusted before they judge the HIP code (tests/test_gpu_pool_head.py,
tests/test_gpu_unimodal_step.py): the fp64 V-only step against central finite differences, its accumulation loop against the single-step
gradients, and the hand-written head (forward and backward formulas) against autograd through oracle.multimodal.additive_attention.  CPU only."""
import pytest
import torch

from facialmmt_amd import synth
from facialmmt_amd.config import default_args

from tests import support_unimodal_oracle as UO

B, L = 3, 6


def _cfg(**kw):
    return default_args(get_vision_utt_max_lens=L, trg_accumulation_steps=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **kw)


def _batch(seed=3):
    dd = torch.float64
    x = synth.tensor("vfeat", (B, L, 512), seed=seed, dtype=dd)
    mask = torch.ones(B, L, dtype=dd)
    mask[1, 4:] = 0
    mask[2, 1:] = 0                                          # a row with exactly one valid token
    labels = torch.from_numpy(synth.randint("labels", (B,), 0, 7, seed=seed + 1))
    return x, mask, labels


def _leaves(cfg, seed=201):
    from facialmmt_amd import models
    m = models.meld_utt_transformer(cfg)
    synth.fill_state_dict(m, seed=seed)
    return UO.leaves(m, torch.float64)


@pytest.fixture(scope="module")
def point():
    cfg = _cfg()
    sd = _leaves(cfg)
    batch = _batch()
    lv = UO.trainable(sd)
    loss = UO.step_loss(sd, cfg, *batch)
    grads = dict(zip(lv, torch.autograd.grad(loss, list(lv.values()), allow_unused=True)))
    assert torch.isfinite(loss) and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    return dict(cfg=cfg, sd=sd, batch=batch, grads=grads)


def _directional(point, seed, h):
    """(<grad, dir>, the central difference at h and at h / 2) for one seeded direction over all leaves: every tensor moves along N(0,1) noise
    times its own largest magnitude, so h is a relative step"""
    lv = UO.trainable(point["sd"])
    g = torch.Generator().manual_seed(seed)
    dirs = {k: torch.randn(v.shape, dtype=torch.float64, generator=g) * float(v.detach().abs().max()) for k, v in lv.items()}
    slope = sum(float((point["grads"][k] * dirs[k]).sum()) for k in lv)
    base = {k: v.detach().clone() for k, v in lv.items()}

    def loss_at(eps):
        with torch.no_grad():
            for k, v in lv.items():
                v.copy_(base[k] + eps * dirs[k])
            return float(UO.step_loss(point["sd"], point["cfg"], *point["batch"]))
    try:
        fds = [(loss_at(e) - loss_at(-e)) / (2 * e) for e in (h, h / 2)]
    finally:
        with torch.no_grad():
            for k, v in lv.items():
                v.copy_(base[k])
    return slope, fds[0], fds[1]


def test_step_reference_gradients_match_finite_differences(point):
    """16 seeded directions over every parameter of the model.  The central differences at h and h / 2 are combined by Richardson's rule
    ((4 fd(h/2) - fd(h)) / 3: the h^2 term of the truncation error cancels, the remainder is O(h^4)); the result agrees with <grad, dir> to 1e-8
    of the slope.  h = 1e-4 of each tensor's magnitude: rounding (2e-16 |loss| / h ~ 1e-11) and the h^4 term both stay orders below the bar."""
    h = 1e-4
    worst = 0.0
    for seed in range(16):
        slope, f1, f2 = _directional(point, 2000 + seed, h)
        fd = (4.0 * f2 - f1) / 3.0
        err = abs(fd - slope)
        print(f"direction {seed}: <grad,dir> {slope:+.12e}  fd {fd:+.12e}  |fd - slope| / |slope| {err / abs(slope):.3e}  (h^2 term {abs(f1 - f2):.3e})")
        assert slope != 0.0
        worst = max(worst, err / abs(slope))
    assert worst <= 1e-8, worst


def test_accumulation_over_the_same_micro_batch_twice_gives_the_single_step_gradients():
    cfg = _cfg()
    sd = _leaves(cfg)
    batch = _batch()
    start = {k: v.detach().clone() for k, v in UO.trainable(sd).items()}
    cfg.clip = 1e9
    one = UO.run(sd, cfg, [batch], lr=0.05, keep_grads=True)
    after_one = {k: v.detach().clone() for k, v in UO.trainable(sd).items()}
    with torch.no_grad():
        for k, v in UO.trainable(sd).items():
            v.copy_(start[k])
    cfg.trg_accumulation_steps = 2
    two = UO.run(sd, cfg, [batch, batch], lr=0.05, keep_grads=True)
    assert len(one["steps"]) == 1 and len(two["steps"]) == 1 and len(two["micro"]) == 2
    assert abs(two["micro"][0]["loss"] * 2 - one["micro"][0]["loss"]) <= 1e-13 * abs(one["micro"][0]["loss"])
    assert abs(two["steps"][0]["norm"] - one["steps"][0]["norm"]) <= 1e-12 * one["steps"][0]["norm"]
    g1, g2 = one["steps"][0]["grads"], two["steps"][0]["grads"]
    assert not one["micro"][0]["unused"]
    for k in g1:
        assert float((g1[k] - g2[k]).norm()) <= 1e-12 * float(g1[k].norm()), k
        assert torch.allclose(after_one[k], start[k] - 0.05 * g1[k], rtol=0, atol=1e-14 * max(1.0, float(start[k].abs().max()))), k
        assert float((sd[k].detach() - after_one[k]).abs().max()) <= 1e-12 * max(1.0, float(after_one[k].abs().max())), k


def test_clip_scales_the_update():
    """a clip below the total norm: the parameters move by -lr * clip / (norm + 1e-6) * gradient (train.py:260-261 with SGD)"""
    cfg = _cfg()
    sd = _leaves(cfg)
    start = {k: v.detach().clone() for k, v in UO.trainable(sd).items()}
    cfg.clip = 1e9
    free = UO.run(_leaves(cfg), cfg, [_batch()], lr=0.05, keep_grads=True)
    norm = free["steps"][0]["norm"]
    cfg.clip = 0.5 * norm
    got = UO.run(sd, cfg, [_batch()], lr=0.05)
    assert abs(got["steps"][0]["norm"] - norm) <= 1e-12 * norm
    coef = cfg.clip / (norm + 1e-6)
    for k, g in free["steps"][0]["grads"].items():
        want = start[k] - 0.05 * coef * g
        assert float((sd[k].detach() - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), k


@pytest.mark.parametrize("shape", [(3, 7, 64), (4, 12, 96), (2, 2, 64)])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_head_formulas_match_autograd(shape, p):
    """the hand-written head of support_unimodal_oracle.head_reference -- what the GPU op is compared with -- against autograd of
    oracle.multimodal.additive_attention + classifier + cross-entropy, with a given keep mask and an upstream gradient != 1: every
    output and gradient to 1e-10 of the tensor's largest magnitude.  d(v_b) is identically zero (softmax shift invariance): it is held
    to 1e-10 of sum |d(score_t)|."""
    Bh, Lh, H = shape
    inp, lengths = UO.head_inputs(Bh, Lh, H, 7, seed=40)
    assert lengths[0] == Lh and (Bh == 1 or lengths[-1] == 1)
    g = torch.Generator().manual_seed(5)
    keep = ((torch.rand(Bh, H, generator=g) >= p).double() / (1.0 - p)) if p > 0 else torch.ones(Bh, H, dtype=torch.float64)
    ref = UO.head_reference(**inp, keep=keep, dloss=0.37)
    auto = UO.head_autograd(**inp, keep=keep, dloss=0.37)
    for k in ("loss", "logits", "alpha", "dh", "dph", "dqq", "dv", "dW", "db"):
        scale = float(auto[k].abs().max())
        err = float((ref[k] - auto[k]).abs().max())
        print(f"{shape} p={p} {k}: max|hand - autograd| {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 1e-10 * scale, (k, err, scale)
    cancel = float(ref["dscore"].abs().sum())
    assert float(ref["dvb"].abs()) <= 1e-10 * cancel and float(auto["dvb"].abs().max()) <= 1e-10 * cancel
    assert float(ref["alpha"][-1, 1:].abs().max()) == 0.0 or Bh == 1      # the one-token row: all weight on token 0


def test_pool_head_header_signatures_and_library_agree():
    """include/fmmt_pool_head.h (included by fmmt.h) == _lib.POOL_HEAD_SIGNATURES == the symbols of the built library, as tests/test_host_cpu.py checks
    fmmt.h against _lib.SIGNATURES; argument validation happens before any launch, so it runs without a GPU"""
    import os
    import re
    from facialmmt_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "pool_head.hip" in build.SOURCES
    assert '#include "fmmt_pool_head.h"' in open(os.path.join(root, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fmmt_pool_head.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.POOL_HEAD_SIGNATURES) == ["fmmt_pool_head_bwd", "fmmt_pool_head_bwd_workspace", "fmmt_pool_head_fwd"]
    assert not set(_lib.POOL_HEAD_SIGNATURES) & set(_lib.SIGNATURES)
    import ctypes as C

    def ctype_of(decl):
        """the ctypes type of one C parameter declaration of the header"""
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    returns = {m.group(2): m.group(1) for m in re.finditer(r"\b(int|size_t)\s+(fmmt_\w+)\s*\(", src)}
    for name, args in protos.items():                         # argument by argument, and the return type
        want = [ctype_of(a) for a in args.split(",") if a.strip()]
        res, got = _lib.POOL_HEAD_SIGNATURES[name]
        assert got == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g is not w], len(got), len(want))
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[returns[name]], name
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    assert all(name in text for name in protos)
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in protos)
    assert lib.fmmt_pool_head_bwd_workspace(4, 1, 768) == 0 and lib.fmmt_pool_head_bwd_workspace(4, 160, 768) >= 4 * 20 * (2 * 768 + 1) * 4
    none9, none7, none19 = [None] * 9, [None] * 7, [None] * 19
    for bad in ((0, 4, 1, 768, 7), (0, 4, 160, 12, 7), (0, 4, 160, 768, 9), (0, 1025, 160, 768, 7), (5, 4, 160, 768, 7)):
        assert lib.fmmt_pool_head_fwd(*bad, *none9, 0.0, 0, *none7, 0, None) == _lib.FMMT_EINVAL, bad
        assert lib.fmmt_pool_head_bwd(*bad, *none19, 0, None) == _lib.FMMT_EINVAL, bad
