"""The step reference of tests/support_step_oracle.py has to be trusted before it judges the HIP steps (tests/test_gpu_step_oracle.py):
its autograd gradients against central finite differences in fp64 (through the slice assignments of select_frames_loop and
slice_target_utterance_loop, train-mode BatchNorm, the Gumbel-softmax), its composition against a hand-assembled loss, and its
accumulation loop against the single-step gradients.  CPU only; 2 utterances of 4 and 3 frames keep it to a couple of minutes."""
import pytest
import torch

from facialmmt_amd import synth
from facialmmt_amd.config import default_args

from tests import support_step_oracle as SO

B, LV, T = 2, 4, 128
NUM_IMGS = (4, 3)
THRESHOLD = 0.3          # between the importances of the seeded draw below: frames are kept and dropped (asserted)
SMOOTH_MARGIN = 1e-3      # no importance closer to the threshold than this: the loss is smooth around the point


def _cfg(**kw):
    return default_args(get_vision_utt_max_lens=LV, get_audio_utt_max_lens=24, trg_accumulation_steps=1, plm_module=synth.make_standin_plm(),
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, crossmodal_attn_dropout_TA=0.0, crossmodal_attn_dropout_TA_V=0.0,
                        FacialEmoImpor_threshold=THRESHOLD, **kw)


def _batch(cfg, n_utt=B):
    """hash-seeded MELD-shaped inputs in fp64, ragged: utterance 1 has one padded vision row"""
    num = list(NUM_IMGS[:n_utt])
    nF = sum(num)
    dd = torch.float64
    ids = torch.from_numpy(synth.randint("ids", (n_utt, T), 3, 1000, seed=1))
    attn = torch.zeros(n_utt, T, dtype=dd)
    attn[:, :100] = 1
    sep = torch.zeros(n_utt, T, dtype=dd)
    sep[:, 20:100:20] = 1
    utt_idx = torch.arange(n_utt) % 8
    audio = synth.tensor("audio", (n_utt, cfg.get_audio_utt_max_lens, cfg.audio_featExtr_dim), seed=2, dtype=dd)
    amask = torch.zeros(n_utt, cfg.get_audio_utt_max_lens, dtype=dd)
    amask[:, :17] = 1
    vision = synth.tensor("vision", (n_utt, LV, cfg.vision_featExtr_dim), seed=3, dtype=dd)
    vmask = torch.zeros(n_utt, LV, dtype=dd)
    for u, n in enumerate(num):
        vmask[u, :n] = 1
        vision[u, n:] = 0
    labels = torch.from_numpy(synth.randint("labels", (n_utt,), 0, 7, seed=4))
    frames = synth.tensor("frames", (nF, 3, 224, 224), seed=1, dtype=dd)
    return (ids, attn, sep, audio, amask, vision, vmask, labels, frames, torch.tensor(num), utt_idx)


def _gumbel(n, seed):
    g = torch.Generator().manual_seed(seed)
    return -torch.empty(n, 7, dtype=torch.float64).exponential_(generator=g).log()


def _models(cfg):
    from facialmmt_amd import models
    swin = models.SwinForAffwildClassification(cfg)
    mm = models.MultiModalTransformerForClassification(cfg)
    synth.fill_state_dict(swin, seed=100)
    synth.fill_state_dict(mm, seed=200)
    return SO.leaves(swin, torch.float64), SO.leaves(mm, torch.float64)


@pytest.fixture(scope="module")
def point():
    """the base point of the finite-difference test: leaves, inputs, noise, loss and autograd gradients"""
    cfg = _cfg()
    ssd, msd = _models(cfg)
    batch = _batch(cfg)
    noise = _gumbel(sum(NUM_IMGS), seed=11)
    plm = SO.standin_plm(msd)
    loss, mask, imp, preds = SO.target_step_loss(ssd, msd, plm, cfg, batch, noise)
    assert float((imp.detach() - THRESHOLD).abs().min()) >= SMOOTH_MARGIN, imp
    kept = imp > THRESHOLD
    assert bool(kept.any()) and not bool(kept.all()), imp                # the packing branch decides something
    ml, sl = SO.trainable(msd), SO.trainable(ssd)
    got = torch.autograd.grad(loss, list(ml.values()) + list(sl.values()), allow_unused=True)
    gm, gs = dict(zip(ml, got[:len(ml)])), dict(zip(sl, got[len(ml):]))
    assert torch.isfinite(loss) and all(g is None or torch.isfinite(g).all() for g in got)
    assert sum(g is not None and float(g.abs().max()) > 0 for g in gs.values()) > 150      # the gradient reaches Swin
    return dict(cfg=cfg, ssd=ssd, msd=msd, batch=batch, noise=noise, plm=plm, loss=loss.detach(), mask=mask, preds=preds.detach(), gm=gm, gs=gs)


def _directional(point, which, seed, h):
    """(<grad, dir>, fd(h), fd(h / 2)) for one seeded random direction over all leaves of one model: every tensor is moved along
    N(0,1) noise times its own largest magnitude, so h is a relative step"""
    sd, grads = (point["msd"], point["gm"]) if which == "mm" else (point["ssd"], point["gs"])
    lv = SO.trainable(sd)
    g = torch.Generator().manual_seed(seed)
    dirs = {k: torch.randn(v.shape, dtype=torch.float64, generator=g) * float(v.detach().abs().max()) for k, v in lv.items()}
    slope = sum(float((grads[k] * dirs[k]).sum()) for k in lv if grads[k] is not None)
    base = {k: v.detach().clone() for k, v in lv.items()}

    def loss_at(eps):
        with torch.no_grad():
            for k, v in lv.items():
                v.copy_(base[k] + eps * dirs[k])
            if which == "mm":                                # Swin does not move: its output is the base point's
                loss, mask, _ = SO.loss_from_preds(point["preds"], point["msd"], point["plm"], point["cfg"], point["batch"])
            else:
                loss, mask, _, _ = SO.target_step_loss(point["ssd"], point["msd"], point["plm"], point["cfg"], point["batch"], point["noise"])
        assert torch.equal(mask, point["mask"])              # no discrete decision flipped
        return float(loss)
    try:
        fds = [(loss_at(e) - loss_at(-e)) / (2 * e) for e in (h, h / 2)]
    finally:
        with torch.no_grad():
            for k, v in lv.items():
                v.copy_(base[k])
    return slope, fds[0], fds[1]


@pytest.mark.parametrize("which", ["mm", "swin"])
def test_reference_gradients_match_finite_differences(point, which):
    """8 seeded directions per model.  The error estimate of the central difference is the difference between its values at h and
    h / 2 (Richardson: an order of magnitude, hence the factor 10); |fd - <grad, dir>| <= 10 |fd(h) - fd(h/2)| + 1e-9 |<grad, dir>|."""
    h = 2e-5
    worst = 0.0
    for seed in range(8):
        slope, f1, f2 = _directional(point, which, 1000 + seed, h)
        est = abs(f1 - f2)
        err = abs(f2 - slope)
        print(f"{which} direction {seed}: <grad,dir> {slope:+.12e}  fd(h/2) {f2:+.12e}  |fd - slope| {err:.3e}  |fd(h) - fd(h/2)| {est:.3e}")
        assert slope != 0.0
        assert err <= 10 * est + 1e-9 * abs(slope), (seed, slope, f1, f2)
        worst = max(worst, err / abs(slope))
    # the check has teeth: the reference judges gradients at 1e-3 (tests/test_gpu_step_oracle.py), so its own must be confirmed an order finer
    assert worst < 1e-4, worst


def test_threshold_zero_is_the_plain_composition():
    """threshold 0, one utterance: every frame is kept in place, the mask is unchanged, and the step loss is
    cross_entropy(multimodal_logits(vision | preds)) assembled by hand"""
    import torch.nn.functional as F
    from oracle.multimodal import multimodal_logits
    from oracle.swin import swin_affwild_logits
    cfg = _cfg()
    cfg.FacialEmoImpor_threshold = 0.0
    cfg.trg_accumulation_steps = 3
    ssd, msd = _models(cfg)
    batch = _batch(cfg, n_utt=1)
    noise = _gumbel(NUM_IMGS[0], seed=12)
    with torch.no_grad():
        loss, mask, imp, preds = SO.target_step_loss(ssd, msd, SO.standin_plm(msd), cfg, batch, noise)
        p = torch.softmax((swin_affwild_logits(ssd, batch[8], training=True) + noise) / cfg.tau, -1)
        vis = torch.cat((batch[5], p[None]), dim=-1)
        table = msd["roberta.emb.weight"]                   # (fill_state_dict refilled the stand-in encoder's table with the model's seed)
        logits = multimodal_logits(msd, lambda ids, m: (table[ids] * m.unsqueeze(-1),), cfg, batch[0], batch[1], batch[2], batch[3], batch[4], vis, batch[6], batch[10])
        want = F.cross_entropy(logits, batch[7]) / 3
    assert torch.equal(mask, batch[6])
    assert torch.equal(preds, p) and torch.allclose(imp, (p * p).sum(1), rtol=1e-14, atol=0)
    assert abs(float(loss) - float(want)) <= 1e-13 * abs(float(want)), (float(loss), float(want))


def test_accumulation_over_the_same_micro_batch_twice_gives_the_single_step_gradients():
    cfg = _cfg()
    ssd, msd = _models(cfg)
    batch = _batch(cfg)
    noise = _gumbel(sum(NUM_IMGS), seed=11)
    start = {k: v.detach().clone() for k, v in SO.trainable(msd).items()}
    cfg.clip = 1e9
    one = SO.run(ssd, msd, cfg, [batch], [noise], [None], lr=0.05, keep_grads=True)
    after_one = {k: v.detach().clone() for k, v in SO.trainable(msd).items()}
    with torch.no_grad():
        for k, v in SO.trainable(msd).items():
            v.copy_(start[k])
    cfg.trg_accumulation_steps = 2
    two = SO.run(ssd, msd, cfg, [batch, batch], [noise, noise], [None, None], lr=0.05, keep_grads=True)
    assert len(one["steps"]) == 1 and len(two["steps"]) == 1 and len(two["micro"]) == 2
    assert abs(two["micro"][0]["loss"] * 2 - one["micro"][0]["loss"]) <= 1e-13 * abs(one["micro"][0]["loss"])
    assert abs(two["steps"][0]["norm"] - one["steps"][0]["norm"]) <= 1e-12 * one["steps"][0]["norm"]
    g1, g2 = one["steps"][0]["grads"], two["steps"][0]["grads"]
    assert one["micro"][0]["unused"] == two["micro"][0]["unused"] == [k for k in g1 if g1[k] is None]
    for k in g1:
        if g1[k] is None:
            assert g2[k] is None, k
            continue
        assert float((g1[k] - g2[k]).norm()) <= 1e-12 * float(g1[k].norm()), k
        # ... and the update moved the parameter by -lr * gradient (no clipping at this clip)
        assert torch.allclose(after_one[k], start[k] - 0.05 * g1[k], rtol=0, atol=1e-14 * max(1.0, float(start[k].abs().max()))), k
        assert float((msd[k].detach() - after_one[k]).abs().max()) <= 1e-12 * max(1.0, float(after_one[k].abs().max())), k
    # Swin's leaves were never touched
    ref, _ = _models(_cfg())
    assert all(torch.equal(ssd[k], ref[k]) for k in ssd)
