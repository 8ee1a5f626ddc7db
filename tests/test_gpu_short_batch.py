"""GPU tests of pad_rows=True on the three graphed steps: the short last batch of an epoch, padded to the captured shape (train_step.pad_*_batch,
PAD_NOTE) and replayed through the SAME captures, against the eager step of the same kind on the COMPACT short batch.

Noise-free configurations, as the ragged step tests arrange them (dropout 0 everywhere, DropPath off, Gumbel-softmax at tau = 1e5), so that nothing drawn
depends on the number of rows.  Tolerances are those of the files named per test; nothing here is wider.

V-only: B = 4, L = 160, fp32, trg_accumulation_steps = 2, fed full, b = 1, full, b = 3 -- two updates, each window mixing a full and a short batch.
  Graphed side: torch.optim.AdamW with a device learning rate, i.e. the FUSED optimizer (asserted); eager side: a deep copy under a stock AdamW.  Bars
  of tests/test_gpu_unimodal_step.py: losses 2e-4 of max(1, |loss|), parameters 1e-4 of max(1, max|p|).  Why Adam can be held to the SGD bar here:
  lr = 1e-3 and eps = 1e-6, two updates.  An entry whose gradient is rounding noise (|g| ~ 1e-9: the key bias of a softmax attention, the pooling's
  value bias) moves by lr |g| / (|g| + eps) ~ 1e-6 per update; an entry at |g| = 1e-7 with 1 % relative noise between the two sides differs by
  1e-5 per update; both below 1e-4.  A real mistake (the short batch weighted by 1 / B, moments that missed an update) flips signs of first-step
  Adam updates: 2e-3 per entry.
T+A+V: B = 2, Lv = 6, frame_capacity = (8, 12), SGD at 0.05, accumulation 2, fed [6, 5], short [3], short [4], [3, 4]; recipe and bars of
  tests/test_gpu_ragged_buckets.py (losses 2e-4, parameters and BatchNorm running statistics 1e-4 of scale, kept-frame masks equal).
Auxiliary: 8 images then 3, SGD, bars of tests/test_gpu_train_step.py's graph-against-eager tests (losses 2e-4, parameters and running mean 1e-4).

Every comparison prints its figures before it asserts (run with -s)."""
import copy
import types

import pytest
import torch

from facialmmt_amd import synth
from tests import test_gpu_ragged_buckets as RB
from tests import test_gpu_unimodal_step as US

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _close(label, a, b, bar):
    worst = (0.0, None)
    for k in a:
        err = float((a[k].detach().double() - b[k].detach().double()).abs().max()) / max(1.0, float(a[k].detach().abs().max()))
        worst = (err, k) if worst[1] is None or err > worst[0] else worst
    print(f"{label}: worst {worst} (bar {bar:.0e})")
    assert worst[0] <= bar, (label, worst)


# ------------------------------------------------------------------------------------------------ V-only
def test_unimodal_short_batches_through_the_fused_optimizer(dev):
    from facialmmt_amd.train_step import GraphedUnimodalStep, UnimodalStep
    cfg, model = US.build(dev, accumulation=2)
    eager_model = copy.deepcopy(model)
    rows = (US.B, 1, US.B, 3)
    batches = [US.micro_batch(dev, 50 + i, n=n) for i, n in enumerate(rows)]
    kw = dict(weight_decay=0.01, eps=1e-6)
    step = GraphedUnimodalStep(model, torch.optim.AdamW(model.parameters(), lr=torch.tensor(1e-3, device=dev), fused=True, capturable=True, **kw), None, cfg,
                               batches[0], pad_rows=True)
    assert step.fused is not None                               # the case the eager route for a short batch broke
    assert step.rows is None and step.padded_calls == 0
    eager = UnimodalStep(eager_model, torch.optim.AdamW(eager_model.parameters(), lr=1e-3, **kw), None, cfg)
    got, want, seen = [], [], []
    for b in batches:
        got.append(float(step(b)))
        seen.append((step.rows, step.padded_calls, step.i_batch))
        want.append(float(eager(b)))
    torch.cuda.synchronize()
    print("losses graphed, padded", got)
    print("losses eager, compact ", want)
    assert seen == [(4, 0, 1), (1, 1, 2), (4, 1, 3), (3, 2, 4)]
    assert step.logits.shape == (US.B, 7) and not step.opt.state         # the moments live in the fused optimizer
    for a, b in zip(want, got):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (want, got)
    start = US.build(dev, accumulation=2)[1]
    moved = sum(int(not torch.equal(p, q)) for p, q in zip(eager_model.parameters(), start.parameters()))
    assert moved > 0.9 * len(list(start.parameters()))
    _close("V-only parameters after two updates", dict(eager_model.named_parameters()), dict(model.named_parameters()), 1e-4)
    for bad in (US.micro_batch(dev, 60, n=US.B + 1), tuple(t[:0] for t in batches[0])):
        with pytest.raises(ValueError):
            step(bad)
    assert step.i_batch == 4 and step.padded_calls == 2


def test_unimodal_full_batches_have_the_bits_of_the_plain_capture_and_the_default_still_raises(dev):
    """pad_rows=True changes nothing on full batches (valid_mean with every label valid: the plain pair's bits), and pad_rows=False rejects a short
    batch as before"""
    from facialmmt_amd.train_step import GraphedUnimodalStep
    out = {}
    for pad in (False, True):
        cfg, model = US.build(dev, accumulation=1)
        step = GraphedUnimodalStep(model, torch.optim.SGD(model.parameters(), lr=0.05), None, cfg, US.micro_batch(dev, 70), pad_rows=pad)
        losses = [step(US.micro_batch(dev, 70 + i)).clone() for i in range(2)]
        if not pad:
            with pytest.raises(ValueError):
                step(US.micro_batch(dev, 72, n=3))
        torch.cuda.synchronize()
        out[pad] = (torch.stack(losses), [p.detach().clone() for p in model.parameters()])
    assert torch.equal(out[False][0], out[True][0])
    assert all(torch.equal(a, b) for a, b in zip(out[False][1], out[True][1]))


# ------------------------------------------------------------------------------------------------ T+A+V
def _short(batch, b):
    """the loader's batch cut to its first b utterances"""
    return tuple(t[:b] for t in batch)


def test_target_step_mixes_full_and_short_batches_in_a_window(dev):
    from facialmmt_amd.train_step import GraphedTargetStep, TargetStep
    buckets = RB.BUCKETS
    seq = (([6, 5], 2), ([3, 4], 1), ([4, 2], 1), ([3, 4], 2))              # (frame counts of the loader batch, rows fed)
    runs = {}
    for side in ("eager", "graphed"):
        cfg, swin, mm = RB._models(dev, 2)
        opt = torch.optim.SGD(mm.parameters(), lr=0.05)
        fed = [_short(RB._batches(dev, cfg, n)[0], b) for n, b in seq]
        if side == "eager":
            step = TargetStep(swin, mm, opt, None, cfg, autocast_dtype=None, frame_capacity=buckets)
        else:
            step = GraphedTargetStep(swin, mm, opt, None, cfg, fed[0], autocast_dtype=None, frame_capacity=buckets, pad_rows=True)
        losses, kept, seen = [], [], []
        for batch in fed:
            loss, k = step(batch)
            losses.append(float(loss))
            kept.append(k.clone())
            seen.append((step.capacity, step.frame_counts.tolist(), getattr(step, "rows", None), getattr(step, "padded_calls", None)))
        torch.cuda.synchronize()
        bn = swin.swin.output_layer[3]
        runs[side] = types.SimpleNamespace(losses=losses, kept=kept, seen=seen, params={k: v.detach().clone() for k, v in mm.named_parameters()},
                                           stats={"mean": bn.running_mean.clone(), "var": bn.running_var.clone()}, tracked=int(bn.num_batches_tracked))
    e, g = runs["eager"], runs["graphed"]
    print("losses eager, compact ", e.losses)
    print("losses graphed, padded", g.losses)
    print("graphed (capacity, frame_counts, rows, padded_calls)", g.seen)
    assert g.seen == [(12, [11, 11], 2, 0), (8, [3, 3], 1, 1), (8, [4, 4], 1, 2), (8, [7, 7], 2, 2)]      # the bucket of the REAL frames
    assert [s[:2] for s in e.seen] == [s[:2] for s in g.seen]
    assert e.losses[0] != e.losses[-1]
    for a, b in zip(e.losses, g.losses):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (e.losses, g.losses)
    for (n, b), ke, kg in zip(seq, e.kept, g.kept):
        assert kg.shape[0] == RB.B and torch.equal(kg[:b], ke) and float(ke.sum()) > 0          # the real rows' kept frames
        assert float(kg[b:].abs().sum()) == 0.0                                                # a padded row keeps nothing
    assert e.tracked == g.tracked == 4
    _close("T+A+V BatchNorm running statistics", e.stats, g.stats, 1e-4)
    _close("T+A+V parameters after two updates", e.params, g.params, 1e-4)


def test_target_step_restrictions_and_the_default(dev):
    from facialmmt_amd.train_step import GraphedTargetStep
    cfg, swin, mm = RB._models(dev, 1)
    opt = torch.optim.SGD(mm.parameters(), lr=0.05)
    padded, compact = RB._batches(dev, cfg, [3, 4])
    before = torch.cuda.memory_allocated(dev)
    with pytest.raises(ValueError, match="frame_capacity"):                  # compact frames: a short batch changes their shape
        GraphedTargetStep(swin, mm, opt, None, cfg, compact, autocast_dtype=None, pad_rows=True)
    for mode in ("pipeline_swin", "branch_graphs", "fork_streams"):
        with pytest.raises(NotImplementedError):
            GraphedTargetStep(swin, mm, opt, None, cfg, padded, autocast_dtype=None, frame_capacity=12, pad_rows=True, **{mode: True})
    active = types.SimpleNamespace(active=True)
    with pytest.raises(NotImplementedError):
        GraphedTargetStep(swin, mm, opt, None, cfg, padded, autocast_dtype=None, frame_capacity=12, pad_rows=True, averager=active)
    assert torch.cuda.memory_allocated(dev) == before                        # raised before any warm-up or capture
    step = GraphedTargetStep(swin, mm, opt, None, cfg, padded, autocast_dtype=None, frame_capacity=12)
    with pytest.raises(ValueError):                                          # pad_rows=False: the short batch is still rejected
        step(_short(padded, 1))
    assert step.i_batch == 0 and step.padded_calls == 0


# ------------------------------------------------------------------------------------------------ auxiliary
def _aux(dev, n):
    import bench
    args = types.SimpleNamespace(aux_images=n, dtype="fp32", input="float")
    imgs, labels = bench.synth_aux_batch(args, torch.device("cpu"), 0)
    return imgs.to(dev), labels.to(dev)


def _aux_model(dev):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    cfg = default_args(aux_accumulation_steps=1)
    swin = models.SwinForAffwildClassification(cfg)
    synth.fill_state_dict(swin, seed=100)
    for m in swin.modules():
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    return cfg, swin.to(dev).train()


def test_auxiliary_step_eight_images_then_three(dev):
    from facialmmt_amd.train_step import AuxStep, GraphedAuxStep
    imgs, labels = _aux(dev, 12)
    full = (imgs[:8].clone(), labels[:8].clone())
    short = (imgs[8:11].clone(), labels[8:11].clone())                                # three images the full batch does not hold
    runs = {}
    for side in ("eager", "graphed", "plain"):
        cfg, swin = _aux_model(dev)
        opt = torch.optim.SGD(swin.parameters(), lr=0.02)
        if side == "eager":
            step = AuxStep(swin, opt, None, cfg)
        else:
            step = GraphedAuxStep(swin, opt, None, cfg, *full, pad_rows=side == "graphed")
        losses = [float(step(*full))]
        if side == "plain":                                                   # pad_rows=False: the short batch is still rejected
            with pytest.raises(ValueError):
                step(*short)
        else:
            losses.append(float(step(*short)))
        torch.cuda.synchronize()
        if side == "graphed":
            assert step.rows == 3 and step.padded_calls == 1 and step.i_batch == 2 and int(step.n_valid) == 3
            with pytest.raises(ValueError):
                step(imgs[:9], labels[:9])
        bn = swin.swin.output_layer[3]
        runs[side] = (losses, {k: v.detach().clone() for k, v in swin.named_parameters()}, {"mean": bn.running_mean.clone(), "var": bn.running_var.clone()},
                      int(bn.num_batches_tracked))
    print("losses eager, compact ", runs["eager"][0])
    print("losses graphed, padded", runs["graphed"][0])
    print("loss of the full batch, pad_rows=False", runs["plain"][0])
    assert runs["plain"][0][0] == runs["graphed"][0][0]                       # n_valid == n_cap: the unmasked bits
    for a, b in zip(runs["eager"][0], runs["graphed"][0]):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (runs["eager"][0], runs["graphed"][0])
    assert runs["eager"][3] == runs["graphed"][3] == 2
    _close("auxiliary BatchNorm running statistics", runs["eager"][2], runs["graphed"][2], 1e-4)
    _close("auxiliary parameters after two updates", runs["eager"][1], runs["graphed"][1], 1e-4)
