"""GPU tests of skip_nonfinite=True on the three graphed training steps: an update whose gradient norm is NaN or infinite is skipped on the device --
parameters, moments and the update count keep their bits --, the monitor counts it, the next clean batch trains; with the option on and finite
gradients every bit is the default step's.

Builders and shapes are those of the files named: the V-only step of tests/test_gpu_unimodal_step.py (B = 4, L = 160, two layers, fp32, dropout 0), the
T+A+V step of tests/test_gpu_ragged_buckets.py (B = 2, Lv = 6, stand-in text encoder, frame_capacity (8, 12)), the auxiliary step of
tests/test_gpu_short_batch.py (8 images).  The optimizers are the ones the FUSED update takes (torch.optim.AdamW / HFAdamW with a device learning
rate): the option exists only there.  Every comparison is torch.equal."""
import pytest
import torch

from tests import test_gpu_ragged_buckets as RB
from tests import test_gpu_short_batch as SB
from tests import test_gpu_unimodal_step as US

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _adamw(params, dev, lr=1e-3):
    return torch.optim.AdamW(params, lr=torch.tensor(lr, device=dev), fused=True, capturable=True, weight_decay=0.01, eps=1e-6)


def _unimodal(dev, accumulation=1, seed=201, **kw):
    from facialmmt_amd.train_step import GraphedUnimodalStep
    cfg, model = US.build(dev, accumulation=accumulation, seed=seed)
    step = GraphedUnimodalStep(model, _adamw(model.parameters(), dev), None, cfg, US.micro_batch(dev, 80), **kw)
    assert step.fused is not None
    return step, model


def _poisoned(batch):
    """the batch with ONE NaN in `feature`, at a token its mask keeps"""
    x, mask, labels = batch
    assert float(mask[0, 5]) == 1.0
    x = x.clone()
    x[0, 5, 11] = float("nan")
    return x, mask, labels


def _state(step, model):
    """everything an update writes: the parameters, the fused moments and the update count"""
    torch.cuda.synchronize()
    return [p.detach().clone() for p in model.parameters()] + [t.clone() for t in step.fused.m + step.fused.v] + [step.fused.step.clone()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _finite(tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


def test_unimodal_step_skips_the_poisoned_batch_and_trains_on(dev):
    clean, clean2 = US.micro_batch(dev, 80), US.micro_batch(dev, 81)
    fed = (clean, _poisoned(clean), clean2)
    step, model = _unimodal(dev, skip_nonfinite=True)
    assert step.monitor is not None and step.tail.monitor is step.monitor and step.fused.monitor is step.monitor
    r = step.monitor.read()                                     # the warm-up passes left nothing
    assert (r.micro_steps, r.nonfinite_losses, r.applied, r.skipped, r.loss_sum, r.last_norm) == (0, 0, 0, 0, 0.0, 0.0) and float(step.fused.step) == 0.0
    start = _state(step, model)
    loss1 = float(step(fed[0]))
    after1 = _state(step, model)
    assert not any(torch.equal(a, b) for a, b in zip(start, after1))
    loss2 = float(step(fed[1]))
    after2 = _state(step, model)
    r = step.monitor.read()
    print("losses", loss1, loss2, "monitor", r)
    assert loss2 != loss2                                       # the forward really was NaN
    assert _same(after1, after2) and float(step.fused.step) == 1.0
    assert (r.skipped, r.applied, r.nonfinite_losses, r.micro_steps) == (1, 1, 1, 1) and r.last_norm != r.last_norm
    assert r.avg_loss == loss1                                  # the one finite loss, an fp32 value widened
    loss3 = float(step(fed[2]))
    after3 = _state(step, model)
    r = step.monitor.read()
    assert loss3 == loss3 and _finite(after3)
    assert not any(torch.equal(a, b) for a, b in zip(after2, after3))
    assert (r.skipped, r.applied, r.nonfinite_losses, r.micro_steps) == (1, 2, 1, 2) and float(step.fused.step) == 2.0
    assert r.last_norm == float(step.fused.norm) and r.last_norm > 0
    assert r.avg_loss == (loss1 + loss3) / 2
    # the default step on the same three batches: today's behaviour, and the proof that the batch was poisonous
    twin, twin_model = _unimodal(dev)
    assert twin.monitor is None and _same(_state(twin, twin_model), start)
    twin(fed[0])
    assert _same(_state(twin, twin_model), after1)             # the option changes no bit of a clean update
    twin(fed[1])
    twin(fed[2])
    torch.cuda.synchronize()
    assert not any(bool(torch.isfinite(p).any()) for p in twin_model.parameters()) and float(twin.fused.step) == 3.0


def test_unimodal_accumulation_window_with_a_bad_first_micro_step(dev):
    """trg_accumulation_steps = 2: the bad batch opens a window, the window's one update is skipped, every flat buffer is exactly zero afterwards and
    the next window applies"""
    clean, clean2 = US.micro_batch(dev, 80), US.micro_batch(dev, 81)
    step, model = _unimodal(dev, accumulation=2, skip_nonfinite=True)
    start = _state(step, model)
    step(_poisoned(clean))
    torch.cuda.synchronize()
    assert any(not _finite([b[0]]) for b in step.flat.buckets)  # the open window holds the poison
    step(clean2)
    assert _same(_state(step, model), start)
    assert all(int(torch.count_nonzero(b[0])) == 0 for b in step.flat.buckets)          # a NaN would count as non-zero
    r = step.monitor.read()
    assert (r.skipped, r.applied, r.nonfinite_losses, r.micro_steps) == (1, 0, 1, 1) and float(step.fused.step) == 0.0
    step(clean)
    step(clean2)
    after = _state(step, model)
    r = step.monitor.read()
    assert _finite(after) and not any(torch.equal(a, b) for a, b in zip(start, after))
    assert (r.skipped, r.applied, r.nonfinite_losses, r.micro_steps) == (1, 1, 1, 3) and float(step.fused.step) == 1.0
    assert all(int(torch.count_nonzero(b[0])) == 0 for b in step.flat.buckets)
    # the same window on a default step of the same start: the clean window's update has the same bits -- nothing of the bad one survived
    twin, twin_model = _unimodal(dev, accumulation=2)
    twin(clean)
    twin(clean2)
    assert _same(_state(twin, twin_model), after)


def test_target_step_keeps_its_bits_on_a_nan_in_audio(dev):
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW
    cfg, swin, mm = RB._models(dev, 1)
    params = [p for p in mm.parameters() if p.requires_grad]
    opt = HFAdamW(params, lr=torch.tensor(1e-4, device=dev), weight_decay=0.01)
    small, large = RB._batches(dev, cfg, [3, 4])[0], RB._batches(dev, cfg, [6, 5])[0]
    step = GraphedTargetStep(swin, mm, opt, None, cfg, small, autocast_dtype=None, frame_capacity=RB.BUCKETS, skip_nonfinite=True)
    assert step.fused is not None and step.monitor is not None and step.monitor.read().micro_steps == 0
    step(small)
    after1 = _state(step, mm)
    audio = large[3].clone()
    audio[1, 0, 0] = float("nan")                               # one row of the batch that replays the OTHER capacity: the captures share the monitor
    loss, _ = step(large[:3] + (audio,) + large[4:])
    after2 = _state(step, mm)
    r = step.monitor.read()
    print("poisoned loss", float(loss), "monitor", r, "capacities", step.replays)
    assert step.replays == {8: 1, 12: 1}
    assert _same(after1, after2) and float(step.fused.step) == 1.0
    assert (r.skipped, r.applied, r.nonfinite_losses, r.micro_steps) == (1, 1, 1, 1)
    step(small)
    after3 = _state(step, mm)
    r = step.monitor.read()
    assert _finite(after3) and (r.skipped, r.applied, r.micro_steps) == (1, 2, 2) and float(step.fused.step) == 2.0
    moved = sum(int(not torch.equal(a, b)) for a, b in zip(after2[:len(params)], after3[:len(params)]))
    assert moved > 0.9 * len(params), (moved, len(params))


def test_auxiliary_step_changes_no_bit_on_clean_batches(dev):
    """nothing changes when nothing is wrong, on the step that has BatchNorm: the twin without the option, same seed, same batches"""
    from facialmmt_amd.train_step import GraphedAuxStep
    imgs, labels = SB._aux(dev, 16)
    fed = [(imgs[:8].clone(), labels[:8].clone()), (imgs[8:].clone(), labels[8:].clone())]
    out = {}
    for guard in (False, True):
        torch.manual_seed(11)
        torch.cuda.manual_seed_all(11)
        cfg, swin = SB._aux_model(dev)
        step = GraphedAuxStep(swin, _adamw(swin.parameters(), dev, lr=5e-5), None, cfg, *fed[0], skip_nonfinite=guard)
        assert step.fused is not None and (step.monitor is not None) == guard
        losses = [step(*b).clone() for b in fed]
        bn = swin.swin.output_layer[3]
        out[guard] = _state(step, swin) + [bn.running_mean.clone(), bn.running_var.clone(), torch.stack(losses)]
        if guard:
            r = step.monitor.read()
            assert (r.applied, r.skipped, r.micro_steps, r.nonfinite_losses) == (2, 0, 2, 0)
            assert r.avg_loss == (float(losses[0]) + float(losses[1])) / 2 and r.last_norm == float(step.fused.norm)
    assert float(out[True][-4]) == 2.0 and _finite(out[True])
    assert _same(out[False], out[True])


def test_the_option_needs_the_fused_update_and_is_no_part_of_the_state(dev):
    from facialmmt_amd.train_step import GraphedUnimodalStep
    cfg, model = US.build(dev)
    before = [p.detach().clone() for p in model.parameters()]
    for opt in (torch.optim.AdamW(model.parameters(), lr=1e-3), torch.optim.SGD(model.parameters(), lr=0.05)):      # a host-float learning rate; not AdamW
        with pytest.raises(ValueError, match="skip_nonfinite"):
            GraphedUnimodalStep(model, opt, None, cfg, US.micro_batch(dev, 80), skip_nonfinite=True)
        assert all(p.grad is None for p in model.parameters()) and not opt.state          # no warm-up pass ran
    assert _same(before, [p.detach() for p in model.parameters()])
    # state_dict() of a guarded step loads into an unguarded step of the same kind, and back; the run continues with the same bits
    clean, clean2 = US.micro_batch(dev, 80), US.micro_batch(dev, 81)
    guarded, g_model = _unimodal(dev, skip_nonfinite=True)
    plain, p_model = _unimodal(dev, seed=202)
    guarded(clean)
    guarded(_poisoned(clean))
    plain.load_state_dict(guarded.state_dict())
    assert _same(_state(guarded, g_model), _state(plain, p_model)) and float(plain.fused.step) == 1.0
    guarded(clean2)
    plain(clean2)
    assert _same(_state(guarded, g_model), _state(plain, p_model))
    plain(clean)
    counters = guarded.monitor.words.clone()
    guarded.load_state_dict(plain.state_dict())
    assert _same(_state(guarded, g_model), _state(plain, p_model)) and float(guarded.fused.step) == 3.0
    assert torch.equal(guarded.monitor.words, counters)         # diagnostics: a loaded state neither carries nor touches them
