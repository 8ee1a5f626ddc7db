"""GPU tests of grad_report=True on the graphed training steps: the per-parameter gradient statistics a captured update leaves behind, the snapshot that
names the tensor behind a skipped update, and that the option changes no bit of the run.

Builders and shapes are those of the files named: the V-only step of tests/test_gpu_unimodal_step.py (B = 4, L = 160, two layers, fp32, dropout 0) with
the fused-update optimizer of tests/test_gpu_guard_steps.py, and the T+A+V step of tests/test_gpu_ragged_buckets.py (B = 2, Lv = 6, stand-in text
encoder, frame_capacity (8, 12)) with bf16 masters of the text encoder as tests/test_gpu_step_state.py builds them.

Tolerances.  Per-parameter norms against the eager twin's p.grad: the bars tests/test_gpu_step_oracle.py::compare_fp32_gradients holds the V-only step's
gradients to in tests/test_gpu_unimodal_step.py -- relative L2 <= 1e-3 per tensor, which bounds the difference of the two norms by 1e-3 of the norm
(triangle inequality); a tensor whose eager gradient lies under 1e-3 of its siblings' scale (the analytically zero ones: the key bias of a softmax
attention, the pooling's value bias) is held to that file's zero-gradient bar, max|g| <= 1e-3 of the siblings' scale.  total_norm against the monitor's
last_norm: N * 2^-24 relative, N the element count -- both are fp32 sums of the same N non-negative squares in some order.
Every comparison prints its figures first (run with -s)."""
import numpy as np
import pytest
import torch

from tests import test_gpu_guard_steps as GS
from tests import test_gpu_ragged_buckets as RB
from tests import test_gpu_step_oracle as TS
from tests import test_gpu_unimodal_step as US

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_unimodal_report_matches_the_eager_twins_gradients(dev):
    from facialmmt_amd.train_step import GradReport, UnimodalStep
    batch = US.micro_batch(dev, 80)
    step, model = GS._unimodal(dev, skip_nonfinite=True, grad_report=True)
    rep = step.grad_report
    assert isinstance(rep, GradReport) and step.tail.report is rep and step.fused.report is rep
    names = [k for k, _ in model.named_parameters()]
    assert rep.names == names and len(names) == step.fused.n and all(p is q for p, q in zip(step.fused.keep[0], model.parameters()))
    r0 = rep.read()                                             # the warm-up passes left nothing
    assert r0.bad_updates == 0 and r0.last_bad is None and r0.total_norm == 0.0 and int(r0.nonfinite.sum()) == 0
    step(batch)
    r = rep.read()
    mon = step.monitor.read()
    # the eager twin: same start, same batch, gradients caught as autograd accumulates them (before the clip scales them)
    cfg, twin = US.build(dev)
    seen, hooks = TS.hook_gradients(twin)
    UnimodalStep(twin, torch.optim.SGD(twin.parameters(), lr=0.0), None, cfg)(batch)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert sorted(seen) == sorted(names)
    ref = {k: g.double() for k, g in seen.items()}
    bad, elements = [], 0
    for i, k in enumerate(names):
        g = ref[k]
        elements += g.numel()
        want, scale = float(g.norm()), TS.siblings_scale(k, ref)
        got, got_max = float(r.norm[i]), float(r.max_abs[i])
        print(f"{k}: report norm {got:.9e} eager {want:.9e}  max_abs {got_max:.6e} eager {float(g.abs().max()):.6e}  siblings' scale {scale:.3e}")
        if float(g.abs().max()) <= 1e-3 * scale:
            ok = got_max <= 1e-3 * scale
        else:
            ok = abs(got - want) <= 1e-3 * want
        if not ok or int(r.nonfinite[i]) != 0:
            bad.append((k, got, want))
    assert not bad, bad
    print(f"total_norm {r.total_norm!r} monitor last_norm {mon.last_norm!r} elements {elements}")
    assert mon.applied == 1 and mon.last_norm > 0
    assert abs(r.total_norm - mon.last_norm) <= elements * 2.0 ** -24 * mon.last_norm
    assert r.bad_updates == 0 and r.last_bad is None
    order = np.argsort(-r.norm, kind="stable")
    assert rep.worst(3) == [names[i] for i in order[:3]]


def test_the_option_changes_no_bit(dev):
    fed = [US.micro_batch(dev, 80 + i) for i in range(3)]
    out = {}
    for on in (False, True):
        step, model = GS._unimodal(dev, grad_report=on)
        assert (step.grad_report is not None) == on and (step.fused.report is not None) == on and (step.tail.report is not None) == on
        assert step.monitor is None
        for b in fed:
            step(b)
        out[on] = GS._state(step, model)
        if on:
            r = step.grad_report.read()
            assert r.total_norm > 0 and int(r.nonfinite.sum()) == 0 and r.bad_updates == 0
            assert "grad_report" not in step.state_dict() and not any("report" in str(k) for k in step.state_dict())
    assert float(out[True][-1]) == 3.0 and GS._finite(out[True])
    assert GS._same(out[False], out[True])


def test_the_report_names_the_cause_of_a_skipped_window(dev):
    """accumulation 2, skip_nonfinite: a NaN written into classifier.bias's flat gradient behind the first micro-step -- the window's update is skipped, and
    the snapshot says why"""
    clean, clean2 = US.micro_batch(dev, 80), US.micro_batch(dev, 81)
    step, model = GS._unimodal(dev, accumulation=2, skip_nonfinite=True, grad_report=True)
    rep = step.grad_report
    start = GS._state(step, model)
    step(clean)
    step.tail.flat_view_of[model.classifier.bias][0] = float("nan")
    step(clean2)
    r, mon = rep.read(), step.monitor.read()
    at = rep.names.index("classifier.bias")
    print("monitor", mon, "bad_updates", r.bad_updates, "first", r.last_bad.first, "nonfinite", r.last_bad.nonfinite.tolist())
    assert mon.skipped == 1 and mon.applied == 0 and r.bad_updates == 1
    assert r.last_bad.first == "classifier.bias"
    assert r.last_bad.nonfinite.tolist() == [1 if i == at else 0 for i in range(rep.n)]
    assert np.isnan(r.last_bad.norm[at]) and np.isfinite(np.delete(r.last_bad.norm, at)).all() and np.isnan(r.last_bad.total_norm)
    assert np.array_equal(r.nonfinite, r.last_bad.nonfinite)   # the last update IS the bad one
    assert GS._same(GS._state(step, model), start)
    snapshot = rep.bad_stats.clone()
    step(clean)
    step(clean2)
    after = GS._state(step, model)
    r, mon = rep.read(), step.monitor.read()
    assert int(r.nonfinite.sum()) == 0 and np.isfinite(r.norm).all() and r.total_norm > 0
    assert abs(r.total_norm - mon.last_norm) <= sum(p.numel() for p in model.parameters()) * 2.0 ** -24 * mon.last_norm
    assert r.bad_updates == 1 and r.last_bad.first == "classifier.bias" and torch.equal(rep.bad_stats, snapshot)
    assert (mon.skipped, mon.applied) == (1, 1)
    # a run that never saw the poisoned window
    twin, twin_model = GS._unimodal(dev, accumulation=2)
    assert twin.grad_report is None
    twin(clean)
    twin(clean2)
    assert GS._same(GS._state(twin, twin_model), after)


def test_state_names_the_parameter_with_a_bad_moment(dev):
    step, model = GS._unimodal(dev, grad_report=True)
    rep = step.grad_report
    step(US.micro_batch(dev, 80))
    before = rep.buf.clone()
    names = rep.names
    at = names.index("attention.linear_key.weight") if "attention.linear_key.weight" in names else len(names) // 2
    step.fused.m[at].view(-1)[3] = float("nan")
    r = rep.state("m")
    print("state('m'): nonfinite", r.nonfinite.tolist())
    assert r.names == names and r.nonfinite.tolist() == [1 if i == at else 0 for i in range(len(names))]
    assert np.isnan(r.norm[at]) and r.worst(1) == [names[at]] and not hasattr(r, "last_bad")
    v = rep.state("v")
    assert int(v.nonfinite.sum()) == 0 and (v.max_abs >= 0).all()
    p = rep.state("p")
    for i, q in enumerate(model.parameters()):
        want = float((q.detach().double() ** 2).sum())
        assert abs(float(p.sumsq[i]) - want) <= (q.numel() + 2) * 2.0 ** -24 * want, names[i]
        assert float(p.max_abs[i]) == float(q.detach().abs().max())
    assert torch.equal(rep.buf, before)                         # on demand: the captured update's records are not touched
    with pytest.raises(ValueError):
        rep.state("g")


def test_target_step_with_bf16_masters_names_the_audio_path(dev):
    """T+A+V, bf16 masters of the text encoder, NO guard: the NaN in the audio input turns the parameters into NaN as ever, and the snapshot says where from"""
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, named_step_parameters, step_parameters
    cfg, swin, mm = RB._models(dev, 1)
    mw = MasterWeights(mm.roberta, torch.bfloat16)
    opt = HFAdamW(step_parameters(mm, mw), lr=torch.tensor(1e-4, device=dev), weight_decay=0.01)
    small, large = RB._batches(dev, cfg, [3, 4])[0], RB._batches(dev, cfg, [6, 5])[0]
    step = GraphedTargetStep(swin, mm, opt, None, cfg, small, autocast_dtype=None, masters=mw, frame_capacity=RB.BUCKETS, grad_report=True)
    rep = step.grad_report
    assert step.fused is not None and step.monitor is None and rep is not None
    named = dict(named_step_parameters(mm, mw))
    assert len(rep.names) == step.fused.n == len(named) and set(rep.names) == set(named)
    assert all(named[k] is p for k, p in zip(rep.names, step.fused.keep[0]))
    assert any(k.startswith("roberta.") for k in rep.names) and not any(k.startswith("param") for k in rep.names)
    step(small)
    r = rep.read()
    elements, norm = sum(p.numel() for p in step.fused.keep[0]), float(step.fused.norm)
    print(f"total_norm {r.total_norm!r} the update's norm word {norm!r} elements {elements}")
    assert r.bad_updates == 0 and int(r.nonfinite.sum()) == 0 and norm > 0 and abs(r.total_norm - norm) <= elements * 2.0 ** -24 * norm
    audio = large[3].clone()
    audio[1, 0, 0] = float("nan")
    step(large[:3] + (audio,) + large[4:])
    r = rep.read()
    audio_path = [i for i, k in enumerate(rep.names) if k.startswith("audio_")]
    print("bad_updates", r.bad_updates, "first", r.last_bad.first, "audio-path tensors with a NaN", int((r.last_bad.nonfinite[audio_path] > 0).sum()), "of", len(audio_path))
    assert r.bad_updates == 1 and audio_path and (r.last_bad.nonfinite[audio_path] > 0).any()
    assert r.last_bad.first in named and r.last_bad.nonfinite[rep.names.index(r.last_bad.first)] > 0
    torch.cuda.synchronize()
    assert not all(bool(torch.isfinite(p).all()) for p in step.fused.keep[0])         # no guard: the update ran on the NaN
