"""GPU tests of state_dict() / load_state_dict() on the training steps (facialmmt_amd/step_state.py): a stopped run continues with the BITS of the
uninterrupted one.

Recipe: run A is the uninterrupted run of n + m micro-steps.  Run B does n, takes state_dict(), and the state goes through a file
(checkpoint.save_training / load_training).  A FRESH model filled from ANOTHER seed gets a fresh optimizer (and scheduler), a new capture -- with the
device generator somewhere else -- and load_state_dict, then runs the m remaining micro-steps.  Compared with torch.equal unless a test says otherwise.

 1. V-only, bf16, dropout 0.1, fused HFAdamW, LambdaLR, accumulation 2, n = m = 3 (saved inside a window); plus: a state with another generator state
    gives other losses, a state with a zeroed window other parameters (a loader that ignored either would pass without these).
 2. The same with train_step.FUSED_ADAMW off: the captured torch.optim.AdamW(capturable=True) keeps its state tensors where they are.
 3. Eager <-> graphed, noise-free fp32: the moments arrive bit for bit; two more micro-steps on both sides at the bars of tests/test_gpu_unimodal_step.py
    (losses 2e-4 of max(1, |loss|), parameters 1e-4 of max(1, max|p|)); Adam at lr 1e-3, eps 1e-6, one update behind the load -- the argument of
    tests/test_gpu_short_batch.py for holding Adam to the SGD bar covers two updates from differing moments, here one from identical ones.
 4. Auxiliary step, 8 images, DropPath at the model's rate, fused AdamW, n = m = 2: also the head's BatchNorm statistics.
 5. T+A+V, frame_capacity (8, 12), pad_rows, hidden dropout 0.1, Gumbel-softmax at tau = 1, fused HFAdamW, accumulation 2: [3, 4], [6, 5], a one-row
    short batch, then [6, 6] behind the save.  The control -- two uninterrupted constructions give equal bits, one of them with a state_dict() taken
    on the way -- is asserted first.  And a MasterWeights text encoder: the masters return bit for bit, the bf16 module holds their rounding.
 6. The restrictions raise and leave the step alone."""
import copy
import types

import pytest
import torch

from facialmmt_amd import checkpoint, synth
from tests import test_gpu_ragged_buckets as RB
from tests import test_gpu_short_batch as SB
from tests import test_gpu_unimodal_step as US

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _schedule(opt):
    """linear warm-up over 3 updates, linear decay to 0 at update 10"""
    return torch.optim.lr_scheduler.LambdaLR(opt, lambda k: (k + 1) / 3.0 if k < 2 else max(0.0, (10 - k) / 8.0))


def _through_a_file(tmp_path, **states):
    path = str(tmp_path / "run.pt")
    checkpoint.save_training(path, extra={"epoch": 1, "best_f1": 0.5}, **states)
    got, extra = checkpoint.load_training(path)
    assert extra == {"epoch": 1, "best_f1": 0.5} and list(got) == list(states)
    return got


def _moments(step):
    """{name: tensor} of the optimizer state wherever it lives: FusedClipAdamW, or optimizer.state of the captured optimizer.step()"""
    if step.fused is not None:
        out = {f"m{i}": t for i, t in enumerate(step.fused.m)}
        out.update({f"v{i}": t for i, t in enumerate(step.fused.v)})
        out["step"] = step.fused.step
        return out
    out = {}
    for i, p in enumerate(step.opt.param_groups[0]["params"]):
        out.update({f"{k}{i}": t for k, t in step.opt.state[p].items() if torch.is_tensor(t)})
    if torch.is_tensor(step.opt.param_groups[0].get("step")):
        out["step"] = step.opt.param_groups[0]["step"]
    return out


def _equal(label, a, b):
    assert a.keys() == b.keys(), label
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (label, bad[:8], len(bad), len(a))


# ------------------------------------------------------------------------------------------------ 1, 2: V-only
def _v_make(dev, fused, model_seed, generator_seed):
    from facialmmt_amd.train_step import GraphedUnimodalStep, HFAdamW
    dtype = torch.bfloat16 if fused else torch.float32
    cfg, model = US.build(dev, accumulation=2, dtype=dtype, dropout=0.1, seed=model_seed)
    torch.manual_seed(generator_seed)
    lr = torch.tensor(1e-3, device=dev)
    if fused:
        opt = HFAdamW(model.parameters(), lr=lr, weight_decay=0.01)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=0.01, eps=1e-6, capturable=True)
    sched = _schedule(opt)
    step = GraphedUnimodalStep(model, opt, sched, cfg, US.micro_batch(dev, 20), autocast_dtype=torch.bfloat16 if fused else None)
    assert (step.fused is not None) == fused
    return types.SimpleNamespace(step=step, model=model, opt=opt, sched=sched, lr=lr)


def _v_end(r, dev):
    torch.cuda.synchronize()
    out = {f"p.{k}": p.detach().clone() for k, p in r.model.named_parameters()}
    out.update({f"o.{k}": t.detach().clone() for k, t in _moments(r.step).items()})
    out["lr"] = r.lr.clone()
    out["last_epoch"] = torch.tensor(r.sched.last_epoch)
    out["rng"] = torch.cuda.get_rng_state(dev)
    return out


def _v_resume(dev, tmp_path, fused):
    batches = [US.micro_batch(dev, 20 + i) for i in range(6)]
    a = _v_make(dev, fused, 201, 99)
    losses_a = torch.stack([a.step(b).clone() for b in batches])
    end_a = _v_end(a, dev)
    b = _v_make(dev, fused, 201, 99)
    losses_b = torch.stack([b.step(x).clone() for x in batches[:3]])
    state = b.step.state_dict()
    assert torch.equal(losses_a[:3], losses_b)
    assert state["kind"] == "unimodal" and state["i_batch"] == 3 and len(state["window"]) == len(list(b.model.parameters()))
    assert any(float(w.abs().max()) > 0 for w in state["window"])
    # today's silent loss: the saved optimizer state HAS the moments of the one update so far, in the class's layout, and optimizer.state is as it was
    saved = state["optimizer"]["state"]
    assert sorted(saved) == list(range(len(list(b.model.parameters()))))
    assert all(float(s["step"]) == 1.0 and float(s["exp_avg"].abs().max()) > 0 and float(s["exp_avg_sq"].max()) > 0 for s in saved.values())
    assert type(state["optimizer"]["param_groups"][0]["lr"]) is float
    if fused:
        assert not b.step.opt.state and all(type(s["step"]) is int for s in saved.values())
    loaded = _through_a_file(tmp_path, unimodal=state)["unimodal"]
    c = _v_make(dev, fused, 555, 1234)                                           # other weights, the generator elsewhere, a new capture
    assert not torch.equal(next(c.model.parameters()), next(b.model.parameters()))
    held = [c.lr.data_ptr()] + [p.data_ptr() for p in c.model.parameters()] + [t.data_ptr() for t in _moments(c.step).values()]
    c.step.load_state_dict(loaded)
    assert held == [c.lr.data_ptr()] + [p.data_ptr() for p in c.model.parameters()] + [t.data_ptr() for t in _moments(c.step).values()]
    assert c.opt.param_groups[0]["lr"] is c.lr and c.step.i_batch == 3 and (not fused or not c.opt.state)
    losses_c = torch.stack([c.step(x).clone() for x in batches[3:]])
    end_c = _v_end(c, dev)
    print(f"losses uninterrupted {losses_a.tolist()} resumed {losses_c.tolist()} lr {float(end_a['lr'])} / {float(end_c['lr'])}")
    assert torch.isfinite(losses_a).all() and len(set(losses_a.tolist())) == 6
    assert torch.equal(losses_a[3:], losses_c)
    _equal("V-only, resumed against uninterrupted", end_a, end_c)
    assert int(end_a["last_epoch"]) == 3 and float(end_a["o.step" if fused else "o.step0"]) == 3.0
    return batches, loaded, c, losses_a, end_a


def test_unimodal_fused_resume_inside_a_window_walks_the_uninterrupted_bits(dev, tmp_path):
    batches, loaded, c, losses_a, end_a = _v_resume(dev, tmp_path, fused=True)
    # sensitivity, on the same constructed step: another generator state -> other dropout masks -> other losses
    torch.manual_seed(4321)
    other = dict(loaded, rng=torch.cuda.get_rng_state(dev))
    assert not torch.equal(other["rng"], loaded["rng"])
    c.step.load_state_dict(other)
    losses_r = torch.stack([c.step(x).clone() for x in batches[3:]])
    torch.cuda.synchronize()
    assert not torch.equal(losses_r, losses_a[3:])
    # ... and a window that lost its first micro-step -> another update -> other parameters
    c.step.load_state_dict(dict(loaded, window=[torch.zeros_like(w) for w in loaded["window"]]))
    for x in batches[3:]:
        c.step(x)
    end_w = _v_end(c, dev)
    assert torch.equal(end_w["rng"], end_a["rng"]) and torch.equal(end_w["lr"], end_a["lr"])
    differ = [k for k in end_a if k.startswith("p.") and not torch.equal(end_a[k], end_w[k])]
    assert len(differ) > 0.5 * len([k for k in end_a if k.startswith("p.")])


def test_unimodal_stock_capturable_optimizer_resumes_in_place(dev, tmp_path, monkeypatch):
    from facialmmt_amd import train_step
    monkeypatch.setattr(train_step, "FUSED_ADAMW", False)
    _, _, c, _, _ = _v_resume(dev, tmp_path, fused=False)
    assert c.step.fused is None and len(c.opt.state) == len(list(c.model.parameters()))


# ------------------------------------------------------------------------------------------------ 3: eager <-> graphed
def _v_plain(dev, graphed, model_seed):
    from facialmmt_amd.train_step import GraphedUnimodalStep, HFAdamW, UnimodalStep
    cfg, model = US.build(dev, accumulation=2, dropout=0.0, seed=model_seed)
    if graphed:
        opt = HFAdamW(model.parameters(), lr=torch.tensor(1e-3, device=dev), weight_decay=0.01)
        step = GraphedUnimodalStep(model, opt, None, cfg, US.micro_batch(dev, 40))
        assert step.fused is not None
    else:
        opt = HFAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        step = UnimodalStep(model, opt, None, cfg)
    return step, model, opt


@pytest.mark.parametrize("direction", ["graphed_to_eager", "eager_to_graphed"])
def test_a_state_moves_between_the_eager_and_the_graphed_step(dev, tmp_path, direction):
    batches = [US.micro_batch(dev, 40 + i) for i in range(5)]
    src, src_model, src_opt = _v_plain(dev, direction == "graphed_to_eager", 201)
    for b in batches[:3]:
        src(b)
    state = _through_a_file(tmp_path, unimodal=src.state_dict())["unimodal"]
    assert state["i_batch"] == 3 and "window" in state
    dst, dst_model, dst_opt = _v_plain(dev, direction == "eager_to_graphed", 555)
    dst.load_state_dict(state)
    torch.cuda.synchronize()
    graphed, eager_opt = (src, dst_opt) if direction == "graphed_to_eager" else (dst, src_opt)
    assert not graphed.opt.state and float(graphed.fused.step) == 1.0 == float(eager_opt.param_groups[0]["step"])
    for i, p in enumerate(eager_opt.param_groups[0]["params"]):
        assert torch.equal(eager_opt.state[p]["exp_avg"], graphed.fused.m[i]) and torch.equal(eager_opt.state[p]["exp_avg_sq"], graphed.fused.v[i]), i
        assert float(graphed.fused.v[i].max()) > 0
    for p, q in zip(src_model.parameters(), dst_model.parameters()):
        assert torch.equal(p, q)
    want = [float(src(b)) for b in batches[3:]]
    got = [float(dst(b)) for b in batches[3:]]
    torch.cuda.synchronize()
    print(f"{direction}: losses source {want} destination {got}")
    for a, b in zip(want, got):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (want, got)
    assert src.i_batch == dst.i_batch == 5
    moved = sum(int(not torch.equal(p, q)) for p, q in zip(src_model.parameters(), US.build(dev, seed=201)[1].parameters()))
    assert moved > 0.9 * len(list(src_model.parameters()))
    SB._close(f"{direction}: parameters after the update behind the load", dict(src_model.named_parameters()), dict(dst_model.named_parameters()), 1e-4)


# ------------------------------------------------------------------------------------------------ 4: auxiliary
def _aux_make(dev, images, labels, model_seed, generator_seed):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    from facialmmt_amd.train_step import GraphedAuxStep, HFAdamW
    cfg = default_args(aux_accumulation_steps=1)
    swin = models.SwinForAffwildClassification(cfg)
    synth.fill_state_dict(swin, seed=model_seed)
    swin.to(dev).train()
    assert any(getattr(m, "drop_prob", 0.0) > 0.0 for m in swin.modules())          # DropPath at the model's default rate
    torch.manual_seed(generator_seed)
    opt = HFAdamW(swin.parameters(), lr=torch.tensor(1e-4, device=dev), weight_decay=0.01)
    step = GraphedAuxStep(swin, opt, None, cfg, images[:8], labels[:8])
    assert step.fused is not None
    return step, swin


def _aux_end(step, swin):
    torch.cuda.synchronize()
    out = {f"p.{k}": p.detach().clone() for k, p in swin.named_parameters()}
    out.update({f"o.{k}": t.detach().clone() for k, t in _moments(step).items()})
    bn = swin.swin.output_layer[3]
    out.update(mean=bn.running_mean.clone(), var=bn.running_var.clone(), tracked=bn.num_batches_tracked.clone())
    return out


def test_auxiliary_step_resumes_with_droppath_and_batchnorm_statistics(dev, tmp_path):
    images, labels = SB._aux(dev, 16)
    feed = [(images[8 * (i % 2):8 * (i % 2) + 8], labels[8 * (i % 2):8 * (i % 2) + 8]) for i in range(4)]
    a, swin_a = _aux_make(dev, images, labels, 100, 31)
    losses_a = torch.stack([a(*x).clone() for x in feed])
    end_a = _aux_end(a, swin_a)
    b, swin_b = _aux_make(dev, images, labels, 100, 31)
    for x in feed[:2]:
        b(*x)
    state = _through_a_file(tmp_path, aux=b.state_dict())["aux"]
    assert state["kind"] == "aux" and state["i_batch"] == 2 and "window" not in state and not b.opt.state
    c, swin_c = _aux_make(dev, images, labels, 321, 77)
    c.load_state_dict(state)
    losses_c = torch.stack([c(*x).clone() for x in feed[2:]])
    end_c = _aux_end(c, swin_c)
    print(f"auxiliary losses uninterrupted {losses_a.tolist()} resumed {losses_c.tolist()}")
    assert len(set(losses_a.tolist())) == 4 and int(end_a["tracked"]) == 4
    assert torch.equal(losses_a[2:], losses_c)
    _equal("auxiliary, resumed against uninterrupted", end_a, end_c)


# ------------------------------------------------------------------------------------------------ 5: T+A+V
def _target_make(dev, sample_counts, other_seed=False, generator_seed=7, masters=False, frame_capacity=RB.BUCKETS):
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, step_parameters
    cfg, swin, mm = RB._models(dev, 2, hidden_dropout=0.1)
    cfg.tau = swin.tau = 1.0                                                     # Gumbel noise matters
    if other_seed:
        synth.fill_state_dict(swin, seed=101)
        synth.fill_state_dict(mm, seed=202)
    mw = MasterWeights(mm.roberta, torch.bfloat16) if masters else None
    torch.manual_seed(generator_seed)
    opt = HFAdamW(step_parameters(mm, mw), lr=torch.tensor(1e-3, device=dev), weight_decay=0.01)
    step = GraphedTargetStep(swin, mm, opt, None, cfg, RB._batches(dev, cfg, sample_counts)[0], autocast_dtype=None, masters=mw,
                             frame_capacity=frame_capacity, pad_rows=True)
    assert step.fused is not None
    return types.SimpleNamespace(step=step, swin=swin, mm=mm, cfg=cfg, masters=mw)


def _target_end(r, losses, kept):
    torch.cuda.synchronize()
    out = {f"p.{k}": p.detach().clone() for k, p in r.mm.named_parameters()}
    out.update({f"o.{k}": t.detach().clone() for k, t in _moments(r.step).items()})
    bn = r.swin.swin.output_layer[3]
    out.update(mean=bn.running_mean.clone(), var=bn.running_var.clone(), tracked=bn.num_batches_tracked.clone())
    out["losses"] = torch.stack(losses)
    out.update({f"kept{i}": k for i, k in enumerate(kept)})
    return out


def _target_feed(dev, cfg):
    full = [RB._batches(dev, cfg, n)[0] for n in ([3, 4], [6, 5], [4, 2], [6, 6])]
    return [full[0], full[1], SB._short(full[2], 1), full[3]]


def _target_calls(r, feed, first=0, save_after=None):
    losses, kept, state = [], [], None
    for i, batch in enumerate(feed):
        loss, k = r.step(batch)
        losses.append(loss.clone())
        kept.append(k.clone())
        if save_after is not None and first + i + 1 == save_after:
            state = r.step.state_dict()
    return losses, kept, state


def test_target_step_resumes_across_capacities_and_a_short_batch(dev, tmp_path):
    a = _target_make(dev, [3, 4])
    feed = _target_feed(dev, a.cfg)
    la, ka, _ = _target_calls(a, feed)
    end_a = _target_end(a, la, ka)
    assert a.step.replays == {8: 2, 12: 2} and a.step.padded_calls == 1
    b = _target_make(dev, [3, 4])
    lb, kb, state = _target_calls(b, feed, save_after=3)                          # a state_dict() taken on the way changes nothing
    end_b = _target_end(b, lb, kb)
    print(f"T+A+V losses, two uninterrupted constructions: {end_a['losses'].tolist()} / {end_b['losses'].tolist()}")
    assert torch.isfinite(end_a["losses"]).all() and all(float(k.sum()) > 0 for k in ka)
    _equal("T+A+V control: two uninterrupted constructions", end_a, end_b)
    assert state["kind"] == "target" and state["i_batch"] == 3 and "window" in state and sorted(state["models"]) == ["mm", "swin"]
    state = _through_a_file(tmp_path, target=state)["target"]
    c = _target_make(dev, [6, 5], other_seed=True, generator_seed=1234)
    held = [p.data_ptr() for m in (c.swin, c.mm) for p in list(m.parameters()) + list(m.buffers())]
    c.step.load_state_dict(state)
    assert held == [p.data_ptr() for m in (c.swin, c.mm) for p in list(m.parameters()) + list(m.buffers())] and not c.step.opt.state
    lc, kc, _ = _target_calls(c, feed[3:], first=3)
    end_c = _target_end(c, la[:3] + lc, ka[:3] + kc)
    print(f"T+A+V loss of the call behind the save: uninterrupted {float(la[3])} resumed {float(lc[0])}")
    _equal("T+A+V, resumed against uninterrupted", end_a, end_c)
    for (k, p), (_, q) in zip(a.swin.state_dict().items(), c.swin.state_dict().items()):
        assert torch.equal(p, q), k                                              # Swin is not stepped here: the loaded weights, the walked statistics


def test_master_weights_return_bit_for_bit_and_the_module_holds_their_rounding(dev):
    r = _target_make(dev, [3, 4], masters=True, frame_capacity=12)
    feed = _target_feed(dev, r.cfg)
    r.step(feed[0])
    state = r.step.state_dict()                                                  # inside a window, before the first update
    keys = [k for k, p in r.mm.named_parameters() if k.startswith("roberta.")]
    assert keys and all(state["models"]["mm"][k].dtype == torch.float32 for k in keys)
    assert all(p.dtype == torch.bfloat16 for k, p in r.mm.named_parameters() if k.startswith("roberta."))
    saved = [m.detach().clone() for m in r.masters.masters]
    for k, (low, m) in zip(keys, r.masters.pairs()):
        assert torch.equal(state["models"]["mm"][k], m.detach().cpu()), k
    r.step(feed[1])                                                              # the update moves the masters
    torch.cuda.synchronize()
    assert any(not torch.equal(s, m) for s, m in zip(saved, r.masters.masters))
    held = [m.data_ptr() for m in r.masters.masters] + [low.data_ptr() for low, _ in r.masters.pairs()]
    r.step.load_state_dict(state)
    torch.cuda.synchronize()
    assert held == [m.data_ptr() for m in r.masters.masters] + [low.data_ptr() for low, _ in r.masters.pairs()]
    for s, (low, m) in zip(saved, r.masters.pairs()):
        assert torch.equal(m, s) and low.dtype == torch.bfloat16 and torch.equal(low, s.to(torch.bfloat16))
    assert r.step.i_batch == 1 and float(r.step.fused.step) == 0.0
    loss, kept = r.step(feed[1])
    assert torch.isfinite(loss) and float(kept.sum()) > 0


# ------------------------------------------------------------------------------------------------ 6: restrictions
def test_restrictions_raise_and_leave_the_step_alone(dev):
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW
    cfg, swin, mm = RB._models(dev, 1)
    _, compact = RB._batches(dev, cfg, [3, 4])
    opt = HFAdamW(mm.parameters(), lr=torch.tensor(1e-3, device=dev), weight_decay=0.01)
    step = GraphedTargetStep(swin, mm, opt, None, cfg, compact, autocast_dtype=None, pipeline_swin=True)
    step(compact, next_batch=compact)
    with pytest.raises(ValueError, match="next_batch=None"):
        step.state_dict()                                                        # the prefetched forward has drawn its noise
    step(compact)
    state = step.state_dict()
    assert state["i_batch"] == 2 and "window" not in state
    torch.cuda.synchronize()
    before = {k: v.detach().clone() for m in (swin, mm) for k, v in m.state_dict().items()}
    before.update({f"o.{k}": t.detach().clone() for k, t in _moments(step).items()})
    other = copy.deepcopy(state)
    other["optimizer"]["param_groups"][0]["betas"] = (0.9, 0.98)
    with pytest.raises(ValueError, match="betas.*launch arguments"):
        step.load_state_dict(other)
    with pytest.raises(ValueError, match="kind"):
        step.load_state_dict(dict(state, kind="aux"))
    with pytest.raises(ValueError, match="format"):
        step.load_state_dict(dict(state, format=0))
    short = copy.deepcopy(state)
    del short["models"]["swin"]["classifier.bias"]
    with pytest.raises(RuntimeError, match="classifier.bias"):
        step.load_state_dict(short)
    active = types.SimpleNamespace(active=True)
    real, step.tail.flat = step.tail.flat, active
    with pytest.raises(NotImplementedError):
        step.state_dict()
    with pytest.raises(NotImplementedError):
        step.load_state_dict(state)
    step.tail.flat = real
    torch.cuda.synchronize()
    after = {k: v for m in (swin, mm) for k, v in m.state_dict().items()}
    after.update({f"o.{k}": t for k, t in _moments(step).items()})
    _equal("a refused state leaves the step alone", before, after)
    assert step.i_batch == 2
    step(compact, next_batch=compact)
    step.load_state_dict(state)                                                  # clears the prefetch
    assert step.prefetched is None and step.i_batch == 2
