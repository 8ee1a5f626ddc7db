"""Host side of save / resume (facialmmt_amd/step_state.py, checkpoint.save_training / load_training), without a GPU.

* The pure part of the fused update's export, step_state.optimizer_state: bare moments and an update count become a state in the optimizer class's own
  layout -- HFAdamW: transformers.AdamW's (an int `step` per parameter, none in the groups, `lr` a float); torch.optim.AdamW: its state_dict()'s --
  and a fresh optimizer that loads it takes the uninterrupted optimizer's fourth step BIT FOR BIT (parameters (300, 70), (4097,), (5,); fixed gradients).
* save_training -> load_training: every tensor equal, `extra` intact, CPU tensors and builtins only; anything else is refused before a file exists.
* load_state_dict validates before it changes anything: another kind or format and differing betas raise ValueError, a missing model key and a
  mis-shaped moment RuntimeError, and the step's tensors, optimizer state, counter and gradients are afterwards what they were.  Exercised on the eager
  V-only step class over a small CPU module (a step on the CPU has no device generator: `rng` is None)."""
import copy
import types

import pytest
import torch

from facialmmt_amd import checkpoint, step_state
from facialmmt_amd.train_step import HFAdamW, UnimodalStep

SHAPES = [(300, 70), (4097,), (5,)]


def _fixed(seed=11):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(sh, generator=g) for sh in SHAPES]
    grads = [[torch.randn(sh, generator=g) * 0.01 for sh in SHAPES] for _ in range(4)]
    return init, grads


def _make(kind, init):
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    if kind == "hf":
        return ps, HFAdamW(ps, lr=4e-3, weight_decay=0.01)
    return ps, torch.optim.AdamW(ps, lr=4e-3, weight_decay=0.01, betas=(0.9, 0.98), eps=1e-6)


def _steps(ps, opt, grads):
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()


@pytest.mark.parametrize("kind", ["hf", "torch"])
def test_bare_moments_become_the_optimizer_classes_own_layout_and_continue_bit_for_bit(kind):
    init, grads = _fixed()
    ref, opt_r = _make(kind, init)
    _steps(ref, opt_r, grads[:3])
    m = [opt_r.state[p]["exp_avg"].clone() for p in ref]                       # bare values, as FusedClipAdamW.export hands them over
    v = [opt_r.state[p]["exp_avg_sq"].clone() for p in ref]
    mine, opt_m = _make(kind, [p.detach() for p in ref])
    sd = step_state.optimizer_state(opt_m, m, v, 3)
    assert not opt_m.state                                                      # the optimizer is only read
    # the layout
    assert set(sd) == {"state", "param_groups"} and sorted(sd["state"]) == [0, 1, 2] and len(sd["param_groups"]) == 1
    group = sd["param_groups"][0]
    assert type(group["lr"]) is float and group["lr"] == 4e-3 and group["params"] == [0, 1, 2] and "step" not in group
    own = opt_r.hf_state_dict() if kind == "hf" else opt_r.state_dict()
    assert set(group) == set(own["param_groups"][0])
    for i, sh in enumerate(SHAPES):
        assert set(sd["state"][i]) == set(own["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert sd["state"][i]["exp_avg"].shape == torch.Size(sh) and sd["state"][i]["exp_avg"].dtype == torch.float32
        if kind == "hf":
            assert type(sd["state"][i]["step"]) is int and sd["state"][i]["step"] == 3 == own["state"][i]["step"]
        else:
            assert torch.equal(sd["state"][i]["step"], own["state"][i]["step"]) and sd["state"][i]["step"].dtype == own["state"][i]["step"].dtype
    checkpoint._require_plain(sd, "optimizer")
    # a fresh optimizer of the class loads it with the class's own loader and continues
    if kind == "hf":
        opt_m.load_hf_state_dict(copy.deepcopy(sd))
    else:
        opt_m.load_state_dict(copy.deepcopy(sd))
    _steps(ref, opt_r, grads[3:])
    _steps(mine, opt_m, grads[3:])
    for a, b in zip(ref, mine):
        assert torch.equal(a, b)
    for a, b in zip(ref, mine):
        assert torch.equal(opt_r.state[a]["exp_avg"], opt_m.state[b]["exp_avg"]) and torch.equal(opt_r.state[a]["exp_avg_sq"], opt_m.state[b]["exp_avg_sq"])
    # ... and so does the in-place loader the steps use, into an optimizer whose state tensors exist already
    third, opt_t = _make(kind, [p.detach() for p in mine])
    _steps(third, opt_t, grads[:1])
    with torch.no_grad():
        for p, q in zip(third, mine):
            p.copy_(q)
    held = {id(p): {k: t for k, t in opt_t.state[p].items() if torch.is_tensor(t)} for p in third}
    now = step_state.stock_optimizer_state(opt_m)
    step_state.check_optimizer_state(now, opt_t)
    step_state.load_optimizer_state(now, opt_t)
    for p in third:
        assert all(opt_t.state[p][k] is t for k, t in held[id(p)].items())     # filled, not replaced
    more = [[g * 0.5 for g in grads[0]]]
    _steps(mine, opt_m, more)
    _steps(third, opt_t, more)
    for a, b in zip(mine, third):
        assert torch.equal(a, b)


def test_moment_count_must_be_the_optimizers():
    init, _ = _fixed()
    ps, opt = _make("hf", init)
    with pytest.raises(RuntimeError):
        step_state.optimizer_state(opt, [torch.zeros(3)], [torch.zeros(3)], 1)


# ------------------------------------------------------------------------------------------------ the step on the CPU
def _tiny_step(seed, betas=(0.9, 0.999), accumulation=2, with_sched=True):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 3))
    with torch.no_grad():
        model[1].running_mean.uniform_(-1, 1)
        model[1].num_batches_tracked.fill_(seed)
    opt = HFAdamW(model.parameters(), lr=1e-3, betas=betas, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0 / (1 + k)) if with_sched else None
    step = UnimodalStep(model, opt, sched, types.SimpleNamespace(trg_accumulation_steps=accumulation, clip=1.0))
    return step


def _advance(step, n):
    """n micro-steps of the step class's own bookkeeping on a stand-in loss (its forward_loss needs the HIP library)"""
    for i in range(n):
        x = torch.randn(4, 6, generator=torch.Generator().manual_seed(50 + step.i_batch))
        (step.model(x).square().mean() / step.args.trg_accumulation_steps).backward()
        step.i_batch += 1
        if step.i_batch % step.args.trg_accumulation_steps == 0:
            torch.nn.utils.clip_grad_norm_(step.model.parameters(), step.args.clip)
            step.opt.step()
            step.sched.step()
            step.opt.zero_grad(set_to_none=True)


def _everything(step):
    out = {f"model.{k}": v.clone() for k, v in step.model.state_dict().items()}
    for i, p in enumerate(step.model.parameters()):
        out[f"grad.{i}"] = None if p.grad is None else p.grad.clone()
        for k, t in (step.opt.state[p] if p in step.opt.state else {}).items():
            out[f"opt.{i}.{k}"] = t.clone()
    g = step.opt.param_groups[0]
    out["lr"], out["step"], out["i_batch"] = float(g["lr"]), float(g.get("step", 0)), step.i_batch
    out["sched"] = copy.deepcopy({k: v for k, v in step.sched.state_dict().items()})
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_a_cpu_step_round_trips_through_a_file_and_continues(tmp_path):
    src = _tiny_step(1)
    _advance(src, 3)                                                            # one update, then one micro-step of an open window
    state = src.state_dict()
    assert state["format"] == step_state.FORMAT and state["kind"] == "unimodal" and state["i_batch"] == 3 and state["rng"] is None
    assert list(state["models"]) == ["model"] and "1.running_mean" in state["models"]["model"] and "1.num_batches_tracked" in state["models"]["model"]
    assert len(state["window"]) == 6 and all(t.dtype == torch.float32 for t in state["window"])
    assert all(type(st["step"]) is int and st["step"] == 1 for st in state["optimizer"]["state"].values())
    assert type(state["optimizer"]["param_groups"][0]["lr"]) is float
    path = str(tmp_path / "run.pt")
    checkpoint.save_training(path, extra={"epoch": 3, "best_f1": 0.66, "note": "x", "history": [0.5, 0.6]}, unimodal=state)
    states, extra = checkpoint.load_training(path)
    assert extra == {"epoch": 3, "best_f1": 0.66, "note": "x", "history": [0.5, 0.6]} and list(states) == ["unimodal"]
    checkpoint._require_plain(states, "loaded")                                  # no CUDA tensor, no object that is not a builtin

    def equal(a, b, where):
        assert type(a) is type(b), where
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and a.device.type == "cpu" and torch.equal(a, b), where
        elif isinstance(a, dict):
            assert list(a) == list(b), where
            for k in a:
                equal(a[k], b[k], f"{where}[{k!r}]")
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), where
            for i, (x, y) in enumerate(zip(a, b)):
                equal(x, y, f"{where}[{i}]")
        else:
            assert a == b, where
    equal(state, states["unimodal"], "state")
    dst = _tiny_step(2)                                                         # another seed: other weights, other statistics
    held = [p.data_ptr() for p in dst.model.parameters()] + [b.data_ptr() for b in dst.model.buffers()]
    dst.load_state_dict(states["unimodal"])
    assert held == [p.data_ptr() for p in dst.model.parameters()] + [b.data_ptr() for b in dst.model.buffers()]
    _same(_everything(src), _everything(dst))
    _advance(src, 3)
    _advance(dst, 3)
    _same(_everything(src), _everything(dst))


def test_save_training_refuses_what_weights_only_cannot_read(tmp_path):
    path = tmp_path / "bad.pt"
    for bad in ({"state": object()}, {"state": {"t": torch.nn.Parameter(torch.zeros(1))}}, {"state": {("a", 1): 0}}):
        with pytest.raises(TypeError):
            checkpoint.save_training(str(path), **bad)
    with pytest.raises(TypeError):
        checkpoint.save_training(str(path), extra={"when": types.SimpleNamespace()})
    assert not list(tmp_path.iterdir())
    torch.save({"format": 99, "states": {}, "extra": {}}, str(path))
    with pytest.raises(ValueError):
        checkpoint.load_training(str(path))


def _tampered(state, how):
    s = copy.deepcopy(state)
    if how == "kind":
        s["kind"] = "aux"
    elif how == "format":
        s["format"] = step_state.FORMAT + 1
    elif how == "missing model key":
        del s["models"]["model"]["1.running_var"]
    elif how == "unexpected model key":
        s["models"]["model"]["extra.weight"] = torch.zeros(1)
    elif how == "mis-shaped parameter":
        s["models"]["model"]["0.weight"] = torch.zeros(5, 7)
    elif how == "mis-shaped moment":
        s["optimizer"]["state"][0]["exp_avg_sq"] = torch.zeros(5, 7)
    elif how == "parameter count":
        s["optimizer"]["param_groups"][0]["params"] = [0, 1, 2, 3]
    elif how == "betas":
        s["optimizer"]["param_groups"][0]["betas"] = (0.9, 0.98)
    elif how == "eps":
        s["optimizer"]["param_groups"][0]["eps"] = 1e-8
    elif how == "weight_decay":
        s["optimizer"]["param_groups"][0]["weight_decay"] = 0.0
    elif how == "correct_bias":
        s["optimizer"]["param_groups"][0]["correct_bias"] = False
    elif how == "window missing":
        del s["window"]
    elif how == "window shape":
        s["window"][1] = torch.zeros(6)
    elif how == "top-level key":
        del s["scheduler"]
    return s


@pytest.mark.parametrize("how,error", [("kind", ValueError), ("format", ValueError), ("missing model key", RuntimeError), ("unexpected model key", RuntimeError),
                                       ("mis-shaped parameter", RuntimeError), ("mis-shaped moment", RuntimeError), ("parameter count", RuntimeError),
                                       ("betas", ValueError), ("eps", ValueError), ("weight_decay", ValueError), ("correct_bias", ValueError),
                                       ("window missing", RuntimeError), ("window shape", RuntimeError), ("top-level key", RuntimeError)])
def test_validation_raises_before_anything_changes(how, error):
    src = _tiny_step(1)
    _advance(src, 3)
    state = src.state_dict()
    dst = _tiny_step(2)
    _advance(dst, 5)                                                            # a live target: moments, an open window, a moved schedule
    before = _everything(dst)
    with pytest.raises(error) as info:
        dst.load_state_dict(_tampered(state, how))
    _same(before, _everything(dst))
    if how in step_state.HYPER:
        assert f"`{how}`" in str(info.value) and "launch arguments" in str(info.value)
    dst.load_state_dict(state)                                                  # the untampered state still loads into the same step
    _same(_everything(src), _everything(dst))


def test_fused_load_from_refuses_other_hyper_parameters_without_a_gpu():
    """FusedClipAdamW.load_from compares the loaded group with the values its (captured) update holds before it copies anything: shown on an object
    assembled by hand, since the constructor needs a device"""
    from facialmmt_amd.train_step import FusedClipAdamW
    p = torch.nn.Parameter(torch.zeros(3))
    fused = FusedClipAdamW.__new__(FusedClipAdamW)
    fused.b1, fused.b2, fused.eps, fused.wd = 0.9, 0.999, 1e-6, 0.01
    fused.keep, fused.m, fused.v, fused.step = ([p], [None]), [torch.ones(3)], [torch.ones(3)], torch.ones(())
    ok = dict(betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
    for field, value in (("betas", (0.9, 0.98)), ("eps", 1e-8), ("weight_decay", 0.0)):
        opt = types.SimpleNamespace(param_groups=[dict(ok, **{field: value})], state={p: {"exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3), "step": 2}})
        with pytest.raises(ValueError, match=field):
            fused.load_from(opt)
        assert float(fused.m[0].sum()) == 3.0 and float(fused.step) == 1.0
    fused.load_from(types.SimpleNamespace(param_groups=[ok], state={p: {"exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3), "step": 2}}))
    assert float(fused.m[0].sum()) == 0.0 and float(fused.step) == 2.0
    m, v, n = fused.export()
    assert n == 2 and torch.equal(m[0], torch.zeros(3)) and m[0] is not fused.m[0]


def test_counters_that_disagree_are_refused_by_the_check_where_the_fused_update_would_load_them():
    """torch.optim.AdamW skips a parameter without a gradient, so an eager state can hold differing per-parameter counters; the fused update has one
    counter: the check refuses such a state (before anything is copied) when `fused` is in use, and lets the optimizer that keeps them take it"""
    init, grads = _fixed()
    ps, opt = _make("torch", init)
    _steps(ps, opt, grads[:1])
    ps[0].grad, ps[1].grad, ps[2].grad = grads[1][0].clone(), grads[1][1].clone(), None
    opt.step()
    sd = step_state.stock_optimizer_state(opt)
    assert {float(s["step"]) for s in sd["state"].values()} == {1.0, 2.0}
    step_state.check_optimizer_state(sd, opt)
    with pytest.raises(ValueError, match="counters disagree"):
        step_state.check_optimizer_state(sd, opt, fused=object())


def test_a_model_entry_that_is_no_tensor_is_a_runtime_error():
    src = _tiny_step(1)
    state = src.state_dict()
    state["models"]["model"]["0.bias"] = 3
    before = _everything(src)
    with pytest.raises(RuntimeError, match="0.bias"):
        src.load_state_dict(state)
    _same(before, _everything(src))
