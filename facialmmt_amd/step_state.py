"""Save and resume of a training step (train_step's six step classes): what `state_dict()` / `load_state_dict()` of a step hold and how a state is
checked before anything is changed.  Host code only: nothing here launches a kernel, and nothing a replay executes changes.

A step's state is a nested dict of CPU tensors and builtins (a file of it loads with torch.load(weights_only=True), checkpoint.save_training):

  format     FORMAT
  kind       "target" | "aux" | "unimodal"
  models     {attribute name of the step: state_dict of that model}, buffers included; where the step runs a sub-module through MasterWeights the
             fp32 master values stand in place of the rounded bf16 ones (MasterWeights.state_dict_fp32's content)
  optimizer  the optimizer class's OWN layout (HFAdamW: hf_state_dict(), i.e. transformers.AdamW's, an int `step` per parameter; anything else:
             state_dict()), `lr` by value.  With the fused update the moments and the counter come out of FusedClipAdamW (optimizer_state)
  scheduler  scheduler.state_dict() on the host, or None
  i_batch    the micro-step counter
  window     only inside an accumulation window (i_batch % accumulation_steps != 0): one fp32 tensor per optimizer parameter, in the optimizer's
             order -- the gradients accumulated so far (graphed: the flat views; eager: p.grad, zeros where there is none).  The common layout is
             what lets a state move between an eager and a graphed step
  rng        torch.cuda.get_rng_state(device): the generator behind DropPath, Gumbel noise and every dropout seed drawn inside the graphs (None for
             a step on the CPU)

Loading copies VALUES into the tensors that exist -- every tensor a captured graph addresses keeps its address -- and validates everything first:
a state that does not fit raises and leaves the step and its models untouched."""
from __future__ import annotations

import types

import torch

from .graph_capture import _bump_versions

FORMAT = 1
KINDS = ("target", "aux", "unimodal")
HYPER = ("betas", "eps", "weight_decay", "correct_bias")
LAUNCH_ARGUMENTS = ("a captured update holds betas, eps, weight decay and correct_bias as launch arguments, so a loaded value cannot take effect: "
                    "build the step's optimizer with the checkpoint's values")


# ------------------------------------------------------------------------------------------------ plain host data
def to_host(obj):
    """`obj` with every tensor as a detached CPU tensor of its own (copied tensor by tensor), mappings as plain dicts, lists and tuples kept;
    TypeError for anything that is not a tensor or a builtin (a file of the result must load with weights_only=True)"""
    if torch.is_tensor(obj):
        t = obj.detach()
        return t.clone() if t.device.type == "cpu" else t.to("cpu")
    if isinstance(obj, dict):
        for k in obj:
            if not isinstance(k, (str, int)):
                raise TypeError(f"key {k!r} of a state is {type(k).__name__}, not a str or an int")
        return {k: to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_host(v) for v in obj) if type(obj) in (list, tuple) else [to_host(v) for v in obj]
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    raise TypeError(f"a step state holds tensors and builtins only, got {type(obj).__name__}")


def _like(live, saved):
    """`saved` with its tensors on the devices of the matching tensors of `live` (a scheduler keeps its base learning rates where the optimizer's are)"""
    if torch.is_tensor(saved):
        if isinstance(live, (int, float)) and saved.numel() == 1:
            return type(live)(saved.item())                  # a state from a step with a device learning rate into one with a float
        return saved.to(live.device, copy=True) if torch.is_tensor(live) else saved.clone()
    if isinstance(saved, dict):
        return {k: _like(live.get(k) if isinstance(live, dict) else None, v) for k, v in saved.items()}
    if isinstance(saved, (list, tuple)):
        pair = live if isinstance(live, (list, tuple)) and len(live) == len(saved) else [None] * len(saved)
        return type(saved)(_like(l, s) for l, s in zip(pair, saved))
    return saved


# ------------------------------------------------------------------------------------------------ optimizer: export
def _is_hf(opt):
    return hasattr(opt, "hf_state_dict")                    # train_step.HFAdamW: transformers.AdamW's layout


def optimizer_params(opt):
    return [p for g in opt.param_groups for p in g["params"]]


def _host_groups(opt):
    """the optimizer's param_groups as its state_dict() numbers them, tensors by value (`lr` on the device: a float), HFAdamW's group counter left out"""
    groups = []
    for g in opt.state_dict()["param_groups"]:
        g = dict(g)
        if _is_hf(opt):
            g.pop("step", None)
        groups.append({k: (float(v) if torch.is_tensor(v) and v.numel() == 1 else to_host(v)) for k, v in g.items()})
    return groups


def optimizer_state(opt, m, v, step):
    """The pure part of the fused update's export: bare first / second moments (one tensor per optimizer parameter, in the optimizer's order) and the
    update count -> a state in `opt`'s own layout.  HFAdamW: transformers.AdamW's (exp_avg, exp_avg_sq and an int `step` per parameter, none in the
    groups); torch.optim.AdamW: its state_dict()'s (`step` a 0-dim fp32 tensor per parameter).  `lr` is a float.  `opt` is only read."""
    groups = _host_groups(opt)
    n = sum(len(g["params"]) for g in groups)
    if len(m) != n or len(v) != n:
        raise RuntimeError(f"optimizer_state: {len(m)} / {len(v)} moments for the optimizer's {n} parameters")
    state = {}
    for g in groups:
        for i in g["params"]:
            count = int(step) if _is_hf(opt) else torch.tensor(float(step), dtype=torch.float32)
            state[i] = {"step": count, "exp_avg": to_host(m[i]), "exp_avg_sq": to_host(v[i])}
    return {"state": state, "param_groups": groups}


def stock_optimizer_state(opt):
    """the state of an optimizer that keeps it itself (eager steps, the captured `optimizer.step()`), on the host, in its class's layout"""
    sd = opt.hf_state_dict() if _is_hf(opt) else opt.state_dict()
    return {"state": to_host(sd["state"]), "param_groups": _host_groups(opt)}


# ------------------------------------------------------------------------------------------------ optimizer: check, then load in place
def _hyper_value(k, v):
    if k == "betas":
        return tuple(float(b) for b in v)
    return bool(v) if k == "correct_bias" else float(v)


def check_hyper(saved, live, who="load_state_dict"):
    """betas / eps / weight decay / correct_bias of a loaded group against the live one: ValueError naming the first field that differs"""
    for k in HYPER:
        if k not in live:
            continue
        if k not in saved or _hyper_value(k, saved[k]) != _hyper_value(k, live[k]):
            raise ValueError(f"{who}: `{k}` of the loaded optimizer state is {saved.get(k)!r}, the step was built with {live[k]!r}; {LAUNCH_ARGUMENTS}")


_GROUP_FREE = ("params", "lr", "initial_lr", "step") + HYPER


def check_optimizer_state(sd, opt, who="load_state_dict", fused=None):
    """A saved optimizer state against the live optimizer, nothing changed: RuntimeError for another layout, parameter count or moment shape,
    ValueError for differing hyper-parameters (check_hyper) or per-parameter counters that disagree where one counter serves them all: a group
    of HFAdamW, and every parameter of the fused update (`fused`: torch.optim.AdamW skips a parameter without a gradient, so an eager state of
    its can hold differing counters; FusedClipAdamW.load_from would refuse it only after the models had been overwritten)"""
    every = set()
    if not isinstance(sd, dict) or set(sd) != {"state", "param_groups"}:
        raise RuntimeError(f"{who}: an optimizer state holds 'state' and 'param_groups'")
    if len(sd["param_groups"]) != len(opt.param_groups):
        raise RuntimeError(f"{who}: {len(sd['param_groups'])} parameter groups loaded, the optimizer has {len(opt.param_groups)}")
    caller = who
    for j, (gs, g) in enumerate(zip(sd["param_groups"], opt.param_groups)):
        who = f"{caller}, group {j}" if len(opt.param_groups) > 1 else caller      # several groups: every message below names its group
        if len(gs["params"]) != len(g["params"]):
            raise RuntimeError(f"{who}: the loaded optimizer state is for {len(gs['params'])} parameters, the optimizer steps {len(g['params'])}")
        other = set(gs).symmetric_difference(g) - set(_GROUP_FREE)
        if other:
            raise RuntimeError(f"{who}: the loaded state is not in {type(opt).__name__}'s layout (group keys {sorted(other)})")
        check_hyper(gs, g, who)
        counts = set()
        for p, i in zip(g["params"], gs["params"]):
            src = sd["state"].get(i, {})
            live = opt.state[p] if p in opt.state else {}
            for k, t in src.items():
                if torch.is_tensor(t) and t.dim() > 0:
                    if tuple(t.shape) != tuple(p.shape):
                        raise RuntimeError(f"{who}: `{k}` of parameter {i} has shape {tuple(t.shape)}, the parameter {tuple(p.shape)}")
                    if live and k not in live:
                        raise RuntimeError(f"{who}: the optimizer keeps no `{k}` for parameter {i}")
                elif k == "step":
                    counts.add(float(t))
            if "step" in src and _is_hf(opt) == torch.is_tensor(src["step"]):
                raise RuntimeError(f"{who}: the loaded state is not in {type(opt).__name__}'s layout (`step` of parameter {i})")
        if _is_hf(opt) and len(counts) > 1:
            raise ValueError(f"{who}: per-parameter step counters of one group disagree: {sorted(counts)}")
        every |= counts
    if fused is not None and len(every) > 1:
        raise ValueError(f"{caller}: per-parameter step counters disagree: {sorted(every)}; the fused update keeps one counter for all parameters of all groups")


def _place(k, t, p, group):
    if not torch.is_tensor(t):
        return t
    if t.dim() == 0 and k == "step" and not (group.get("capturable") or group.get("fused")):
        return t.clone()                                    # torch keeps the counter of a plain AdamW on the host
    return t.to(p.device, copy=True)


@torch.no_grad()
def load_optimizer_state(sd, opt, fused=None):
    """A checked state into the live optimizer, IN PLACE: a tensor `optimizer.state` already holds is filled (a captured `optimizer.step()` addresses
    it: Optimizer.load_state_dict would replace it), one it does not hold yet is created; a tensor `lr` is filled, HFAdamW's group counter too.
    `fused` (FusedClipAdamW): the moments and the counter go into ITS buffers (load_from) and `optimizer.state` stays as it is -- empty."""
    hf = _is_hf(opt)
    loaded = {}
    for gs, g in zip(sd["param_groups"], opt.param_groups):
        counts = set()
        for p, i in zip(g["params"], gs["params"]):
            src = sd["state"].get(i, {})
            if hf and "step" in src:
                counts.add(int(src["step"]))
            loaded[p] = src
            if fused is not None:
                continue
            own = {k: t for k, t in src.items() if not (hf and k == "step")}
            live = opt.state[p] if p in opt.state else None
            if not live:
                if own:
                    opt.state[p] = {k: _place(k, t, p, g) for k, t in own.items()}
                continue
            for k, t in live.items():
                if not torch.is_tensor(t):
                    live[k] = _place(k, own[k], p, g) if k in own else t
                elif k not in own:
                    t.zero_()
                elif torch.is_tensor(own[k]):
                    t.copy_(own[k])
                else:
                    t.fill_(float(own[k]))
        if torch.is_tensor(g["lr"]):
            g["lr"].fill_(float(gs["lr"]))
        else:
            g["lr"] = float(gs["lr"])
        if hf:
            n = float(counts.pop()) if counts else 0.0
            if torch.is_tensor(g.get("step")):
                g["step"].fill_(n)
            elif n:
                g["step"] = torch.full((), n, dtype=torch.float32, device=g["params"][0].device)
    if fused is not None:                                    # host tensors straight into the buffers the captured update addresses: no second device copy
        fused.load_from(types.SimpleNamespace(param_groups=[dict(g) for g in sd["param_groups"]], state=loaded))


# ------------------------------------------------------------------------------------------------ models
def _master_prefix(module, masters):
    for name, m in module.named_modules():
        if m is masters.module:
            return name + "." if name else ""
    return None


def model_state(module, masters=None):
    """module.state_dict() on the host (buffers included), the fp32 masters in place of the values they are rounded to"""
    prefix = _master_prefix(module, masters) if masters is not None else None
    fp32 = {prefix + k: t for k, t in masters.fp32_items()} if prefix is not None else {}
    return {k: to_host(fp32.get(k, v)) for k, v in module.state_dict().items()}         # a rounded value with a master is never copied out


def plan_model_load(name, module, saved, masters=None, who="load_state_dict"):
    """A saved model state against the live module, nothing changed: RuntimeError for a missing / unexpected / mis-shaped key, as
    load_state_dict(strict=True); returns the copies [(live tensor, saved tensor)] that load it in place -- a parameter with a master gets the
    value in its master (the caller rounds it back: sync_low), a frozen one in the module and in the fp32 copy MasterWeights keeps"""
    if not isinstance(saved, dict):
        raise RuntimeError(f"{who}: no state of model `{name}`")
    own = module.state_dict()
    missing = [k for k in own if k not in saved]
    unexpected = [k for k in saved if k not in own]
    bad = [(k, tuple(saved[k].shape) if torch.is_tensor(saved[k]) else type(saved[k]).__name__, tuple(own[k].shape)) for k in own
           if k in saved and (not torch.is_tensor(saved[k]) or tuple(saved[k].shape) != tuple(own[k].shape))]
    if missing or unexpected or bad:
        raise RuntimeError(f"{who}: the state of `{name}` does not fit {type(module).__name__}: missing {missing[:5]} unexpected {unexpected[:5]} "
                           f"mis-shaped {bad[:5]}")
    copies = [(own[k], saved[k]) for k in own]
    prefix = _master_prefix(module, masters) if masters is not None else None
    if prefix is not None:
        by_id = {id(m) for _, m in masters.pairs()}
        for k, t in masters.fp32_items():
            if prefix + k in saved:
                if id(t) in by_id:
                    copies = [c for c in copies if c[0] is not own[prefix + k]]
                copies.append((t, saved[prefix + k]))
    return copies


# ------------------------------------------------------------------------------------------------ the eager half
class EagerTail:
    """What an eager step keeps behind its backward, in the terms of train_step.FlatGradientTail's state methods: the optimizer holds its own
    state, an open accumulation window is in p.grad.
    Limitation: the window's layout (one fp32 tensor per parameter) cannot tell "no gradient" from "a gradient of zeros", and the optimizer treats
    them differently (it skips a parameter without a gradient: no moment decay, no weight decay).  `load` reads an all-zero entry as NO gradient,
    which is what an eager step has for a parameter outside the graph; a parameter that is in the graph and held a gradient of exact zeros at
    save time resumes without one -- the same unless the window's remaining backwards leave it without a gradient too."""
    fused = masters = None

    def __init__(self, opt, exchange=None):
        self.opt, self.exchange = opt, exchange

    def require_single_rank(self, what):
        if self.exchange is not None and getattr(self.exchange, "active", True):
            raise NotImplementedError(f"{what}: one rank only (not with an active gradient exchange: per-rank generator state is not saved)")

    def optimizer_state(self):
        return stock_optimizer_state(self.opt)

    def window(self):
        return [torch.zeros(p.shape, dtype=torch.float32) if p.grad is None else p.grad.detach().to("cpu", torch.float32, copy=True)
                for p in optimizer_params(self.opt)]

    def check_window(self, who):
        pass

    @torch.no_grad()
    def load(self, optimizer, window):
        load_optimizer_state(optimizer, self.opt)
        for i, p in enumerate(optimizer_params(self.opt)):
            src = None if window is None else window[i]
            if src is None or not bool(src.any()):          # nothing accumulated: what the eager step has for it is NO gradient (the optimizer then skips the parameter)
                if p.grad is not None and self.exchange is not None:
                    p.grad.zero_()                           # views of an averager's buckets must survive
                else:
                    p.grad = None
            elif p.grad is not None:
                p.grad.copy_(src)
            else:
                p.grad = src.to(p.device, p.dtype)


# ------------------------------------------------------------------------------------------------ the step
def _tail_of(step):
    tail = getattr(step, "tail", None)
    return tail if tail is not None else EagerTail(step.opt, getattr(step, "exchange", None))


def _models_of(step):
    return {name: getattr(step, name) for name in step.STATE_MODELS}


def _device_of(step):
    return next(next(iter(_models_of(step).values())).parameters()).device


def export_step(step):
    tail = _tail_of(step)
    tail.require_single_rank(f"{type(step).__name__}.state_dict")
    if getattr(step, "prefetched", None) is not None:
        raise ValueError(f"{type(step).__name__}.state_dict: a Swin forward is prefetched (pipeline_swin) and has already drawn its noise; save after "
                         "a call made with next_batch=None")
    dev = _device_of(step)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    acc = int(getattr(step.args, step.STATE_WINDOW))
    state = {"format": FORMAT, "kind": step.STATE_KIND,
             "models": {name: model_state(m, tail.masters) for name, m in _models_of(step).items()},
             "optimizer": tail.optimizer_state(),
             "scheduler": None if step.sched is None else to_host(step.sched.state_dict()),
             "i_batch": int(step.i_batch)}
    if step.i_batch % acc != 0:
        state["window"] = tail.window()
    state["rng"] = torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None
    return state


_KEYS = {"format", "kind", "models", "optimizer", "scheduler", "i_batch", "rng"}


def load_step(step, state):
    who = f"{type(step).__name__}.load_state_dict"
    tail = _tail_of(step)
    tail.require_single_rank(who)
    # -- everything is checked before anything changes
    if not isinstance(state, dict) or state.get("format") != FORMAT:
        raise ValueError(f"{who}: a step state of format {FORMAT}, got format {state.get('format') if isinstance(state, dict) else type(state).__name__!r}")
    if state.get("kind") != step.STATE_KIND:
        raise ValueError(f"{who}: a state of kind {state.get('kind')!r} cannot be loaded into a {step.STATE_KIND!r} step")
    if set(state) - {"window"} != _KEYS:
        raise RuntimeError(f"{who}: missing {sorted(_KEYS - set(state))} unexpected {sorted(set(state) - _KEYS - {'window'})}")
    models = _models_of(step)
    if not isinstance(state["models"], dict) or set(state["models"]) != set(models):
        raise RuntimeError(f"{who}: the state holds the models {sorted(state['models'])}, the step {sorted(models)}")
    copies = []
    for name, m in models.items():
        copies += plan_model_load(name, m, state["models"][name], tail.masters, who)
    check_optimizer_state(state["optimizer"], step.opt, who, tail.fused)
    params = optimizer_params(step.opt)
    acc = int(getattr(step.args, step.STATE_WINDOW))
    i_batch = state["i_batch"]
    if isinstance(i_batch, bool) or not isinstance(i_batch, int) or i_batch < 0:
        raise RuntimeError(f"{who}: i_batch {i_batch!r}")
    window = state.get("window")
    if (i_batch % acc != 0) != (window is not None):
        raise RuntimeError(f"{who}: i_batch {i_batch} with accumulation over {acc} micro-steps " + ("needs" if window is None else "has no open") + " `window`")
    if window is not None:
        if len(window) != len(params):
            raise RuntimeError(f"{who}: `window` holds {len(window)} gradients, the optimizer steps {len(params)} parameters")
        for i, (t, p) in enumerate(zip(window, params)):
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(p.shape):
                raise RuntimeError(f"{who}: `window` entry {i} does not have its parameter's shape {tuple(p.shape)}")
    tail.check_window(who)
    if (state["scheduler"] is None) != (step.sched is None):
        raise RuntimeError(f"{who}: the state " + ("has no" if state["scheduler"] is None else "has a") + " scheduler, the step " +
                           ("has one" if step.sched is not None else "has none"))
    dev = _device_of(step)
    rng = state["rng"]
    if dev.type == "cuda":
        if not torch.is_tensor(rng) or rng.dtype != torch.uint8 or rng.shape != torch.cuda.get_rng_state(dev).shape:
            raise RuntimeError(f"{who}: `rng` is not a generator state of {dev}")
        torch.cuda.synchronize(dev)
    # -- values into the tensors that exist; nothing is rebound
    with torch.no_grad():
        for dst, src in copies:
            dst.copy_(src)
        if tail.masters is not None:
            tail.masters.sync_low()
    tail.load(state["optimizer"], window)
    moved = {id(p): p for m in models.values() for p in m.parameters()}
    moved.update({id(p): p for p in params})
    _bump_versions(list(moved.values()))                    # cached bf16 shadows are rebuilt
    step.i_batch = i_batch
    if hasattr(step, "prefetched"):
        step.prefetched = None
    if dev.type == "cuda":
        torch.cuda.set_rng_state(rng, dev)
    if step.sched is not None:
        step.sched.load_state_dict(_like(step.sched.__dict__, state["scheduler"]))


class StepState:
    """state_dict() / load_state_dict(state) of a training step (module docstring): mixed into the six step classes, which name their `STATE_KIND`,
    the attributes that hold their models (`STATE_MODELS`) and the field of `args` with their accumulation steps (`STATE_WINDOW`)."""
    STATE_KIND = STATE_WINDOW = None
    STATE_MODELS = ()

    def state_dict(self):
        """Everything a stopped run needs to continue with the bits of the uninterrupted one, as CPU tensors and builtins; may synchronise with the
        host, and may be called between any two calls of the step.  NotImplementedError with an active gradient exchange; ValueError while a
        prefetched Swin forward is pending (pipeline_swin: save after a call made with next_batch=None)."""
        return export_step(self)

    def load_state_dict(self, state):
        """A state of a step of the same kind -- eager or graphed -- into this constructed step: checked first (ValueError: another kind or format,
        hyper-parameters that differ from what the step was built with; RuntimeError: keys, shapes or counts that do not fit -- the step and its
        models are then untouched), then copied IN PLACE into parameters, buffers, masters, moments, flat gradient buffers and the
        learning-rate word; the generator is set and the scheduler loaded.  Which batch comes next is the caller's."""
        load_step(self, state)
