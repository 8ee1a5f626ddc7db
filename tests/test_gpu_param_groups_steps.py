"""GPU tests of a graphed training step whose optimizer has two parameter groups: the fused update stays on (one launch, fmmt_adamw_groups), and with
it what depends on it -- skip_nonfinite, the replica digest, the moments in state_dict().

The model is the V-only one of tests/test_gpu_unimodal_step.py (B = 4, L = 160, two layers, fp32, dropout 0).  Its torch.optim.AdamW is split by
name (train_step.named_step_parameters) into a decay group and a no-decay group -- biases and LayerNorm weights --, each with its own device
learning rate, under a LambdaLR with one lambda per group.

The base learning rates are 1e-4 / 5e-5, tests/test_gpu_unimodal_step.py's for this model: the comparison with the stock path over three steps is one
of trajectories, and a run whose loss diverges amplifies last-bit differences whichever kernel wrote them."""
import copy

import pytest
import torch

from tests import test_gpu_unimodal_step as US

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-6, 2e-7                                          # test_fused_clip_adamw_matches_torch's
BASE_LR = (1e-4, 5e-5)
LAMBDAS = (lambda k: (k + 1) / 3.0 if k < 2 else max(0.0, (10 - k) / 8.0), lambda k: 1.0 / (1 + k))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _no_decay(name):
    # this model's LayerNorms are named `...dense_norm.LayerNorm.weight`, `...norm...`: matched without case, wider than a bare "LayerNorm"
    return name.endswith("bias") or "norm" in name.lower()


def _optimizer(model, dev, weight_decay=(0.01, 0.0)):
    from facialmmt_amd.train_step import named_step_parameters
    named = list(named_step_parameters(model))
    assert len(named) == len(list(model.parameters()))
    split = [[p for n, p in named if not _no_decay(n)], [p for n, p in named if _no_decay(n)]]
    assert len(split[0]) > 2 and len(split[1]) > 2
    order = [int(_no_decay(n)) for n, _ in named]
    assert order != sorted(order)                                # the groups interleave in the model's (= the descriptor table's) order
    lrs = [torch.tensor(lr, device=dev) for lr in BASE_LR]
    opt = torch.optim.AdamW([dict(params=ps, lr=lr, weight_decay=wd) for ps, lr, wd in zip(split, lrs, weight_decay)], eps=1e-6, capturable=True)
    return opt, lrs, torch.optim.lr_scheduler.LambdaLR(opt, list(LAMBDAS)), order


class Run:
    def __init__(self, dev, graphed=True, seed=201, weight_decay=(0.01, 0.0), **kw):
        from facialmmt_amd.train_step import GraphedUnimodalStep, UnimodalStep
        self.cfg, self.model = US.build(dev, seed=seed)
        self.opt, self.lrs, self.sched, self.order = _optimizer(self.model, dev, weight_decay)
        if graphed:
            self.step = GraphedUnimodalStep(self.model, self.opt, self.sched, self.cfg, US.micro_batch(dev, 80), **kw)
        else:
            self.step = UnimodalStep(self.model, self.opt, self.sched, self.cfg)

    def state(self):
        """everything an update writes: parameters, the fused moments and count (or the optimizer's own), both learning rates"""
        torch.cuda.synchronize()
        out = [p.detach().clone() for p in self.model.parameters()] + [lr.clone() for lr in self.lrs]
        fused = getattr(self.step, "fused", None)
        if fused is not None:
            return out + [t.clone() for t in fused.m + fused.v] + [fused.step.clone()]
        return out + [self.opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq") for p in self.model.parameters()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _batches(dev, n):
    return [US.micro_batch(dev, 80 + i) for i in range(n)]


def test_two_groups_keep_the_fused_update_and_match_the_stock_path(dev, monkeypatch):
    from facialmmt_amd import train_step
    batches = _batches(dev, 3)
    a = Run(dev)
    assert a.step.tail.fused is not None and a.step.fused is a.step.tail.fused and a.step.handover is not None
    assert a.step.fused.group_table is not None and a.step.fused.group_of.tolist() == a.order
    assert float(a.lrs[0]) == pytest.approx(BASE_LR[0] / 3) and float(a.lrs[1]) == pytest.approx(BASE_LR[1])
    start = a.state()
    losses_a = [float(a.step(b)) for b in batches]
    torch.cuda.synchronize()
    assert not a.opt.state and float(a.step.fused.step) == 3.0  # the moments stay in the fused update
    assert a.opt.param_groups[0]["lr"] is a.lrs[0] and a.opt.param_groups[1]["lr"] is a.lrs[1]
    assert float(a.lrs[0]) == pytest.approx(BASE_LR[0] * LAMBDAS[0](3)) and float(a.lrs[1]) == pytest.approx(BASE_LR[1] * LAMBDAS[1](3))
    d = a.step.replica_digest()
    assert d.shape == (6,) and d.dtype == torch.int64 and d.is_cuda
    assert not any(torch.equal(x, y) for x, y in zip(a.state()[:len(a.order)], start[:len(a.order)]))
    monkeypatch.setattr(train_step, "FUSED_ADAMW", False)       # what the step did for this optimizer before: clip_grad_norm_ + optimizer.step()
    b = Run(dev)
    assert b.step.tail.fused is None
    losses_b = [float(b.step(x)) for x in batches]
    torch.cuda.synchronize()
    assert b.opt.state and all(float(b.opt.state[p]["step"]) == 3.0 for p in b.model.parameters())
    print("losses fused", losses_a, "stock", losses_b)
    worst = 0.0
    for (n, pa), pb in zip(a.model.named_parameters(), b.model.parameters()):
        worst = max(worst, float((pa.detach() - pb.detach()).abs().max()))
        assert torch.allclose(pa, pb, rtol=RTOL, atol=ATOL), (n, float((pa.detach() - pb.detach()).abs().max()))
    print("max |fused - stock| over all parameters after three steps", worst)
    with pytest.raises(ValueError, match="replica_digest"):
        b.step.replica_digest()


def test_skip_nonfinite_is_accepted_with_two_groups(dev):
    clean, clean2 = _batches(dev, 2)
    x, mask, labels = clean
    assert float(mask[0, 5]) == 1.0
    bad = x.clone()
    bad[0, 5, 11] = float("nan")                                # one NaN at a token the mask keeps
    g = Run(dev, skip_nonfinite=True)
    assert g.step.fused is not None and g.step.fused.monitor is g.step.monitor and g.step.fused.group_table is not None
    plain = Run(dev)
    assert _same(g.state(), plain.state())
    g.step(clean)
    plain.step(clean)
    after1 = g.state()
    assert _same(after1, plain.state())                          # clean batch: every bit of the step without the option
    loss = float(g.step((bad, mask, labels)))
    after2 = g.state()
    r = g.step.monitor.read()
    n = len(g.order)
    assert loss != loss and (r.skipped, r.applied, r.nonfinite_losses) == (1, 1, 1)
    assert _same(after1[:n], after2[:n]) and _same(after1[n + 2:], after2[n + 2:])      # parameters, moments, count; the schedule advanced
    assert float(g.step.fused.step) == 1.0 and g.sched.last_epoch == 2
    g.step(clean2)
    r = g.step.monitor.read()
    assert (r.skipped, r.applied) == (1, 2) and all(bool(torch.isfinite(t).all()) for t in g.state())
    # the step without the option on the same clean batches, its schedule advanced by hand over the skipped update: every bit again
    plain.sched.step()
    plain.step(clean2)
    assert _same(g.state(), plain.state())


def test_save_and_resume_with_two_groups(dev):
    batches = _batches(dev, 4)
    a = Run(dev)
    for b in batches:
        a.step(b)
    end_a = a.state()
    b = Run(dev)
    for x in batches[:2]:
        b.step(x)
    state = copy.deepcopy(b.step.state_dict())
    groups = state["optimizer"]["param_groups"]
    assert len(groups) == 2 and [type(g["lr"]) for g in groups] == [float, float] and groups[0]["lr"] != groups[1]["lr"]
    assert [g["weight_decay"] for g in groups] == [0.01, 0.0]
    assert len(state["optimizer"]["state"]) == len(b.order) and all(float(s["step"]) == 2.0 for s in state["optimizer"]["state"].values())
    c = Run(dev, seed=555)                                        # other weights, a new capture
    assert not _same(c.state(), b.state())
    held = [t.data_ptr() for t in c.lrs + c.step.fused.m + c.step.fused.v]
    # a state whose second group's weight decay differs: ValueError, nothing changed
    other = copy.deepcopy(state)
    other["optimizer"]["param_groups"][1]["weight_decay"] = 0.01
    before = c.state()
    with pytest.raises(ValueError, match="group 1.*`weight_decay`"):
        c.step.load_state_dict(other)
    assert _same(c.state(), before) and c.step.i_batch == 0 and c.sched.last_epoch == 0
    c.step.load_state_dict(state)
    assert _same(c.state(), b.state()) and not c.opt.state
    assert held == [t.data_ptr() for t in c.lrs + c.step.fused.m + c.step.fused.v]
    assert c.opt.param_groups[0]["lr"] is c.lrs[0] and c.opt.param_groups[1]["lr"] is c.lrs[1]
    assert float(c.lrs[0]) == groups[0]["lr"] and float(c.lrs[1]) == groups[1]["lr"]          # both learning rates restored
    for x in batches[2:]:
        c.step(x)
    assert _same(c.state(), end_a)                                # the bits of the uninterrupted run
    # a grouped graphed state into a grouped EAGER step of the same optimizer, and back
    e = Run(dev, graphed=False, seed=777)
    e.step.load_state_dict(state)
    n = len(e.order)
    assert _same(e.state()[:n + 2], b.state()[:n + 2])
    assert _same(e.state()[n + 2:], b.state()[n + 2:-1]) and all(float(e.opt.state[p]["step"]) == 2.0 for p in e.model.parameters())
    back = Run(dev, seed=556)
    back.step.load_state_dict(copy.deepcopy(e.step.state_dict()))
    assert _same(back.state(), b.state())
