"""The `criterion` argument of the training steps (train_step.Criterion: class weights and label smoothing), on the small synthetic configurations of
tests/test_gpu_step_oracle.py and tests/test_gpu_unimodal_step.py.

  (a) criterion=None is the parent's behaviour: a graphed target, auxiliary and V-only step built without the argument and one built with criterion=None
      walk the same BITS of loss and parameters over three updates;
  (b) a weighted, smoothed criterion (eps = 0.1) against the fp64 step -- tests/support_step_oracle.py and tests/support_unimodal_oracle.py with their loss
      replaced by Criterion.reference (tests/support_criterion.loss_replaced) -- on GraphedTargetStep, GraphedAuxStep and GraphedUnimodalStep: losses,
      total norms and the parameters after three clipped SGD steps through those files' own compare_trajectory, i.e. at exactly their bars;
  (c) the eager step with the same criterion, start and noise: its losses against the graphed step's at 2e-4 of max(1, |loss|), the bar
      tests/test_gpu_train_step.py holds eager against graphed to;
  (d) pad_rows=True with a criterion: a short batch's loss is Criterion.reference over its real rows in the fp64 model, at (b)'s loss bar;
  (e) skip_nonfinite + grad_report + an accumulation window of two + a criterion: one window runs, the loss is finite, one update applied."""
import pytest
import torch

from tests import support_criterion as SC
from tests import support_step_oracle as SO
from tests import support_unimodal_oracle as UO
from tests import test_gpu_guard_steps as GS
from tests import test_gpu_step_oracle as TS
from tests import test_gpu_unimodal_step as TU
from tests.test_gpu_step_oracle import noise, norms  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EPS, LR = 0.1, TS.LR
EAGER_GRAPHED = 2e-4                                          # of max(1, |loss|): tests/test_gpu_train_step.py::test_whole_step_graphs_equal_eager_step


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def criteria(dev, kind="random"):
    """the same criterion twice: for the fp64 reference on the CPU and for the step on the device"""
    from facialmmt_amd.train_step import Criterion
    w = SC.weights_for(kind, 7)
    return Criterion(w, EPS, device="cpu"), Criterion(w, EPS, device=dev)


def _params(module):
    return {k: p.detach().clone() for k, p in module.named_parameters()}


# ------------------------------------------------------------------------------------------------ (a)
def _walk_target(dev, noise, **kw):
    from facialmmt_amd.train_step import GraphedTargetStep
    cfg, swin, mm, batch = TS.build(dev, accumulation=1, drop_path=False)
    torch.manual_seed(77)
    noise.fill(TS.gumbel(31))
    step = GraphedTargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=LR), None, cfg, batch, autocast_dtype=None, **kw)
    losses = []
    for i in range(3):
        noise.fill(TS.gumbel(31 + i))
        losses.append(step(batch)[0].clone())
    torch.cuda.synchronize()
    return torch.stack(losses), _params(mm)


def _walk_aux(dev, **kw):
    from facialmmt_amd.train_step import GraphedAuxStep
    cfg, swin = TS.build_aux(dev, drop_path=False, accumulation=1)
    imgs, labels = TS.aux_batch(dev)
    torch.manual_seed(77)
    step = GraphedAuxStep(swin, torch.optim.SGD(swin.parameters(), lr=LR), None, cfg, imgs, labels, **kw)
    losses = torch.stack([step(imgs, labels).clone() for _ in range(3)])
    torch.cuda.synchronize()
    return losses, _params(swin)


def _walk_unimodal(dev, **kw):
    from facialmmt_amd.train_step import GraphedUnimodalStep
    cfg, model = TU.build(dev, accumulation=1)
    batches = [TU.micro_batch(dev, 10 + i) for i in range(3)]
    torch.manual_seed(77)
    step = GraphedUnimodalStep(model, torch.optim.SGD(model.parameters(), lr=LR), None, cfg, batches[0], **kw)
    losses = torch.stack([step(b).clone() for b in batches])
    torch.cuda.synchronize()
    return losses, _params(model)


@pytest.mark.parametrize("which", ["target", "aux", "unimodal"])
def test_criterion_none_walks_the_parents_bits(dev, noise, which):
    walk = {"target": lambda **kw: _walk_target(dev, noise, **kw), "aux": lambda **kw: _walk_aux(dev, **kw), "unimodal": lambda **kw: _walk_unimodal(dev, **kw)}[which]
    l0, p0 = walk()
    l1, p1 = walk(criterion=None)
    print(f"{which}: losses {l0.tolist()}")
    assert torch.isfinite(l0).all() and torch.equal(l0, l1)
    assert sorted(p0) == sorted(p1) and all(torch.equal(p0[k], p1[k]) for k in p0)


# ------------------------------------------------------------------------------------------------ (b), (c)
def _eager_against_graphed(label, eager, graphed):
    print(f"{label} eager losses {eager} graphed {graphed}")
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= EAGER_GRAPHED * max(1.0, abs(a)), (label, eager, graphed)


def test_target_step_with_a_criterion_against_the_fp64_step(dev, noise, norms):
    from facialmmt_amd.train_step import GraphedTargetStep, TargetStep
    cpu_crit, dev_crit = criteria(dev)
    cfg, swin, mm, batch = TS.build(dev, accumulation=1, drop_path=False)
    with SC.loss_replaced(cpu_crit):
        ref, msd, gs = TS.reference_trajectory(swin, mm, cfg, batch, [None] * 3, 3, 10000)
    swin_start = _params(swin)
    noise.fill(gs[0])
    step = GraphedTargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=LR), None, cfg, batch, autocast_dtype=None, criterion=dev_crit)
    assert step.fused is None and norms and step.criterion is dev_crit
    captured = norms[-1]
    losses, masks, got = [], [], []
    for i in range(3):
        noise.fill(gs[i])
        loss, mask = step(batch)
        losses.append(float(loss))
        masks.append(mask.clone())
        got.append(float(captured))
    torch.cuda.synchronize()
    TS.compare_trajectory("criterion, graphed target", ref, msd, losses, masks, got, mm, swin, swin_start, cfg.clip)
    cfg2, swin2, mm2, batch2 = TS.build(dev, accumulation=1, drop_path=False)
    cfg2.clip = cfg.clip
    eager = TargetStep(swin2, mm2, torch.optim.SGD(mm2.parameters(), lr=LR), None, cfg2, autocast_dtype=None, criterion=dev_crit)
    eager_losses = []
    for i in range(3):
        noise.fill(gs[i])
        eager_losses.append(float(eager(batch2)[0]))
    _eager_against_graphed("target", eager_losses, losses)


def test_auxiliary_step_with_a_criterion_against_the_fp64_step(dev, norms):
    from facialmmt_amd.train_step import AuxStep, GraphedAuxStep
    cpu_crit, dev_crit = criteria(dev, "zero_class")
    cfg, swin = TS.build_aux(dev, drop_path=False, accumulation=1)
    imgs, labels = TS.aux_batch(dev)
    ref_batch = [(imgs.double().cpu(), labels.cpu())] * 3
    with SC.loss_replaced(cpu_crit):
        cfg.clip = 1e9
        free = SO.run_aux(SO.leaves(swin, torch.float64), cfg, ref_batch, [None] * 3, lr=LR)
        ns = [s["norm"] for s in free["steps"]]
        # between the first norm (the same in both runs: nothing was clipped before it) and the largest later one, so that the clip binds in one step and not
        # in another, as TS.reference_trajectory arranges it; asserted below on the run the step is compared with
        cfg.clip = float((ns[0] * max(ns[1:])) ** 0.5)
        ssd = SO.leaves(swin, torch.float64)
        ref = SO.run_aux(ssd, cfg, ref_batch, [None] * 3, lr=LR)
    ns = [s["norm"] for s in ref["steps"]]
    assert max(ns) > cfg.clip > min(ns), (ns, cfg.clip)
    step = GraphedAuxStep(swin, torch.optim.SGD(swin.parameters(), lr=LR), None, cfg, imgs, labels, criterion=dev_crit)
    captured = norms[-1]
    losses, got = [], []
    for _ in range(3):
        losses.append(float(step(imgs, labels)))
        got.append(float(captured))
    torch.cuda.synchronize()
    # TS.compare_trajectory is the target step's: a kept-frame mask per micro-step (none here: a constant on both sides) and a Swin nobody may move (here: no module)
    one = torch.ones(1, 1)
    for m in ref["micro"]:
        m["mask"] = one
    TS.compare_trajectory("criterion, graphed auxiliary", ref, ssd, losses, [one] * 3, got, swin, torch.nn.Module(), {}, cfg.clip)
    cfg2, swin2 = TS.build_aux(dev, drop_path=False, accumulation=1)
    cfg2.clip = cfg.clip
    eager = AuxStep(swin2, torch.optim.SGD(swin2.parameters(), lr=LR), None, cfg2, criterion=dev_crit)
    _eager_against_graphed("auxiliary", [float(eager(imgs, labels)) for _ in range(3)], losses)


def test_unimodal_step_with_a_criterion_against_the_fp64_step(dev, norms):
    from facialmmt_amd.train_step import GraphedUnimodalStep, UnimodalStep
    cpu_crit, dev_crit = criteria(dev)
    cfg, model = TU.build(dev, accumulation=1)
    batches = [TU.micro_batch(dev, 10 + i) for i in range(3)]
    with SC.loss_replaced(cpu_crit):
        ref, sd = TU.reference_trajectory(model, cfg, batches)
    step = GraphedUnimodalStep(model, torch.optim.SGD(model.parameters(), lr=LR), None, cfg, batches[0], criterion=dev_crit)
    assert step.fused is None and norms
    captured = norms[-1]
    losses, got = [], []
    for b in batches:
        losses.append(float(step(b)))
        got.append(float(captured))
    torch.cuda.synchronize()
    TU.compare_trajectory("criterion, graphed unimodal", ref, sd, losses, got, model, cfg.clip)
    cfg2, model2 = TU.build(dev, accumulation=1)
    cfg2.clip = cfg.clip
    eager = UnimodalStep(model2, torch.optim.SGD(model2.parameters(), lr=LR), None, cfg2, criterion=dev_crit)
    _eager_against_graphed("unimodal", [float(eager(b)) for b in batches], losses)


# ------------------------------------------------------------------------------------------------ (d)
def _loss_bar(label, got, want):
    """the loss bar of TS.compare_trajectory / TU.compare_trajectory, through TU.compare_trajectory itself: one micro-step, no update looked at"""
    print(f"{label}: loss {got:.9f} reference {want:.9f}")
    ref = {"micro": [{"loss": want}], "steps": [{"norm": 1.0}] * 3}
    TU.compare_trajectory(label, ref, {}, [got], [1.0] * 3, torch.nn.Module(), 0.0)


def test_pad_rows_with_a_criterion_unimodal(dev):
    from facialmmt_amd.train_step import GraphedUnimodalStep
    cpu_crit, dev_crit = criteria(dev)
    cfg, model = TU.build(dev, accumulation=1)
    sd = UO.leaves(model, torch.float64)
    step = GraphedUnimodalStep(model, torch.optim.SGD(model.parameters(), lr=LR), None, cfg, TU.micro_batch(dev, 10), pad_rows=True, criterion=dev_crit)
    short = TU.micro_batch(dev, 11, n=TU.B - 1)
    got = float(step(short))
    assert step.rows == TU.B - 1 and step.padded_calls == 1
    with SC.loss_replaced(cpu_crit), torch.no_grad():
        want = float(UO.step_loss(sd, cfg, *TU.to_ref(short)))
    _loss_bar("pad_rows unimodal", got, want)


def test_pad_rows_with_a_criterion_auxiliary(dev):
    from facialmmt_amd.train_step import GraphedAuxStep
    cpu_crit, dev_crit = criteria(dev)
    cfg, swin = TS.build_aux(dev, drop_path=False, accumulation=1)
    ssd = SO.leaves(swin, torch.float64)
    imgs, labels = TS.aux_batch(dev)
    step = GraphedAuxStep(swin, torch.optim.SGD(swin.parameters(), lr=LR), None, cfg, imgs, labels, pad_rows=True, criterion=dev_crit)
    b = imgs.shape[0] - 5
    got = float(step(imgs[:b], labels[:b]))
    assert step.rows == b and step.padded_calls == 1
    with SC.loss_replaced(cpu_crit), torch.no_grad():
        want = float(SO.aux_step_loss(ssd, imgs[:b].double().cpu(), labels[:b].cpu()))
    _loss_bar("pad_rows auxiliary", got, want)


# ------------------------------------------------------------------------------------------------ (e)
def test_guard_report_accumulation_and_a_criterion_together(dev):
    _, dev_crit = criteria(dev)
    step, model = GS._unimodal(dev, accumulation=2, skip_nonfinite=True, grad_report=True, criterion=dev_crit)
    losses = [float(step(TU.micro_batch(dev, 80 + i))) for i in range(2)]
    mon, rep = step.monitor.read(), step.grad_report.read()
    print(f"losses {losses}; applied {mon.applied} skipped {mon.skipped} last norm {mon.last_norm}; report total norm {rep.total_norm}")
    assert all(l == l and abs(l) < 1e4 for l in losses)
    assert mon.applied == 1 and mon.skipped == 0 and mon.micro_steps == 2 and rep.bad_updates == 0 and rep.total_norm > 0
    with pytest.raises(ValueError, match="global_rows"):      # class weights and global_rows: refused before anything is copied or launched
        step(TU.micro_batch(dev, 82), global_rows=4)
