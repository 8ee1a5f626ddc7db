"""GPU tests of the target-task steps with color_jitter= (the MELD train transform drawn on the device, inside the captured graphs): on the small
batch of tests/test_gpu_ragged_step.py -- B = 2 utterances, Lv = 6 frame slots, capacity 12, its noise-free configuration (fp32, tau = 1e5, threshold
0.1, DropPath and dropout off, stand-in text encoder, SGD) and its tolerances (losses 2e-4, parameters and BatchNorm statistics 1e-4 of scale, kept
masks equal and non-empty) -- with the frames as uint8 112 x 112 crops, the 'cv2' resize of the MELD path."""
import types

import numpy as np
import pytest
import torch

from facialmmt_amd import ops
from facialmmt_amd.augment import ColorJitter
from oracle import preproc as P
from tests import support_color_jitter as J
from tests import test_gpu_ragged_step as RS

pytestmark = pytest.mark.gpu

B, LV, CAP = RS.B, RS.LV, RS.CAP
SEQ = ([5, 2], [6, 6], [1, 3], [5, 2])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _models(dev, accumulation=1):
    cfg, swin, mm = RS._models(dev, accumulation)
    swin.swin.input_resize = "cv2"
    return cfg, swin, mm


def _batch(dev, cfg, num_imgs, rank=0):
    """the loader's batch: frames (B, Lv, 112, 112, 3) uint8 with every slot random, num_imgs as the reference's collate yields it"""
    import bench
    args = types.SimpleNamespace(utts=B, frames=LV, dtype="fp32", plm="roberta-large", input="u8", resize="cv2")
    batch = list(bench.synth_batch(args, dev, rank, cfg))
    batch[0] = batch[0] % 1000
    batch[8] = batch[8].view(B, LV, *batch[8].shape[1:])
    vmask = torch.zeros(B, LV, device=dev)
    for u, k in enumerate(num_imgs):
        vmask[u, :k] = 1
    batch[6], batch[9] = vmask, list(num_imgs)
    return tuple(batch)


def _walk(step, batches, seeds):
    out = types.SimpleNamespace(losses=[], kept=[], tables=[], counts=[], means=[])
    bn = step.swin.swin.output_layer[3]
    for batch, seed in zip(batches, seeds):
        if seed is not None:
            torch.manual_seed(seed)
        loss, k = step(batch)
        out.losses.append(loss.clone())
        out.kept.append(k.clone())
        out.tables.append(step.last_jitter.clone())
        out.counts.append(step.frame_counts.tolist())
        out.means.append(bn.running_mean.clone())
    torch.cuda.synchronize()
    return out


def _end(swin, mm):
    bn = swin.swin.output_layer[3]
    return {k: v.detach().clone() for k, v in mm.named_parameters()}, bn.running_mean.clone(), bn.running_var.clone()


def _check_tables(tables, rows):
    for t in tables:
        assert t.shape == (rows, 8) and t.dtype == torch.int32
        fac = t[:, :3].contiguous().view(torch.float32)
        assert (fac >= 0.5).all() and (fac <= 1.5).all() and (t[:, 3] >= 0).all() and (t[:, 3] <= 255).all()
        assert (t[:, 4:].sort(1).values == torch.arange(4, dtype=torch.int32, device=t.device)).all()


@pytest.fixture(scope="module")
def eager(dev):
    """TargetStep(frame_capacity, color_jitter) over SEQ, reseeded in front of every call; the patch embedding's inputs and output of the last call"""
    from facialmmt_amd.train_step import TargetStep
    cfg, swin, mm = _models(dev)
    step = TargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=0.05), None, cfg, autocast_dtype=None, frame_capacity=CAP, color_jitter=ColorJitter())
    assert step.last_jitter is None
    pe, seen = swin.swin.patch_embed, []
    real = pe.forward_u8

    def recorder(x, resize="pil", dtype=None, jitter=None):
        y = real(x, resize, dtype, jitter=jitter)
        seen.append((x.clone(), resize, dtype, None if jitter is None else jitter.clone(), y.detach().clone()))
        return y
    pe.forward_u8 = recorder
    run = _walk(step, [_batch(dev, cfg, n) for n in SEQ], [1000 + i for i in range(len(SEQ))])
    run.end, run.seen, run.pe = _end(swin, mm), seen, pe
    pe.forward_u8 = real
    return run


def test_graphed_replays_equal_the_eager_step_from_the_same_generator_state(dev, eager):
    from facialmmt_amd.train_step import GraphedTargetStep
    cfg, swin, mm = _models(dev)
    batches = [_batch(dev, cfg, n) for n in SEQ]
    step = GraphedTargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=0.05), None, cfg, batches[0], autocast_dtype=None, frame_capacity=CAP,
                             color_jitter=ColorJitter())
    g = _walk(step, batches, [1000 + i for i in range(len(SEQ))])
    print("losses eager  ", [float(x) for x in eager.losses])
    print("losses graphed", [float(x) for x in g.losses])
    assert g.counts == eager.counts == [[sum(n)] * 2 for n in SEQ]
    _check_tables(g.tables, CAP)
    for i, (a, b) in enumerate(zip(eager.tables, g.tables)):
        assert torch.equal(a, b), i                                               # the same draws
    assert not torch.equal(g.tables[0], g.tables[1])
    assert float(eager.losses[0]) != float(eager.losses[-1])
    for a, b in zip(eager.losses, g.losses):
        assert abs(float(a) - float(b)) <= 2e-4 * max(1.0, abs(float(a))), (eager.losses, g.losses)
    for a, b in zip(eager.kept, g.kept):
        assert torch.equal(a, b) and float(a.sum()) > 0
    (p0, rm0, rv0), (p1, rm1, rv1) = eager.end, _end(swin, mm)
    assert (rm0 - rm1).abs().max().item() <= 1e-4 * max(1.0, rm0.abs().max().item())
    assert (rv0 - rv1).abs().max().item() <= 1e-4 * max(1.0, rv0.abs().max().item())
    for k in p0:                                                                   # four SGD updates: the gradients of every micro-step
        assert (p0[k] - p1[k]).abs().max().item() <= 1e-4 * max(1.0, p0[k].abs().max().item()), k
    # two consecutive replays of the same batch without a reseed draw different tables
    more = _walk(step, [batches[0], batches[0]], [None, None])
    _check_tables(more.tables, CAP)
    assert not torch.equal(more.tables[0], more.tables[1]) and not torch.equal(more.tables[0], g.tables[-1])


def test_the_jitter_reaches_swin_and_none_leaves_it_out(dev, eager):
    """color_jitter=None: no table, and Swin sees other frames than under the jitter -- its BatchNorm's running mean after one call differs.  (The
    loss does not: in this noise-free configuration Swin only selects frames, and tau = 1e5 keeps them all.)"""
    from facialmmt_amd.train_step import TargetStep
    cfg, swin, mm = _models(dev)
    step = TargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=0.05), None, cfg, autocast_dtype=None, frame_capacity=CAP)
    torch.manual_seed(1000)
    loss, kept = step(_batch(dev, cfg, SEQ[0]))
    assert step.last_jitter is None and step.color_jitter is None and torch.isfinite(loss)
    plain = swin.swin.output_layer[3].running_mean
    assert (plain - eager.means[0]).abs().max().item() > 1e-3 * max(1.0, plain.abs().max().item())


def test_last_jitter_fed_back_reproduces_the_patch_matrix(dev, eager):
    x, resize, dtype, table, y = eager.seen[-1]
    assert len(eager.seen) == len(SEQ) and resize == "cv2" and x.dtype == torch.uint8 and x.shape == (CAP, 112, 112, 3)
    assert torch.equal(table, eager.tables[-1])
    with torch.no_grad():
        assert torch.equal(eager.pe.forward_u8(x, resize, dtype, jitter=eager.tables[-1]), y)
        assert not torch.equal(eager.pe.forward_u8(x, resize, dtype), y)
    n = sum(SEQ[-1])                                                               # the real frames against the oracle; the padded slots are zeros, jittered too
    want = P.patch_cols(np.ascontiguousarray(P.normalize_lut()[J.apply_table(P.resize_u8(x[:n].cpu().numpy(), "cv2"), table[:n].cpu().numpy())].transpose(0, 3, 1, 2)))
    got = ops.patch_embed_u8(x, "cv2", torch.float32, jitter=table)
    assert np.array_equal(got[:n * 3136].cpu().numpy(), want)


def test_short_batch_through_pad_rows(dev):
    """GraphedTargetStep(frame_capacity, pad_rows=True, color_jitter) on a batch cut to one utterance against the eager step on that utterance: the
    padded row keeps nothing and leaves no trace in the update"""
    from facialmmt_amd.train_step import GraphedTargetStep, TargetStep
    runs = {}
    for side in ("eager", "graphed"):
        cfg, swin, mm = _models(dev)
        opt = torch.optim.SGD(mm.parameters(), lr=0.05)
        full = _batch(dev, cfg, [5, 2])
        short = tuple(t[:1] for t in _batch(dev, cfg, [4, 3], rank=1))
        if side == "eager":
            step = TargetStep(swin, mm, opt, None, cfg, autocast_dtype=None, frame_capacity=CAP, color_jitter=ColorJitter())
        else:
            step = GraphedTargetStep(swin, mm, opt, None, cfg, full, autocast_dtype=None, frame_capacity=CAP, pad_rows=True, color_jitter=ColorJitter())
        runs[side] = (_walk(step, [full, short], [41, 42]), _end(swin, mm), getattr(step, "padded_calls", None))
    (e, (pe_, _, _), _), (g, (pg, _, _), padded_calls) = runs["eager"], runs["graphed"]
    print("losses eager", [float(x) for x in e.losses], "graphed", [float(x) for x in g.losses])
    assert padded_calls == 1 and g.counts == e.counts == [[7, 7], [4, 4]]
    for a, b in zip(e.tables, g.tables):
        assert a.shape == (CAP, 8) and torch.equal(a, b)
    for a, b in zip(e.losses, g.losses):
        assert abs(float(a) - float(b)) <= 2e-4 * max(1.0, abs(float(a)))
    assert torch.equal(g.kept[0], e.kept[0]) and torch.equal(g.kept[1][:1], e.kept[1]) and float(e.kept[1].sum()) > 0
    assert float(g.kept[1][1:].abs().sum()) == 0.0
    for k in pe_:
        assert (pe_[k] - pg[k]).abs().max().item() <= 1e-4 * max(1.0, pe_[k].abs().max().item()), k


def test_an_evaluation_between_training_replays_is_not_jittered_and_leaves_them_alone(dev):
    from facialmmt_amd.eval_step import GraphedEvalStep
    from facialmmt_amd.train_step import GraphedTargetStep

    def run(with_eval):
        cfg, swin, mm = _models(dev)
        batch = _batch(dev, cfg, [5, 2])
        step = GraphedTargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=0.05), None, cfg, batch, autocast_dtype=None, frame_capacity=CAP,
                                 color_jitter=ColorJitter())
        losses, tables, logits = [], [], None
        for i in range(3):
            if with_eval and i == 2:
                ev = GraphedEvalStep(swin, mm, cfg, batch, gumbel="off", frame_capacity=CAP)
                held = step.last_jitter.clone()
                logits = [ev(batch)[0].clone() for _ in range(2)]
                assert torch.equal(logits[0], logits[1])                          # no jitter (and no noise): an evaluation is a function of the batch
                assert torch.equal(step.last_jitter, held) and swin.training and mm.training
            torch.manual_seed(1234 + i)
            loss, _ = step(batch)
            losses.append(loss.clone())
            tables.append(step.last_jitter.clone())
        torch.cuda.synchronize()
        return losses, tables, _end(swin, mm)
    (l0, t0, (p0, rm0, rv0)), (l1, t1, (p1, rm1, rv1)) = run(False), run(True)
    assert not torch.equal(l0[0], l0[2])
    for a, b in zip(l0 + t0 + [rm0, rv0], l1 + t1 + [rm1, rv1]):
        assert torch.equal(a, b)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


def test_a_saved_and_reloaded_step_continues_with_the_same_tables(dev):
    """the draws come from the device generator state_dict() already saves: no new state"""
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, step_parameters

    def make(model_seed, generator_seed):
        cfg, swin, mm = _models(dev, 2)
        if model_seed:
            from facialmmt_amd import synth
            synth.fill_state_dict(mm, seed=model_seed)
        torch.manual_seed(generator_seed)
        opt = HFAdamW(step_parameters(mm, None), lr=torch.tensor(1e-3, device=dev), weight_decay=0.01)
        batches = [_batch(dev, cfg, n) for n in SEQ]
        step = GraphedTargetStep(swin, mm, opt, None, cfg, batches[0], autocast_dtype=None, frame_capacity=CAP, pad_rows=True, color_jitter=ColorJitter())
        return step, batches
    a, batches = make(0, 7)
    first = _walk(a, batches[:1], [None])
    state = a.state_dict()
    assert set(state) <= {"format", "kind", "models", "optimizer", "scheduler", "i_batch", "rng", "window"}      # nothing new is saved
    rest = _walk(a, batches[1:], [None] * 3)
    b, _ = make(202, 1234)
    b.load_state_dict(state)
    again = _walk(b, batches[1:], [None] * 3)
    assert not torch.equal(rest.tables[0], first.tables[0]) and not torch.equal(rest.tables[0], rest.tables[1])
    for i in range(3):
        assert torch.equal(rest.tables[i], again.tables[i]), i
        assert torch.equal(rest.losses[i], again.losses[i]) and torch.equal(rest.kept[i], again.kept[i]), i


def test_float_frames_and_other_objects_are_refused(dev):
    from facialmmt_amd.train_step import GraphedTargetStep, TargetStep
    cfg, swin, mm = _models(dev)
    opt = torch.optim.SGD(mm.parameters(), lr=0.05)
    floats = RS._batches(dev, cfg, [5, 2])[0]                                      # (B, Lv, 3, 224, 224) float frames
    with pytest.raises(ValueError, match="uint8"):
        GraphedTargetStep(swin, mm, opt, None, cfg, floats, autocast_dtype=None, frame_capacity=CAP, color_jitter=ColorJitter())
    step = TargetStep(swin, mm, opt, None, cfg, autocast_dtype=None, frame_capacity=CAP, color_jitter=ColorJitter())
    bn = swin.swin.output_layer[3]
    with pytest.raises(ValueError, match="uint8"):
        step(floats)
    assert int(bn.num_batches_tracked) == 0                                        # refused in front of Swin
    for cls, extra in ((TargetStep, ()), (GraphedTargetStep, (floats,))):
        with pytest.raises(TypeError):
            cls(swin, mm, opt, None, cfg, *extra, autocast_dtype=None, color_jitter=dict(brightness=0.5))


def test_pipeline_swin_draws_inside_the_graph_of_swins_forward(dev):
    """pipeline_swin: the draw belongs to graph S, so the forward prefetched for the next call has its own table, which is the one `last_jitter` shows"""
    import bench
    from facialmmt_amd.train_step import GraphedTargetStep
    cfg, swin, mm = _models(dev)
    args = types.SimpleNamespace(utts=B, frames=LV, dtype="fp32", plm="roberta-large", input="u8", resize="cv2")
    batch = list(bench.synth_batch(args, dev, 0, cfg))                             # compact frames (B * Lv, 112, 112, 3), every slot real
    batch[0] = batch[0] % 1000
    batch = tuple(batch)
    step = GraphedTargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=0.05), None, cfg, batch, autocast_dtype=None, pipeline_swin=True,
                             color_jitter=ColorJitter())
    torch.manual_seed(5)
    seen, losses = [], []
    for nxt in (batch, batch, None):
        loss, kept = step(batch, next_batch=nxt)
        losses.append(float(loss))
        torch.cuda.synchronize()                                                   # the prefetched forward runs on a stream of its own
        seen.append(step.last_jitter.clone())
    _check_tables(seen, B * LV)
    assert all(torch.isfinite(torch.tensor(losses))) and float(kept.sum()) > 0
    assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[1], seen[2])      # two prefetched forwards, then none
