"""GPU tests of the auxiliary-task steps with augment= (the Aff-Wild2 train transform drawn on the device, inside graph A): on the small
configuration of tests/test_gpu_short_batch.py's auxiliary test -- fp32, DropPath off, SGD -- and its tolerances (losses 2e-4, parameters and
BatchNorm statistics 1e-4 of scale), with the images as uint8 112 x 112 crops, the 'pil' resize of the Aff-Wild2 path."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facialmmt_amd import ops
from facialmmt_amd.augment import AffWildAugment
from oracle import preproc as P
from tests import support_aff_augment as A
from tests import test_gpu_short_batch as SB

pytestmark = pytest.mark.gpu

B = 4
SEEDS = (1000, 1001, 1002)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _feed(dev, n=3):
    import bench
    imgs, labels = bench.synth_aux_batch(types.SimpleNamespace(aux_images=B * n, dtype="fp32", input="u8"), dev, 0)
    assert imgs.dtype == torch.uint8 and imgs.shape == (B * n, 112, 112, 3)
    return [(imgs[B * i:B * i + B].clone(), labels[B * i:B * i + B].clone()) for i in range(n)]


def _aug():
    return AffWildAugment(grayscale_p=0.5, jitter_p=0.5, blur_p=0.7, erase_p=0.6)        # every stage likely within a batch of four


def _walk(step, feed, seeds):
    out = types.SimpleNamespace(losses=[], tables=[])
    for (imgs, labels), seed in zip(feed, seeds):
        if seed is not None:
            torch.manual_seed(seed)
        out.losses.append(step(imgs, labels).clone())
        out.tables.append(None if step.last_augment is None else step.last_augment.clone())
    torch.cuda.synchronize()
    return out


def _end(swin):
    bn = swin.swin.output_layer[3]
    out = {k: v.detach().clone() for k, v in swin.named_parameters()}
    out.update(bn_mean=bn.running_mean.clone(), bn_var=bn.running_var.clone())
    return out


def _close(a, b, tol):
    for k in a:
        assert (a[k] - b[k]).abs().max().item() <= tol * max(1.0, a[k].abs().max().item()), k


def _check_tables(tables):
    from facialmmt_amd import _lib
    for t in tables:
        assert t.shape == (B, 20) and t.dtype == torch.int32
        assert _lib.load().fmmt_aug_table_check(t.cpu().contiguous().data_ptr(), B) == 0


@pytest.fixture(scope="module")
def eager(dev):
    """AuxStep(augment) over three batches, reseeded in front of every call; the patch embedding's inputs and output of the last call"""
    from facialmmt_amd.train_step import AuxStep
    cfg, swin = SB._aux_model(dev)
    step = AuxStep(swin, torch.optim.SGD(swin.parameters(), lr=0.02), None, cfg, augment=_aug())
    assert step.last_augment is None
    pe, seen = swin.swin.patch_embed, []
    real = pe.forward_u8

    def recorder(x, resize="pil", dtype=None, jitter=None, augment=None):
        y = real(x, resize, dtype, jitter=jitter, augment=augment)
        seen.append((x.clone(), resize, dtype, jitter, None if augment is None else augment.clone(), y.detach().clone(),
                     {k: v.detach().clone() for k, v in pe.state_dict().items()}))       # the step updates Swin: the weights this forward ran with
        return y
    pe.forward_u8 = recorder
    run = _walk(step, _feed(dev), SEEDS)
    pe.forward_u8 = real
    run.end, run.seen, run.pe = _end(swin), seen, pe
    return run


def test_graphed_replays_equal_the_eager_step_from_the_same_generator_state(dev, eager):
    from facialmmt_amd.train_step import GraphedAuxStep
    cfg, swin = SB._aux_model(dev)
    feed = _feed(dev)
    step = GraphedAuxStep(swin, torch.optim.SGD(swin.parameters(), lr=0.02), None, cfg, *feed[0], augment=_aug())
    g = _walk(step, feed, SEEDS)
    print("losses eager  ", [float(x) for x in eager.losses])
    print("losses graphed", [float(x) for x in g.losses])
    _check_tables(g.tables)
    for i, (a, b) in enumerate(zip(eager.tables, g.tables)):
        assert torch.equal(a, b), i                                               # the same draws
    assert not torch.equal(g.tables[0], g.tables[1])
    stages = torch.cat(g.tables)
    assert (stages[:, 8] & 1).any() and (stages[:, 9] >= 0).any() and (stages[:, 14] > 0).any() and (stages[:, 4:8] != 4).any()
    for a, b in zip(eager.losses, g.losses):
        assert abs(float(a) - float(b)) <= 2e-4 * max(1.0, abs(float(a))), (eager.losses, g.losses)
    _close(eager.end, _end(swin), 1e-4)                                            # three SGD updates: the gradients of every step
    more = _walk(step, [feed[0], feed[0]], [None, None])                           # no reseed: every replay draws anew
    assert not torch.equal(more.tables[0], more.tables[1]) and not torch.equal(more.tables[0], g.tables[-1])


def test_last_augment_fed_back_reproduces_the_patch_matrix(dev, eager):
    import copy
    x, resize, dtype, jitter, table, y, weights = eager.seen[-1]
    assert len(eager.seen) == 3 and resize == "pil" and jitter is None and x.dtype == torch.uint8 and x.shape == (B, 112, 112, 3)
    assert torch.equal(table, eager.tables[-1])
    pe = copy.deepcopy(eager.pe)
    pe.load_state_dict(weights)
    with torch.no_grad():
        assert torch.equal(pe.forward_u8(x, resize, dtype, augment=eager.tables[-1]), y)
        assert not torch.equal(pe.forward_u8(x, resize, dtype), y)
    host = table.cpu().numpy()
    want64, mask = A.erase(P.normalize_lut()[A.apply_table(P.resize_u8(x.cpu().numpy(), "pil"), host)].transpose(0, 3, 1, 2), host)
    want, inside = P.patch_cols(np.ascontiguousarray(want64)), P.patch_cols(np.ascontiguousarray(mask.astype(np.float32))) > 0
    got = ops.patch_embed_u8(x, "pil", torch.float32, augment=table).cpu().numpy()
    assert np.array_equal(got[~inside], want[~inside].astype(np.float32))
    assert inside.sum() == 0 or np.abs(got[inside] - want[inside]).max() <= 2e-5


def test_none_gives_the_bits_of_a_step_built_without_the_argument(dev, eager):
    from facialmmt_amd.train_step import AuxStep, GraphedAuxStep
    runs = []
    for kw in ({}, {"augment": None}):
        cfg, swin = SB._aux_model(dev)
        feed = _feed(dev)
        step = GraphedAuxStep(swin, torch.optim.SGD(swin.parameters(), lr=0.02), None, cfg, *feed[0], **kw)
        run = _walk(step, feed, SEEDS)
        assert step.last_augment is None and step.augment is None and run.tables == [None] * 3
        runs.append((run.losses, _end(swin)))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert abs(float(runs[0][0][0]) - float(eager.losses[0])) > 1e-6                # and the augmentation reaches the loss
    cfg, swin = SB._aux_model(dev)
    assert AuxStep(swin, None, None, cfg).last_augment is None


def test_short_batch_through_pad_rows(dev):
    """GraphedAuxStep(pad_rows=True, augment) on three images: the padded zero image gets a record too and leaves no trace -- an eager step on the
    three images with the first three records of `last_augment` gives the loss and the update"""
    from facialmmt_amd.train_step import AuxStep, GraphedAuxStep
    feed = _feed(dev, 2)
    short = (feed[1][0][:3].clone(), feed[1][1][:3].clone())
    cfg, swin_g = SB._aux_model(dev)
    step = GraphedAuxStep(swin_g, torch.optim.SGD(swin_g.parameters(), lr=0.02), None, cfg, *feed[0], pad_rows=True, augment=_aug())
    g = _walk(step, [feed[0], short], [41, 42])
    assert step.padded_calls == 1 and step.rows == 3 and g.tables[1].shape == (B, 20)
    cfg, swin_e = SB._aux_model(dev)
    opt = torch.optim.SGD(swin_e.parameters(), lr=0.02)
    ref = AuxStep(swin_e, opt, None, cfg, augment=_aug())
    e = _walk(ref, [feed[0]], [41])
    assert torch.equal(e.tables[0], g.tables[0])
    loss = swin_e(short[0], False, short[1], F.cross_entropy, augment=g.tables[1][:3])
    loss.backward()
    torch.nn.utils.clip_grad_norm_(swin_e.parameters(), cfg.clip)
    opt.step()
    print("losses eager", float(e.losses[0]), float(loss), "graphed", [float(x) for x in g.losses])
    for a, b in zip((e.losses[0], loss.detach()), g.losses):
        assert abs(float(a) - float(b)) <= 2e-4 * max(1.0, abs(float(a)))
    _close(_end(swin_e), _end(swin_g), 1e-4)


def test_a_saved_and_reloaded_step_continues_with_the_same_tables(dev):
    """the draws come from the device generator state_dict() already saves: no new state"""
    from facialmmt_amd.train_step import GraphedAuxStep, HFAdamW
    from facialmmt_amd import synth
    feed = _feed(dev)

    def make(model_seed, generator_seed):
        cfg, swin = SB._aux_model(dev)
        synth.fill_state_dict(swin, seed=model_seed)
        torch.manual_seed(generator_seed)
        opt = HFAdamW(swin.parameters(), lr=torch.tensor(1e-4, device=dev), weight_decay=0.01)
        return GraphedAuxStep(swin, opt, None, cfg, *feed[0], augment=_aug())
    a = make(100, 7)
    first = _walk(a, feed[:1], [None])
    state = a.state_dict()
    assert set(state) <= {"format", "kind", "models", "optimizer", "scheduler", "i_batch", "rng", "window"}      # nothing new is saved
    rest = _walk(a, feed[1:], [None, None])
    b = make(202, 1234)
    b.load_state_dict(state)
    again = _walk(b, feed[1:], [None, None])
    assert not torch.equal(rest.tables[0], first.tables[0]) and not torch.equal(rest.tables[0], rest.tables[1])
    for i in range(2):
        assert torch.equal(rest.tables[i], again.tables[i]), i
        assert torch.equal(rest.losses[i], again.losses[i]), i


def test_an_evaluation_between_replays_is_not_augmented_and_leaves_them_alone(dev):
    from facialmmt_amd.train_step import GraphedAuxStep

    def run(with_eval):
        cfg, swin = SB._aux_model(dev)
        feed = _feed(dev)
        step = GraphedAuxStep(swin, torch.optim.SGD(swin.parameters(), lr=0.02), None, cfg, *feed[0], augment=_aug())
        losses, tables = [], []
        for i in range(3):
            if with_eval and i == 2:
                held = step.last_augment.clone()
                swin.eval()
                with torch.no_grad():
                    logits = [swin(feed[0][0], False).clone() for _ in range(2)]
                swin.train()
                assert torch.equal(logits[0], logits[1])                          # no augmentation: an evaluation is a function of the batch
                assert torch.equal(step.last_augment, held)
            torch.manual_seed(1234 + i)
            losses.append(step(*feed[i]).clone())
            tables.append(step.last_augment.clone())
        torch.cuda.synchronize()
        return losses, tables, _end(swin)
    (l0, t0, e0), (l1, t1, e1) = run(False), run(True)
    for a, b in zip(l0 + t0, l1 + t1):
        assert torch.equal(a, b)
    for k in e0:
        assert torch.equal(e0[k], e1[k]), k
