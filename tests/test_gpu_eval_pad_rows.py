"""GPU tests of GraphedEvalStep(pad_rows=True): the short last batch of a split padded to the captured rows (train_step.pad_target_batch), replayed in the
bucket its real frames pick, with the real row count in a device word that the captured metric update reads (ops.eval_accumulate_rows).

Shapes of tests/test_gpu_ragged_eval.py (tests/support_eval_pad.py): B = 2, Lv = 6, buckets (8, 12); a split of three batches, the last with one row.
Bars: against the launch-by-launch EvalStep(frame_capacity=bucket) fed the batch this test padded itself -- the same kernels on the same rows --
torch.equal on results, truths and accumulators.  Against the step WITHOUT pad_rows, whose 1-row batch runs unpadded through the eager step (another
M may pick another GEMM path): the project's fp32 parity bound, 1e-3 of the largest |logit|."""
import numpy as np
import pytest
import torch

from tests import support_eval_pad as SP

pytestmark = pytest.mark.gpu

B, NL, BUCKETS = SP.B, SP.NL, SP.BUCKETS
COUNTS = ([5, 2], [6, 6], [3])                                  # frames per utterance: buckets 8, 12, 8; the last batch has ONE row
_MODELS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _shared(dev):
    if "m" not in _MODELS:
        _MODELS["m"] = SP.build(dev)
    return _MODELS["m"]


@pytest.mark.parametrize("gumbel", ["off", "sample"])
def test_the_short_batch_is_replayed_and_equals_the_eager_step_on_the_padded_batch(dev, gumbel):
    from facialmmt_amd.eval_step import EvalStep, GraphedEvalStep, MeldMetrics
    from facialmmt_amd.train_step import pad_target_batch
    swin, mm, cfg = _shared(dev)
    batches = SP.split(dev, cfg, COUNTS, 70)
    step = GraphedEvalStep(swin, mm, cfg, batches[0], autocast_dtype=None, gumbel=gumbel, frame_capacity=BUCKETS, pad_rows=True,
                           metrics=MeldMetrics(NL, dev, collect_rows=8))
    assert step.metrics.result().count == 0 and int(step.metrics.cursor.item()) == 0 and step.padded_calls == 0 and step.rows is None
    step.metrics.results.fill_(-7.0)
    step.metrics.truths.fill_(-7)
    shared = MeldMetrics(NL, dev, collect_rows=8)               # the eager side collects too: it keeps the padded row, the host counts it out
    eager = {c: EvalStep(swin, mm, cfg, autocast_dtype=None, gumbel=gumbel, metrics=shared, frame_capacity=c) for c in BUCKETS}
    for i, (batch, bucket) in enumerate(zip(batches, (8, 12, 8))):
        b = len(batch[7])
        torch.manual_seed(900 + i)
        lg, mg = step(batch)
        assert step.capacity == bucket and step.rows == b and lg.shape == (b, NL) and mg.shape[0] == b
        lg, mg = lg.clone(), mg.clone()
        torch.manual_seed(900 + i)
        le, me = eager[bucket](pad_target_batch(batch, B))
        assert le.shape == (B, NL)
        assert torch.equal(lg, le[:b]), (i, (lg.float() - le[:b].float()).abs().max().item())
        assert torch.equal(mg, me[:b]), i
        assert torch.equal(step.frame_counts, eager[bucket].frame_counts) and step.frame_counts.tolist() == [sum(COUNTS[i])] * 2
    assert step.replays == 3 and step.fallbacks == 0 and step.padded_calls == 1
    results, truths = step.metrics.collected()
    assert results.shape == (5, NL) and int(step.metrics.cursor.item()) == 5 and int(shared.cursor.item()) == 6
    assert int(shared.truths[5].item()) == -100                 # the padded row: kept by the eager update, nowhere in the step's buffers
    assert torch.equal(results, shared.results[:5]) and torch.equal(truths, shared.truths[:5])
    assert torch.equal(truths, torch.cat([torch.as_tensor(x[7], device=dev) for x in batches]))
    assert bool((step.metrics.results[5:] == -7.0).all()) and bool((step.metrics.truths[5:] == -7).all())
    assert torch.equal(step.metrics.acc, shared.acc)            # loss-sum bits, count, confusion: the padded row's label is -100 on both sides
    assert step.metrics.result().count == 5


def test_against_the_fallback_of_the_step_without_pad_rows(dev):
    from facialmmt_amd.eval_step import GraphedEvalStep, MeldMetrics, evaluate
    swin, mm, cfg = _shared(dev)
    batches = SP.split(dev, cfg, COUNTS, 70)
    outs = []
    for pad in (False, True):
        step = GraphedEvalStep(swin, mm, cfg, batches[0], autocast_dtype=None, gumbel="off", frame_capacity=BUCKETS, pad_rows=pad,
                               metrics=MeldMetrics(NL, dev, collect_rows=8))
        loss, results, truths = evaluate(step, batches)
        assert (step.replays, step.fallbacks, step.padded_calls) == ((3, 0, 1) if pad else (2, 1, 0))
        outs.append((loss, results.clone(), truths.clone(), step.metrics.result()))
    (l0, r0, t0, m0), (l1, r1, t1, m1) = outs
    assert r0.shape == r1.shape == (5, NL) and torch.equal(t0, t1) and m0.count == m1.count == 5
    assert torch.equal(r0[:4], r1[:4])                          # the full batches: the same graphs
    scale = r0.abs().max().item()
    err = (r0[4] - r1[4]).abs().max().item()
    print(f"short batch, padded replay against unpadded eager step: |logits err| = {err:.3e}, largest |logit| = {scale:.3e}, bar {1e-3 * scale:.3e}")
    assert err <= 1e-3 * scale
    assert abs(l0 - l1) <= 1e-3 * scale


def test_without_collecting_metrics_the_step_hands_back_the_real_rows(dev):
    from facialmmt_amd.eval_step import GraphedEvalStep, MeldMetrics, evaluate
    swin, mm, cfg = _shared(dev)
    batches = SP.split(dev, cfg, COUNTS, 70)
    step = GraphedEvalStep(swin, mm, cfg, batches[0], autocast_dtype=None, gumbel="off", frame_capacity=BUCKETS, pad_rows=True)
    lg, mg = step(batches[2])
    assert lg.shape == (1, NL) and mg.shape[0] == 1 and step.rows == 1 and step.padded_calls == 1 and step.fallbacks == 0
    loss, results, truths = evaluate(step, batches)
    assert results.shape == (5, NL) and truths.shape == (5,) and step.metrics.result().count == 5 and step.fallbacks == 0 and step.padded_calls == 2
    collecting = GraphedEvalStep(swin, mm, cfg, batches[0], autocast_dtype=None, gumbel="off", frame_capacity=BUCKETS, pad_rows=True,
                                 metrics=MeldMetrics(NL, dev, collect_rows=5))
    loss2, results2, truths2 = evaluate(collecting, batches)
    assert torch.equal(results, results2) and torch.equal(truths, truths2) and loss == loss2
    assert np.array_equal(step.metrics.result().confusion, collecting.metrics.result().confusion)


def test_pad_rows_needs_frame_capacity(dev):
    from facialmmt_amd.eval_step import GraphedEvalStep
    swin, mm, cfg = _shared(dev)
    batch = SP.loader_batch(dev, cfg, [5, 2], 70)
    with pytest.raises(ValueError, match="pad_rows.*frame_capacity"):
        GraphedEvalStep(swin, mm, cfg, batch, gumbel="off", pad_rows=True)


def test_training_graphs_continue_bit_for_bit_after_a_padded_evaluation(dev):
    """the recipe of tests/test_gpu_ragged_eval.py::test_ragged_training_graphs_continue_bit_for_bit_after_a_ragged_evaluation, one training step on
    either side of an evaluation that ends in a padded replay"""
    from facialmmt_amd.eval_step import GraphedEvalStep, MeldMetrics, evaluate
    from facialmmt_amd.train_step import GraphedTargetStep

    def run(with_eval):
        swin, mm, cfg = SP.build(dev, tau=1e5, FacialEmoImpor_threshold=0.1)
        for m in swin.modules():
            if hasattr(m, "drop_prob"):
                m.drop_prob = 0.0
        batches = SP.split(dev, cfg, ([5, 2], [6, 6]), 0)
        opt = torch.optim.SGD(mm.parameters(), lr=0.05)
        step = GraphedTargetStep(swin, mm, opt, None, cfg, batches[0], autocast_dtype=None, frame_capacity=12)
        losses = []
        for i in range(2):
            if with_eval and i == 1:
                ev = GraphedEvalStep(swin, mm, cfg, batches[0], gumbel="sample", frame_capacity=BUCKETS, pad_rows=True, metrics=MeldMetrics(NL, dev, collect_rows=6))
                _, results, _ = evaluate(ev, SP.split(dev, cfg, COUNTS, 10))
                assert results.shape == (5, NL) and ev.replays == 3 and ev.fallbacks == 0 and ev.padded_calls == 1
                assert swin.training and mm.training
            torch.manual_seed(1234 + i)
            loss, _ = step(batches[i])
            losses.append(loss.clone())
        torch.cuda.synchronize()
        state = {f"{n}.{k}": v.detach().clone() for n, m in (("swin", swin), ("mm", mm)) for k, v in m.state_dict().items()}
        return losses, state

    l0, s0 = run(False)
    l1, s1 = run(True)
    for a, b in zip(l0, l1):
        assert torch.equal(a, b), (l0, l1)
    assert s0.keys() == s1.keys()
    for k in s0:
        if k.endswith("embed_positions._float_tensor"):         # a torch.FloatTensor(1) placeholder nothing ever writes or reads: uninitialised memory
            continue
        assert torch.equal(s0[k], s1[k]), k
