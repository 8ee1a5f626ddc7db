"""GPU tests of evaluation on RAGGED batches: EvalStep / GraphedEvalStep(frame_capacity=...) fed the loader's (B, Lv, ...) padded frames and the real
counts, MeldMetrics(collect_rows=...) and evaluate() without per-batch clones.

Shapes of tests/test_gpu_ragged_step.py (B = 2, Lv = 6, stand-in text encoder); the padded frame slots hold random data, not zeros: packing, not
luck, has to remove them.  Bars: against the compact-frames path that existed before, logits to 1e-3 max(1, max|want|) under the guards of
tests/test_gpu_eval_step.py::test_eval_step_matches_hand_assembled_eager (fp32 compute), masks and counts exact; graph against launch by launch,
collected against cloned, and training with against without an evaluation: torch.equal."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facialmmt_amd import ops, synth

pytestmark = pytest.mark.gpu

B, LV, NL, CAP = 2, 6, 7, 12
SEQUENCE = ([5, 2], [6, 6], [1, 3])
# The head of the seeded synthetic weights answers close to 1/7 everywhere (importance ~ 0.143 for every frame); as in
# tests/test_gpu_eval_step.py::_head_params the classifier is scaled so that the frame filter has something to decide.
CLASSIFIER_SCALE = 4.0
# Per mode: the data seed (bench.synth_batch's rank) and, for "sample", where the search for the seed of each batch's noise table starts.  The seed of
# a batch is the first one from there on that meets the guards, which are computed from the fp64 importances and the logits of the step on the compact
# frames alone (choose_seed below), never from an output of the new path: "if a seed fails a guard, change the seed", done by the test itself so
# that the choice is the same rule on every machine.  Under the noise most rows lie above the threshold (sum p^2 of a 7-way softmax of logits with a
# Gumbel draw on top is rarely below 0.2), so a seed under which a batch drops a frame has to be looked for: the search asks that of EVERY batch.
CASES = {"off": ((0, 1, 2), (0, 0, 0)), "sample": ((0, 1, 2), (4336, 4341, 4350))}
SEED_SEARCH = 2000                                              # seeds tried per batch before the test gives up (a failure, not a skip)
SEED_MARGIN = 1e-2                                              # the search keeps ten times the distance to the threshold that the test asserts
_MODELS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _build(dev, act=torch.float32, **kw):
    """as tests/test_gpu_eval_step.py::_build: fp32 parameters, the stand-in text encoder, seeded weights"""
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    cfg = default_args(get_vision_utt_max_lens=LV, get_audio_utt_max_lens=24, trg_accumulation_steps=1, plm_module=synth.make_standin_plm(),
                       hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, crossmodal_attn_dropout_TA=0.0, crossmodal_attn_dropout_TA_V=0.0, **kw)
    cfg.compute_dtype = act
    swin = models.SwinForAffwildClassification(cfg)
    mm = models.MultiModalTransformerForClassification(cfg)
    synth.fill_state_dict(swin, seed=100)
    synth.fill_state_dict(mm, seed=200)
    with torch.no_grad():
        swin.classifier.weight.mul_(CLASSIFIER_SCALE)
    swin.to(dev).train()
    mm.to(dev).train()
    if act == torch.bfloat16:
        swin.swin.input_dtype = act
    return swin, mm, cfg


def _shared(dev, act=torch.float32):
    """one pair of models per dtype for the tests that only evaluate (an evaluation changes nothing in them)"""
    if act not in _MODELS:
        _MODELS[act] = _build(dev, act)
    return _MODELS[act]


def _ragged(dev, cfg, counts, rank, act=torch.float32):
    """(loader batch, compact batch) for the given frame counts: the same synthetic batch, frames (B, Lv, 3, 224, 224) with EVERY slot random;
    num_imgs a list in the loader batch (the reference's collate), a device tensor in the compact one"""
    import bench
    nb = len(counts)
    args = types.SimpleNamespace(utts=nb, frames=LV, dtype="bf16" if act == torch.bfloat16 else "fp32", plm="roberta-large", input="float", resize="pil")
    batch = list(bench.synth_batch(args, dev, rank, cfg))
    batch[0] = batch[0] % 1000                                  # ids within the stand-in encoder's vocabulary
    frames = batch[8].view(nb, LV, 3, 224, 224)
    vmask = torch.zeros(nb, LV, device=dev)
    for u, k in enumerate(counts):
        vmask[u, :k] = 1
    batch[6] = vmask
    padded, compact = list(batch), list(batch)
    padded[8], padded[9] = frames, list(counts)
    compact[8] = torch.cat([frames[u, :k] for u, k in enumerate(counts)], dim=0).contiguous()
    compact[9] = torch.tensor(counts, device=dev)
    return tuple(padded), tuple(compact)


def _on_device(batch):
    return batch[:9] + (torch.tensor(batch[9], device=batch[8].device),) + batch[10:]


class NoiseTable:
    """stands in for ops.gumbel_noise: the first n rows of ONE table, so that row i gets the same noise whatever n is (torch's own draw for n rows
    is no prefix of its draw for more).  A captured graph holds a view of the table: fill() writes in place."""

    def __init__(self, dev):
        self.table = torch.zeros(CAP, NL, device=dev)

    def fill(self, seed):
        g = torch.Generator(device=self.table.device).manual_seed(seed)
        self.table.copy_(-torch.empty(CAP, NL, device=self.table.device).exponential_(generator=g).log())

    def __call__(self, n, num_labels, device, dtype=torch.float32):
        assert n <= CAP and num_labels == NL
        return self.table[:n]


def features(swin, compact_frames):
    swin.eval()
    with torch.no_grad():
        feats = swin.swin(compact_frames)
    swin.train()
    return feats


def importance64(swin, feats, noise):
    """fp64 restatement of the head (src/models.py:28-32 + train.py:186-188) on the features of the compact frames"""
    h = torch.relu(feats.double() @ swin.linear.weight.double().t() + swin.linear.bias.double())
    logits = h @ swin.classifier.weight.double().t() + swin.classifier.bias.double()
    if noise is not None:
        logits = logits + noise.double()
    p = torch.softmax(logits / swin.tau, dim=1)
    return (p * p).sum(1)


def guards(imp64, thr, want):
    """the conditions under which a comparison against the compact path means something (from the reference side alone)"""
    margin = (imp64 - thr).abs().min().item()
    tol = 1e-3 * max(1.0, want.abs().max().item())
    top2 = want.double().topk(2, dim=1).values
    gap = (top2[:, 0] - top2[:, 1]).min().item()
    kept = int((imp64 > thr).sum())
    return margin, tol, gap, kept


def choose_seed(swin, feats, table, thr, start):
    """the seeds from `start` on under which, by the fp64 importances alone, no importance lies within SEED_MARGIN of the threshold and the batch
    drops a frame and keeps one; the caller takes the first whose reference logits also pass the top-two guard"""
    n = feats.shape[0]
    for seed in range(start, start + SEED_SEARCH):
        table.fill(seed)
        imp64 = importance64(swin, feats, table.table[:n])
        if (imp64 - thr).abs().min().item() > SEED_MARGIN and 0 < int((imp64 > thr).sum()) < n:
            yield seed


# ---------------------------------------------------------------------------------------------- 1. against the path that existed before
@pytest.mark.parametrize("gumbel", ["off", "sample"])
def test_graphed_ragged_step_equals_eval_step_on_compact_frames(dev, gumbel, monkeypatch):
    """[5, 2] -> [6, 6] -> [1, 3] through GraphedEvalStep(frame_capacity=12), every batch a REPLAY, against EvalStep on the compact frames"""
    from facialmmt_amd.eval_step import EvalStep, GraphedEvalStep
    swin, mm, cfg = _shared(dev)
    thr = cfg.FacialEmoImpor_threshold
    table = NoiseTable(dev)
    monkeypatch.setattr(ops, "gumbel_noise", table)
    ranks, seeds = CASES[gumbel]
    pairs = [_ragged(dev, cfg, counts, rank) for counts, rank in zip(SEQUENCE, ranks)]
    table.fill(seeds[0])
    eager = EvalStep(swin, mm, cfg, autocast_dtype=None, gumbel=gumbel)
    graphed = GraphedEvalStep(swin, mm, cfg, pairs[0][0], autocast_dtype=None, gumbel=gumbel, frame_capacity=CAP)
    assert graphed.metrics.result().count == 0
    dropped = 0
    for i, ((padded, compact), counts, seed) in enumerate(zip(pairs, SEQUENCE, seeds)):
        n = sum(counts)
        feats = features(swin, compact[8])
        counted = eager.metrics.acc.clone()
        for seed in choose_seed(swin, feats, table, thr, seed) if gumbel == "sample" else (seed,):
            table.fill(seed)
            eager.metrics.acc.copy_(counted)                    # a seed given up below has counted nothing
            want, want_mask = eager(compact)
            want, want_mask = want.float().clone(), want_mask.clone()
            imp64 = importance64(swin, feats, table.table[:n] if gumbel == "sample" else None)
            margin, tol, gap, kept = guards(imp64, thr, want)
            if gap > 10 * tol or gumbel == "off":
                break
        else:
            pytest.fail(f"batch {i}: no seed in {SEED_SEARCH} meets the guards")
        print(f"{gumbel} batch {i} counts {counts} seed {seed}: min |importance - threshold| = {margin:.3e}, kept {kept} of {n}, min top-two gap = {gap:.3e}, tol = {tol:.1e}")
        assert margin > 1e-3, "an importance lies within 1e-3 of the threshold: change the seed"
        assert gap > tol, "a row's top-two logits are closer than the tolerance: change the seed"
        dropped += 0 < kept < n
        got, got_mask = graphed(padded if i != 1 else _on_device(padded))          # the middle batch with num_imgs on the device
        err = (got.float() - want).abs().max().item()
        print(f"{gumbel} batch {i}: |logits err| = {err:.3e}")
        assert err <= tol
        assert torch.equal(got_mask, want_mask)
        assert graphed.frame_counts.tolist() == [n, n] and graphed.importance.shape == (CAP,)
        assert (graphed.importance[:n].double() - imp64).abs().max().item() <= 1e-3
    assert dropped >= 1, "no batch dropped a frame: the filter decided nothing"
    r0, r1 = eager.metrics.result(), graphed.metrics.result()
    assert np.array_equal(r0.confusion, r1.confusion) and r0.count == r1.count == 3 * B
    assert graphed.replays == len(pairs) and graphed.fallbacks == 0


# ---------------------------------------------------------------------------------------------- 2. graph == launch by launch
@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_bucketed_graphs_equal_the_launch_by_launch_step_bit_for_bit(dev, act):
    from facialmmt_amd.eval_step import EvalStep, GraphedEvalStep, MeldMetrics
    swin, mm, cfg = _shared(dev, act)
    ac = torch.bfloat16 if act == torch.bfloat16 else None
    padded = [_ragged(dev, cfg, counts, rank=20 + i, act=act)[0] for i, counts in enumerate(([5, 2], [6, 6], [1, 3]))]
    graphed = GraphedEvalStep(swin, mm, cfg, padded[1], autocast_dtype=ac, gumbel="sample", frame_capacity=(8, 12))      # the sample batch: 12 frames
    assert graphed.metrics.result().count == 0                  # warm-up and capture of both buckets counted nothing
    shared = MeldMetrics(NL, dev)
    eager = {c: EvalStep(swin, mm, cfg, autocast_dtype=ac, gumbel="sample", metrics=shared, frame_capacity=c) for c in (8, 12)}
    calls = [(padded[0], 8, 7), (padded[1], 12, 12), (padded[2], 8, 4), (_on_device(padded[0]), 12, 7), (_on_device(padded[2]), 12, 4)]
    for i, (batch, bucket, total) in enumerate(calls):
        torch.manual_seed(900 + i)
        lg, mg = graphed(batch)
        assert graphed.capacity == bucket, (i, graphed.capacity)
        torch.manual_seed(900 + i)
        le, me = eager[bucket](batch)
        assert lg.shape == le.shape and torch.equal(lg, le), (i, (lg.float() - le.float()).abs().max().item())
        assert torch.equal(mg, me), i
        assert torch.equal(graphed.frame_counts, eager[bucket].frame_counts) and graphed.frame_counts.tolist() == [total, total], i
        assert torch.equal(graphed.importance, eager[bucket].importance) and graphed.importance.shape == (bucket,)
        assert torch.equal(graphed.metrics.acc, shared.acc), i
    assert graphed.replays == len(calls) and graphed.fallbacks == 0
    first = None
    for rep in range(12):                                       # twelve replays of one batch
        graphed.metrics.reset()
        torch.manual_seed(31)
        lg, mg = graphed(padded[0])
        cur = (lg.clone(), mg.clone(), graphed.metrics.acc.clone(), graphed.frame_counts.clone())
        first = first or cur
        assert all(torch.equal(a, b) for a, b in zip(first, cur)), rep


# ---------------------------------------------------------------------------------------------- 3. a whole split
def test_evaluate_collects_a_ragged_split_without_clones(dev):
    from facialmmt_amd.eval_step import GraphedEvalStep, MeldMetrics, evaluate
    swin, mm, cfg = _shared(dev)
    split = [_ragged(dev, cfg, counts, rank=40 + i)[0] for i, counts in enumerate(([5, 2], [6, 6], [1, 3]))]
    ignored = list(split[2])
    ignored[7] = torch.tensor([int(split[2][7][0]), -100], device=dev)
    split[2] = tuple(ignored)
    split.append(_ragged(dev, cfg, [4], rank=47)[0])            # the short last batch: B = 1, another shape
    outs = []
    for collect in (None, 8):                                   # 7 rows in buffers of 8
        step = GraphedEvalStep(swin, mm, cfg, split[0], autocast_dtype=None, gumbel="sample", frame_capacity=(8, 12),
                               metrics=MeldMetrics(NL, dev, collect_rows=collect))
        torch.manual_seed(55)
        loss, results, truths = evaluate(step, split)
        assert step.replays == 3 and step.fallbacks == 1
        outs.append((loss, results.clone(), truths.clone(), step.metrics.result()))
    (l0, r0, t0, m0), (l1, r1, t1, m1) = outs
    assert l0 == l1 and torch.equal(r0, r1) and torch.equal(t0, t1)
    assert r1.shape == (3 * B + 1, NL) and r1.dtype == torch.float32 and t1.dtype == torch.int64 and int(t1[5]) == -100
    assert m1.count == m0.count == 3 * B and np.array_equal(m0.confusion, m1.confusion)
    ok = t1 >= 0
    want = F.cross_entropy(r1[ok].double(), t1[ok], reduction="mean").item()
    assert abs(l1 - want) <= 1e-5 * abs(want)
    # a split longer than the buffers: everything is counted, collected() refuses
    small = GraphedEvalStep(swin, mm, cfg, split[0], autocast_dtype=None, gumbel="off", frame_capacity=CAP, metrics=MeldMetrics(NL, dev, collect_rows=5))
    with pytest.raises(ValueError, match="7 rows.*collect_rows=5"):
        evaluate(small, split)
    assert small.metrics.result().count == 3 * B


# ---------------------------------------------------------------------------------------------- 4. errors
def test_too_many_frames_and_compact_frames_raise_before_anything_is_launched(dev):
    from facialmmt_amd.eval_step import EvalStep, GraphedEvalStep
    swin, mm, cfg = _shared(dev)
    fits, fits_compact = _ragged(dev, cfg, [5, 2], rank=60)
    full, _ = _ragged(dev, cfg, [6, 6], rank=61)
    with pytest.raises(ValueError, match="frame_capacity=8"):                    # the constructor's sample batch is checked the same way
        GraphedEvalStep(swin, mm, cfg, full, gumbel="sample", frame_capacity=(4, 8))
    with pytest.raises(ValueError, match="ascending"):
        GraphedEvalStep(swin, mm, cfg, fits, gumbel="sample", frame_capacity=(8, 8))
    with pytest.raises(ValueError, match="frame_capacity"):
        GraphedEvalStep(swin, mm, cfg, fits_compact, gumbel="sample", frame_capacity=8)
    step = GraphedEvalStep(swin, mm, cfg, fits, gumbel="sample", frame_capacity=(4, 8))
    torch.cuda.synchronize()
    before = (step.metrics.acc.clone(), [t.clone() for t in step.static], torch.cuda.get_rng_state(dev))
    for bad in (full, fits_compact):
        with pytest.raises(ValueError, match="frame_capacity"):
            step(bad)
    with pytest.raises(ValueError, match="frame_capacity"):
        EvalStep(swin, mm, cfg, gumbel="sample", metrics=step.metrics, frame_capacity=8)(fits_compact)
    with pytest.raises(ValueError, match="frame_capacity=8"):
        EvalStep(swin, mm, cfg, gumbel="sample", metrics=step.metrics, frame_capacity=8)(full)
    torch.cuda.synchronize()
    assert torch.equal(step.metrics.acc, before[0]) and all(torch.equal(a, b) for a, b in zip(step.static, before[1]))
    assert torch.equal(torch.cuda.get_rng_state(dev), before[2])
    assert step.replays == 0 and step.fallbacks == 0
    logits, kept = step(fits)                                                    # and the step still works
    assert step.capacity == 8 and step.frame_counts.tolist() == [7, 7] and bool(torch.isfinite(logits).all()) and float(kept.sum()) > 0
    assert step.replays == 1 and step.metrics.result().count == B


# ---------------------------------------------------------------------------------------------- 5. training is untouched
def test_ragged_training_graphs_continue_bit_for_bit_after_a_ragged_evaluation(dev):
    """the recipe of tests/test_gpu_eval_step.py::test_training_graphs_continue_bit_for_bit_after_an_evaluation with
    GraphedTargetStep(frame_capacity=12) and a bucketed ragged evaluation in between"""
    from facialmmt_amd.eval_step import GraphedEvalStep, MeldMetrics
    from facialmmt_amd.train_step import GraphedTargetStep

    def run(with_eval):
        swin, mm, cfg = _build(dev, tau=1e5, FacialEmoImpor_threshold=0.1)
        for m in swin.modules():
            if hasattr(m, "drop_prob"):
                m.drop_prob = 0.0
        batches = [_ragged(dev, cfg, counts, rank=i)[0] for i, counts in enumerate(SEQUENCE)]
        opt = torch.optim.SGD(mm.parameters(), lr=0.05)
        step = GraphedTargetStep(swin, mm, opt, None, cfg, batches[0], autocast_dtype=None, frame_capacity=CAP)
        losses = []
        for i in range(4):
            if with_eval and i == 2:
                before = [m.training for model in (swin, mm) for m in model.modules()]
                ev = GraphedEvalStep(swin, mm, cfg, batches[0], gumbel="sample", frame_capacity=(8, 12), metrics=MeldMetrics(NL, dev, collect_rows=3 * B))
                for k in range(3):
                    ev(_ragged(dev, cfg, SEQUENCE[k], rank=10 + k)[0])
                assert ev.metrics.result().count == 3 * B and ev.replays == 3 and ev.metrics.collected()[0].shape == (3 * B, NL)
                assert [m.training for model in (swin, mm) for m in model.modules()] == before and swin.training and mm.training
            torch.manual_seed(1234 + i)
            loss, _ = step(batches[i % 3])
            losses.append(loss.clone())
        torch.cuda.synchronize()
        state = {f"{n}.{k}": v.detach().clone() for n, m in (("swin", swin), ("mm", mm)) for k, v in m.state_dict().items()}
        return losses, state

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert not torch.equal(l0[0], l0[3])                        # the optimizer moved something
    for a, b in zip(l0, l1):
        assert torch.equal(a, b), (l0, l1)
    assert s0.keys() == s1.keys()
    assert any("running_mean" in k for k in s0)
    for k in s0:                                                # parameters and BatchNorm running statistics
        if k.endswith("embed_positions._float_tensor"):         # a torch.FloatTensor(1) placeholder nothing ever writes or reads: uninitialised memory
            continue
        assert torch.equal(s0[k], s1[k]), k
