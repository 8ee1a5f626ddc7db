"""GPU tests of the evaluation step (facialmmt_amd/eval_step.py, csrc/eval.hip): the two entry points against fp64 / numpy restatements written
here, EvalStep against the hand-assembled eager sequence on the existing modules, GraphedEvalStep against EvalStep bit for bit, training graphs
undisturbed by an evaluation in between, the unimodal step, and torch.library.opcheck on the two operators.

Bars: probabilities to 1e-3 absolute (the project's fp32 parity bar, 1e-3 of the output's scale); counts, argmax and masks exact; the loss sum to
1e-5 relative against fp64 (a 7-term fp32 log-sum-exp carries a few ulp per row, the sum itself is a double)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facialmmt_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu

NL = 7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import facialmmt_amd.torch_ops  # noqa: F401
    return torch.device("cuda:0")


def _head64(feats, w1, b1, w2, b2, gumbel, tau):
    """fp64 restatement of src/models.py:28-32 (target task) + train.py:186-188"""
    h = torch.relu(feats.double() @ w1.double().t() + b1.double())
    logits = h @ w2.double().t() + b2.double()
    if gumbel is not None:
        logits = logits + gumbel.double()
    p = torch.softmax(logits / tau, dim=1)
    return p, (p * p).sum(1)


def _head_params(dev, seed=3):
    torch.manual_seed(seed)
    lin, cls = torch.nn.Linear(512, 64).to(dev), torch.nn.Linear(64, NL).to(dev)
    with torch.no_grad():
        cls.weight.mul_(4.0)                                   # spread the distribution: a head that answers 1/7 everywhere tests little
    return lin, cls


# ---------------------------------------------------------------------------------------------- 1. fmmt_emotion_head_fwd
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [1, 7, 160, 640, 1000])
def test_emotion_head_matches_fp64(dev, dtype, N):
    lin, cls = _head_params(dev)
    g = torch.Generator(device=dev).manual_seed(10 + N)
    wide = (torch.randn(N, 640, generator=g, device=dev) * 1.5).to(dtype)
    for name, feats in (("contiguous", wide[:, :512].contiguous()), ("strided", wide[:, 64:576])):
        for noise in (False, True):
            for tau in (1.0, 0.5):
                gum = -torch.empty(N, NL, device=dev).exponential_(generator=g).log() if noise else None
                with torch.no_grad():
                    preds, imp = ops.emotion_head(feats, lin, cls, tau, gum)
                want, want_imp = _head64(feats, lin.weight, lin.bias, cls.weight, cls.bias, gum, tau)
                assert preds.shape == (N, NL) and preds.dtype == torch.float32 and imp.shape == (N,)
                e1, e2 = (preds.double() - want).abs().max().item(), (imp.double() - want_imp).abs().max().item()
                print(f"emotion_head {name} N={N} {dtype} noise={noise} tau={tau}: |preds err|={e1:.2e} |importance err|={e2:.2e}")
                assert e1 <= 1e-3 and e2 <= 1e-3, (name, noise, tau, e1, e2)
                assert (preds.sum(1) - 1).abs().max().item() <= 1e-5


def test_emotion_head_matches_the_module_under_one_seed(dev):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    swin = models.SwinForAffwildClassification(default_args())
    synth.fill_state_dict(swin, seed=100)
    swin.to(dev).eval()
    frames = synth.tensor("frames", (5, 3, 224, 224), seed=1).to(dev)
    with torch.no_grad():
        torch.manual_seed(77)
        want = swin(frames, is_trg_task=True)
        torch.manual_seed(77)
        feats = swin.swin(frames)
        preds, imp = ops.emotion_head(feats, swin.linear, swin.classifier, swin.tau, ops.gumbel_noise(5, NL, dev))
        plain, _ = ops.emotion_head(feats, swin.linear, swin.classifier, swin.tau, None)
    e = (preds - want).abs().max().item()
    print(f"emotion_head vs module: {e:.2e}")
    assert e <= 1e-3
    assert (imp - (want * want).sum(1)).abs().max().item() <= 1e-3
    assert (plain - torch.softmax(swin(frames) / swin.tau, dim=1)).abs().max().item() <= 1e-3
    with pytest.raises(NotImplementedError):
        ops.emotion_head(feats.clone().requires_grad_(True), swin.linear, swin.classifier, swin.tau)
    with torch.no_grad(), pytest.raises(_lib.FmmtError):
        ops.emotion_head(feats[:, :500], swin.linear, swin.classifier, swin.tau)


# ---------------------------------------------------------------------------------------------- 2. fmmt_eval_accumulate
def _acc_reference(logits, labels):
    lg = logits.float().cpu().numpy()
    lab = labels.cpu().numpy()
    arg = np.argmax(lg, axis=1)
    ok = lab >= 0
    conf = np.zeros((NL, NL), dtype=np.int64)
    np.add.at(conf, (lab[ok], arg[ok]), 1)
    lab64 = torch.from_numpy(np.where(ok, lab, -100))
    loss = F.cross_entropy(logits.double().cpu(), lab64, reduction="sum", ignore_index=-100).item() if ok.any() else 0.0
    return arg, conf, int(ok.sum()), loss


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_eval_accumulate_matches_numpy(dev, dtype):
    from facialmmt_amd.eval_step import MeldMetrics
    g = torch.Generator(device=dev).manual_seed(5)
    runs = []
    for rep in range(2):
        m = MeldMetrics(NL, dev)
        conf, count, loss = np.zeros((NL, NL), dtype=np.int64), 0, 0.0
        keep = torch.full((1024 + 1 + 300, NL), -1.0, device=dev)
        off = 0
        g.manual_seed(5)
        for B in (1024, 1, 300):                                # three successive updates into the same accumulators
            logits = (torch.randn(B, NL, generator=g, device=dev) * 3).to(dtype)
            labels = torch.randint(0, NL, (B,), generator=g, device=dev)
            if B > 1:
                logits[::5, 4] = logits[::5, 2] = logits[::5].max(dim=1).values + 1     # ties: the first maximum (class 2) wins
                logits[3] = 0.5                                                          # all equal: class 0
                labels[::7] = -100                                                       # ignored rows
                labels[1] = -1
            pred = m.update(logits, labels, logits_out=keep, out_offset=off, pred=True)
            arg, c, n, l = _acc_reference(logits, labels)
            assert np.array_equal(pred.cpu().numpy(), arg), B
            assert torch.equal(keep[off:off + B], logits.float())
            conf, count, loss, off = conf + c, count + n, loss + l, off + B
        r = m.result()
        assert np.array_equal(r.confusion, conf) and r.count == count
        rel = abs(r.loss_sum - loss) / abs(loss)
        print(f"eval_accumulate {dtype}: loss sum {r.loss_sum!r} against fp64 {loss!r}: rel {rel:.2e}")
        assert rel <= 1e-5
        assert abs(r.avg_loss - loss / count) <= 1e-5 * abs(loss / count)
        runs.append(m.acc.clone())
    assert torch.equal(runs[0], runs[1])                        # bit-identical, the loss sum's double included
    m = MeldMetrics(NL, dev)
    m.update(torch.zeros(4, NL, device=dev), torch.full((4,), -100, device=dev))
    assert m.result().count == 0 and m.result().loss_sum == 0.0
    with pytest.raises(_lib.FmmtError):
        m.update(torch.zeros(1025, NL, device=dev), torch.zeros(1025, dtype=torch.int64, device=dev))
    with pytest.raises(NotImplementedError):
        m.update(torch.zeros(4, NL, device=dev, requires_grad=True), torch.zeros(4, dtype=torch.int64, device=dev))


# ---------------------------------------------------------------------------------------------- models for 3-5
def _cfg(B, Lv, act, **kw):
    from facialmmt_amd.config import default_args
    cfg = default_args(get_vision_utt_max_lens=Lv, get_audio_utt_max_lens=24, trg_accumulation_steps=1, plm_module=synth.make_standin_plm(),
                       hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, crossmodal_attn_dropout_TA=0.0, crossmodal_attn_dropout_TA_V=0.0, **kw)
    cfg.compute_dtype = act
    return cfg


def _build(dev, act=torch.float32, B=2, Lv=6, **kw):
    """as tests/test_gpu_train_step.py::_build: fp32 parameters, the stand-in text encoder, seeded weights"""
    from facialmmt_amd import models
    cfg = _cfg(B, Lv, act, **kw)
    swin = models.SwinForAffwildClassification(cfg)
    mm = models.MultiModalTransformerForClassification(cfg)
    synth.fill_state_dict(swin, seed=100)
    synth.fill_state_dict(mm, seed=200)
    swin.to(dev).train()
    mm.to(dev).train()
    if act == torch.bfloat16:
        swin.swin.input_dtype = act
    return swin, mm, cfg


def _batch(dev, cfg, B, Lv, rank, act=torch.float32):
    import bench
    args = types.SimpleNamespace(utts=B, frames=Lv, dtype="bf16" if act == torch.bfloat16 else "fp32", plm="roberta-large", input="float", resize="pil")
    batch = list(bench.synth_batch(args, dev, rank, cfg))
    batch[0] = batch[0] % 1000                                  # ids within the stand-in encoder's vocabulary
    return tuple(batch)


def _modes(*models):
    return [m.training for model in models for m in model.modules()]


# ---------------------------------------------------------------------------------------------- 3. EvalStep against the eager sequence
def test_eval_step_matches_hand_assembled_eager(dev):
    from facialmmt_amd.eval_step import EvalStep, confusion_matrix
    from facialmmt_amd.train_step import select_frames
    B, Lv = 2, 6
    swin, mm, cfg = _build(dev)
    thr = cfg.FacialEmoImpor_threshold
    step = EvalStep(swin, mm, cfg, autocast_dtype=None, gumbel="sample")
    before = _modes(swin, mm)
    conf = np.zeros((NL, NL), dtype=np.int64)
    # seeds: chosen from the fp64 importances alone (every frame further than 5e-3 from the threshold AND some frames dropped, so the filter decides
    # something), before any output of the step was looked at
    for i, seed in enumerate((4336, 4341, 4336)):
        batch = _batch(dev, cfg, B, Lv, rank=i)
        (ids, attn_mask, sep_mask, audio, audio_mask, vision, vision_mask, labels, frames, num_imgs, utt_idx) = batch
        # the eager evaluation a user assembles from the existing modules
        swin.eval()
        mm.eval()
        with torch.no_grad():
            torch.manual_seed(seed)
            preds = swin(frames, is_trg_task=True)
            vis, want_mask = select_frames(preds.float(), vision, vision_mask, num_imgs, thr)
            want = mm(ids, attn_mask, sep_mask, audio, audio_mask, vis, want_mask, utt_idx).float()
            # the conditions under which the comparison means something: no importance within 1e-3 of the threshold (fp64), no near-tie of logits
            torch.manual_seed(seed)
            feats = swin.swin(frames)
            noise = ops.gumbel_noise(feats.shape[0], NL, dev)
            _, imp64 = _head64(feats, swin.linear.weight, swin.linear.bias, swin.classifier.weight, swin.classifier.bias, noise, swin.tau)
        swin.train()
        mm.train()
        margin = (imp64 - thr).abs().min().item()
        scale = max(1.0, want.abs().max().item())
        tol = 1e-3 * scale
        top2 = want.double().topk(2, dim=1).values
        gap = (top2[:, 0] - top2[:, 1]).min().item()
        print(f"batch {i} seed {seed}: min |importance - threshold| = {margin:.3e}, kept {int((imp64 > thr).sum())} of {imp64.numel()}, min top-two gap = {gap:.3e}, tol = {tol:.1e}")
        assert margin > 1e-3, "an importance lies within 1e-3 of the threshold: change the seed"
        assert gap > tol, "a row's top-two logits are closer than the tolerance: change the seed"
        torch.manual_seed(seed)
        got, got_mask = step(batch)
        err = (got.float() - want).abs().max().item()
        print(f"batch {i}: |logits err| = {err:.3e}")
        assert err <= tol
        assert torch.equal(got_mask, want_mask)
        assert (step.importance.double() - imp64).abs().max().item() <= 1e-3
        conf += confusion_matrix(want.argmax(1).cpu().numpy(), labels.cpu().numpy(), NL)
        assert _modes(swin, mm) == before                      # back in training mode, module by module
    r = step.metrics.result()
    assert np.array_equal(r.confusion, conf) and r.count == 3 * B
    # "off": deterministic, consumes no random numbers, equals the noise-free module
    off = EvalStep(swin, mm, cfg, gumbel="off")
    state = torch.cuda.get_rng_state(dev)
    a = off(batch)[0].clone()
    assert torch.equal(torch.cuda.get_rng_state(dev), state)
    assert torch.equal(a, off(batch)[0])


# ---------------------------------------------------------------------------------------------- 4. GraphedEvalStep == EvalStep
@pytest.mark.parametrize("act", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graphed_eval_step_equals_eval_step_bit_for_bit(dev, act):
    from facialmmt_amd.eval_step import EvalStep, GraphedEvalStep, evaluate
    B, Lv = 2, 6
    swin, mm, cfg = _build(dev, act)
    ac = torch.bfloat16 if act == torch.bfloat16 else None
    batches = [_batch(dev, cfg, B, Lv, rank=i, act=act) for i in range(3)] + [_batch(dev, cfg, 1, Lv, rank=7, act=act)]     # the last one: another shape
    eager = EvalStep(swin, mm, cfg, autocast_dtype=ac, gumbel="sample")
    before = _modes(swin, mm)
    graphed = GraphedEvalStep(swin, mm, cfg, batches[0], autocast_dtype=ac, gumbel="sample")
    assert _modes(swin, mm) == before
    assert graphed.metrics.result().count == 0                  # warm-up and capture counted nothing
    for i, batch in enumerate(batches):
        torch.manual_seed(900 + i)
        le, me = eager(batch)
        le, me = le.clone(), me.clone()
        torch.manual_seed(900 + i)
        lg, mg = graphed(batch)
        assert lg.shape == le.shape and torch.equal(lg, le), (i, (lg.float() - le.float()).abs().max().item())
        assert torch.equal(mg, me), i
        assert torch.equal(graphed.metrics.acc, eager.metrics.acc), i
    assert graphed.metrics.result().count == 3 * B + 1
    first = None
    for rep in range(12):                                       # twelve replays of one batch
        graphed.metrics.reset()
        torch.manual_seed(31)
        lg, mg = graphed(batches[1])
        cur = (lg.clone(), mg.clone(), graphed.metrics.acc.clone())
        first = first or cur
        assert all(torch.equal(a, b) for a, b in zip(first, cur)), rep
    # a whole "split" through evaluate(): same numbers from both steps, labels of padded rows ignored
    padded = list(batches[2])
    padded[7] = torch.tensor([int(batches[2][7][0]), -100], device=dev)
    split = batches[:2] + [tuple(padded), batches[3]]
    outs = []
    for s in (eager, graphed):
        torch.manual_seed(55)
        loss, results, truths = evaluate(s, split)
        outs.append((loss, results, truths, s.metrics.result()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert outs[1][3].count == 2 * B + 1 + 1 and outs[1][1].shape == (3 * B + 1, NL)
    ok = outs[1][2] >= 0
    want = F.cross_entropy(outs[1][1][ok].double(), outs[1][2][ok], reduction="mean").item()
    assert abs(outs[1][0] - want) <= 1e-5 * abs(want)


# ---------------------------------------------------------------------------------------------- 5. training is untouched
def test_training_graphs_continue_bit_for_bit_after_an_evaluation(dev):
    from facialmmt_amd.eval_step import GraphedEvalStep
    from facialmmt_amd.train_step import GraphedTargetStep
    B, Lv = 2, 6

    def run(with_eval):
        swin, mm, cfg = _build(dev, tau=1e5, FacialEmoImpor_threshold=0.1)
        for m in swin.modules():
            if hasattr(m, "drop_prob"):
                m.drop_prob = 0.0
        batch = _batch(dev, cfg, B, Lv, rank=0)
        opt = torch.optim.SGD(mm.parameters(), lr=0.05)
        step = GraphedTargetStep(swin, mm, opt, None, cfg, batch, autocast_dtype=None)
        losses = []
        for i in range(4):
            if with_eval and i == 2:
                before = _modes(swin, mm)
                ev = GraphedEvalStep(swin, mm, cfg, batch, gumbel="sample")
                for k in range(3):
                    ev(_batch(dev, cfg, B, Lv, rank=10 + k))
                assert ev.metrics.result().count == 3 * B
                assert _modes(swin, mm) == before and swin.training and mm.training
            torch.manual_seed(1234 + i)
            loss, _ = step(batch)
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


# ---------------------------------------------------------------------------------------------- 6. unimodal
def test_unimodal_eval_step(dev):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    from facialmmt_amd.eval_step import UnimodalEvalStep, confusion_matrix, evaluate, f1_from_confusion
    cfg = default_args(get_vision_utt_max_lens=12)
    cfg.compute_dtype = torch.float32
    model = models.meld_utt_transformer(cfg)
    synth.fill_state_dict(model, seed=300)
    model.to(dev).train()
    g = torch.Generator(device=dev).manual_seed(8)
    loader = []
    for B in (5, 5, 3):
        mask = torch.zeros(B, 12, device=dev)
        mask[:, :9] = 1
        loader.append((torch.randn(B, 12, cfg.vision_featExtr_dim, generator=g, device=dev), mask, torch.randint(0, NL, (B,), generator=g, device=dev)))
    step = UnimodalEvalStep(model, cfg)
    loss, results, truths = evaluate(step, loader)
    assert model.training
    model.eval()
    with torch.no_grad():
        want = torch.cat([model(x, m) for x, m, _ in loader]).float()
    model.train()
    labels = torch.cat([l for _, _, l in loader])
    assert (results - want).abs().max().item() <= 1e-3 * max(1.0, want.abs().max().item())
    assert torch.equal(truths, labels)
    want_loss = F.cross_entropy(results.double(), labels, reduction="mean").item()
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    conf = confusion_matrix(results.argmax(1).cpu().numpy(), labels.cpu().numpy(), NL)
    r = step.metrics.result()
    assert np.array_equal(r.confusion, conf) and r.count == 13
    assert r.weighted_f1 == f1_from_confusion(conf)[0]


# ---------------------------------------------------------------------------------------------- 7. torch.ops.fmmt
def test_operators_match_front_end_and_pass_opcheck(dev):
    lin, cls = _head_params(dev)
    feats = torch.randn(40, 512, device=dev).bfloat16()
    gum = ops.gumbel_noise(40, NL, dev)
    with torch.no_grad():
        a = torch.ops.fmmt.emotion_head(feats, lin.weight, lin.bias, cls.weight, cls.bias, gum, 0.5)
        b = ops.emotion_head(feats, lin, cls, 0.5, gum)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    logits, labels = torch.randn(33, NL, device=dev), torch.randint(0, NL, (33,), device=dev)
    acc1, acc2 = torch.zeros(2 + NL * NL, dtype=torch.int64, device=dev), torch.zeros(2 + NL * NL, dtype=torch.int64, device=dev)
    keep = torch.zeros(40, NL, device=dev)
    p1 = torch.ops.fmmt.eval_accumulate(logits, labels, acc1, keep, 5)
    p2 = ops.eval_accumulate(logits, labels, acc2)
    assert torch.equal(p1, p2) and torch.equal(acc1, acc2) and torch.equal(keep[5:38], logits)
    tests = ("test_schema", "test_faketensor")
    w = [t.detach() for t in (lin.weight, lin.bias, cls.weight, cls.bias)]
    torch.library.opcheck(torch.ops.fmmt.emotion_head.default, (feats, *w, gum, 0.5), test_utils=tests)
    torch.library.opcheck(torch.ops.fmmt.emotion_head.default, (feats.float(), *w, None, 1.0), test_utils=tests)
    torch.library.opcheck(torch.ops.fmmt.eval_accumulate.default, (logits, labels, acc1, keep, 0), test_utils=tests)
    torch.library.opcheck(torch.ops.fmmt.eval_accumulate.default, (logits.bfloat16(), labels, acc1, None, 0), test_utils=tests)
