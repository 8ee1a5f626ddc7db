"""The V-only training step (train_step.UnimodalStep / GraphedUnimodalStep over models.meld_utt_transformer.forward_loss) against the reference.

Pinned to the reference's own numbers: forward_loss's logits in eval() mode reach the golden logits of tests/golden/multimodal.npz (`meld_utt`) and lv320.npz
(`meld_utt_320`) at the tolerances tests/test_gpu_crossmodal.py holds `forward` to (fp32 1e-3; the bf16 model within 5e-2 of the fp32 result's scale).
Against the fp64 step of tests/support_unimodal_oracle.py (assembled from oracle/ alone, validated by finite differences in tests/test_unimodal_oracle_cpu.py):
fp32, dropout 0, B = 4, L = 160, two layers -- one micro-step's loss and every gradient (1e-3 of the tensor's scale and relative L2 <= 1e-3; a gradient that is
identically zero -- the key bias of a softmax attention, the pooling's value bias -- is held to 1e-3 of its siblings' scale, as tests/test_gpu_step_oracle.py
explains), the total norms and the parameters after three clipped SGD steps with accumulation windows of 1 and 2, eager and graphed, at that file's bars (loss 2e-4,
norm 1e-4, parameters 1e-4 of max(1, max|p|)); the clip is set between the smallest and the largest norm of the unclipped reference run, so it binds in one step and
not in another (asserted on the reference).  bf16: the rules of test_one_step_every_gradient_bf16, stock bf16 autocast of the oracle's graph beside it."""

import pytest
import torch

from facialmmt_amd import synth
from tests import support_unimodal_oracle as UO
from tests import test_gpu_step_oracle as TS

pytestmark = pytest.mark.gpu

B, L = 4, 160
LR = 0.05
LENGTHS = (L, 117, 64, 1)                                     # a fully valid row ... a row with exactly one valid token


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def norms(monkeypatch):
    """the return values of clip_grad_norm_ as the steps call it (a captured step: the tensor of the captured call, re-read after a replay)"""
    seen = []
    inner = torch.nn.utils.clip_grad_norm_

    def wrapped(*a, **kw):
        seen.append(inner(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", wrapped)
    return seen


def build(dev, accumulation=1, dtype=torch.float32, dropout=0.0, seed=201):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    cfg = default_args(get_vision_utt_max_lens=L, trg_accumulation_steps=accumulation, hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout,
                       compute_dtype=dtype)
    assert cfg.vision_utt_Transformernum == 2
    model = models.meld_utt_transformer(cfg)
    synth.fill_state_dict(model, seed=seed)
    return cfg, model.to(dev).train()


def micro_batch(dev, i, n=B):
    x = synth.tensor("vfeat_step", (n, L, 512), seed=300 + i)
    mask = torch.zeros(n, L)
    for r in range(n):
        mask[r, :LENGTHS[(r + i) % len(LENGTHS)]] = 1
    labels = torch.from_numpy(synth.randint("labels_step", (n,), 0, 7, seed=400 + i))
    return x.to(dev), mask.to(dev), labels.to(dev)


def to_ref(batch):
    x, m, l = batch
    return x.double().cpu(), m.double().cpu(), l.cpu()


# ------------------------------------------------------------------------------------------------ pinned to the reference's goldens
@pytest.mark.parametrize("Lg,name,file,cut", [(20, "meld_utt", "multimodal", 14), (320, "meld_utt_320", "lv320", 250)])
def test_forward_loss_logits_reach_the_reference_goldens(golden, dev, Lg, name, file, cut):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    x = synth.tensor("vfeat" if Lg == 20 else "vfeat320", (2, Lg, 512), seed=12).to(dev)
    vmask = torch.ones(2, Lg, device=dev)
    vmask[1, cut:] = 0
    labels = torch.tensor([2, 5], device=dev)
    m = models.meld_utt_transformer(default_args(get_vision_utt_max_lens=Lg)).eval()
    synth.fill_state_dict(m, seed=201)
    m.to(dev)
    with torch.no_grad():
        loss, out = m.forward_loss(x, vmask, labels)
        fwd = m(x, vmask)
    golden.check(file, name, out, atol=1e-3, rtol=1e-3)
    want = torch.nn.functional.cross_entropy(fwd.double(), labels)
    assert abs(float(loss) - float(want)) <= 1e-3 * max(1.0, abs(float(want)))
    m16 = models.meld_utt_transformer(default_args(get_vision_utt_max_lens=Lg, compute_dtype=torch.bfloat16)).eval()
    synth.fill_state_dict(m16, seed=201)
    m16.to(dev)
    with torch.no_grad():
        out16 = m16.forward_loss(x, vmask, labels)[1]
    assert out16.dtype == torch.float32
    assert (out16 - out).abs().max().item() <= 5e-2 * max(1.0, out.abs().max().item())
    with pytest.raises(ValueError):
        m.forward_loss(x[:, :1], vmask[:, :1], labels)


def test_state_dict_and_forward_are_untouched(dev):
    """forward_loss is an addition: the module's keys are the reference's, and `forward` still gives the logits forward_loss reports"""
    cfg, model = build(dev)
    from facialmmt_amd import models
    assert list(model.state_dict()) == list(models.meld_utt_transformer(cfg).state_dict())
    x, m, l = micro_batch(dev, 0)
    model.eval()
    with torch.no_grad():
        a, b = model(x, m), model.forward_loss(x, m, l)[1]
    assert (a - b).abs().max().item() <= 1e-3 * max(1.0, a.abs().max().item())


# ------------------------------------------------------------------------------------------------ fp32 against the fp64 step
def test_one_micro_step_every_gradient_fp32(dev):
    from facialmmt_amd.train_step import UnimodalStep
    cfg, model = build(dev, accumulation=2)                   # the first micro-step of a window of two: .grad survives
    sd = UO.leaves(model, torch.float64)
    batch = micro_batch(dev, 0)
    ref = UO.run(sd, cfg, [to_ref(batch)], lr=LR)
    step = UnimodalStep(model, torch.optim.SGD(model.parameters(), lr=LR), None, cfg)
    loss = float(step(batch))
    torch.cuda.synchronize()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    print(f"loss {loss:.9f} reference {ref['micro'][0]['loss']:.9f}")
    assert abs(loss - ref["micro"][0]["loss"]) <= 1e-3 * max(1.0, abs(ref["micro"][0]["loss"]))
    assert not ref["micro"][0]["unused"]
    TS.compare_fp32_gradients(grads, ref["pending_grads"], "unimodal micro-step")
    got_norm = float(UO.total_norm([g for g in grads.values()]))
    want_norm = float(UO.total_norm(list(ref["pending_grads"].values())))
    print(f"total norm {got_norm:.9f} reference {want_norm:.9f}")
    assert abs(got_norm - want_norm) <= 1e-4 * want_norm


def reference_trajectory(model, cfg, batches):
    """the reference run twice: unclipped to see the norms, then with the clip between the smallest and the largest of them"""
    ref_batches = [to_ref(b) for b in batches]
    cfg.clip = 1e9
    free = UO.run(UO.leaves(model, torch.float64), cfg, ref_batches, lr=LR)
    ns = [s["norm"] for s in free["steps"]]
    cfg.clip = float((min(ns) * max(ns)) ** 0.5)
    sd = UO.leaves(model, torch.float64)
    ref = UO.run(sd, cfg, ref_batches, lr=LR)
    ns = [s["norm"] for s in ref["steps"]]
    assert max(ns) > cfg.clip > min(ns), (ns, cfg.clip)
    return ref, sd


def compare_trajectory(label, ref, sd, losses, got_norms, model, clip):
    print(f"{label} losses {losses} reference {[m['loss'] for m in ref['micro']]}")
    print(f"{label} total norms {got_norms} reference {[s['norm'] for s in ref['steps']]} clip {clip:.6f}")
    for l, m in zip(losses, ref["micro"]):
        assert abs(l - m["loss"]) <= 2e-4 * max(1.0, abs(m["loss"])), label
    assert len(got_norms) == len(ref["steps"]) == 3
    for n, s in zip(got_norms, ref["steps"]):
        assert abs(n - s["norm"]) <= 1e-4 * s["norm"], label
    worst, bad = (0.0, None), []
    for k, p in model.named_parameters():
        r = sd[k].detach()
        err = float((p.detach().cpu().double() - r).abs().max()) / max(1.0, float(r.abs().max()))
        worst = max(worst, (err, k))
        if not err <= 1e-4:
            bad.append((k, err))
    print(f"{label} parameters after the last step: worst {worst}")
    assert not bad, (label, bad[:10])


@pytest.mark.parametrize("accumulation", [1, 2])
@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_trajectory_fp32(dev, norms, graphed, accumulation):
    from facialmmt_amd.train_step import GraphedUnimodalStep, UnimodalStep
    cfg, model = build(dev, accumulation=accumulation)
    n_micro = 3 * accumulation
    batches = [micro_batch(dev, 10 + i) for i in range(n_micro)]
    ref, sd = reference_trajectory(model, cfg, batches)
    opt = torch.optim.SGD(model.parameters(), lr=LR)
    if graphed:
        step = GraphedUnimodalStep(model, opt, None, cfg, batches[0])
        assert step.fused is None and norms                  # SGD: graph B holds clip_grad_norm_ itself
        captured = norms[-1]
    else:
        step = UnimodalStep(model, opt, None, cfg)
    del norms[:]
    losses, got = [], []
    for i, b in enumerate(batches):
        losses.append(float(step(b)))
        if graphed and (i + 1) % accumulation == 0:
            got.append(float(captured))
    torch.cuda.synchronize()
    if not graphed:
        got = [float(n) for n in norms]
    compare_trajectory(f"{'graphed' if graphed else 'eager'} x{accumulation}", ref, sd, losses, got, model, cfg.clip)


# ------------------------------------------------------------------------------------------------ consistency of the graphed step
def _graphed_run(dev, n_steps, with_eval=False, dropout=0.1, accumulation=1):
    from facialmmt_amd.eval_step import UnimodalEvalStep
    from facialmmt_amd.train_step import GraphedUnimodalStep, HFAdamW
    cfg, model = build(dev, accumulation=accumulation, dtype=torch.bfloat16, dropout=dropout)
    torch.manual_seed(99)
    lr = torch.tensor(1e-4, device=dev)
    opt = HFAdamW(model.parameters(), lr=lr, weight_decay=0.01)
    batches = [micro_batch(dev, 20 + i) for i in range(n_steps)]
    step = GraphedUnimodalStep(model, opt, None, cfg, batches[0], autocast_dtype=torch.bfloat16)
    assert step.fused is not None and step.handover is not None
    ev = UnimodalEvalStep(model, cfg)
    losses = []
    for i, b in enumerate(batches):
        losses.append(step(b).clone())
        if with_eval and i == 0:
            logits = ev(micro_batch(dev, 77))
            assert torch.isfinite(logits).all() and model.training
    torch.cuda.synchronize()
    return step, model, torch.stack(losses), {k: p.detach().clone() for k, p in model.named_parameters()}


def test_graphed_step_is_bit_identical_over_two_constructions_and_with_an_evaluation_in_between(dev):
    """default dropout (0.1), bf16, fused AdamW: three replays -- the same bits from a second construction under the same generator seed, and from a run
    with a UnimodalEvalStep batch between the replays (evaluation draws nothing and leaves the training state alone)"""
    _, _, l1, p1 = _graphed_run(dev, 3)
    _, _, l2, p2 = _graphed_run(dev, 3)
    _, _, l3, p3 = _graphed_run(dev, 3, with_eval=True)
    print(f"losses {l1.tolist()}")
    assert torch.isfinite(l1).all()
    assert torch.equal(l1, l2) and torch.equal(l1, l3)
    start = build(dev, dtype=torch.bfloat16)[1]
    moved = 0
    for k, q in start.named_parameters():
        assert torch.equal(p1[k], p2[k]) and torch.equal(p1[k], p3[k]), k
        moved += int(not torch.equal(p1[k], q.detach()))
    assert moved > 0.9 * len(p1)


def test_graphed_step_draws_fresh_masks_and_rejects_another_shape(dev, monkeypatch):
    """the same batch replayed with a zero learning rate and ONLY the head's dropout on (the encoder's probabilities are 0): nothing but the head's keep mask
    can change the loss, so three different losses show that graph A reads a freshly drawn device seed on every replay; the keep masks themselves, copied out
    of the captured forward's buffer after each replay, differ as well.  Then the default configuration (every dropout at 0.1): three finite, different losses."""
    from facialmmt_amd import ops
    from facialmmt_amd.train_step import GraphedUnimodalStep, UnimodalStep
    cfg, model = build(dev, dtype=torch.bfloat16, dropout=0.0)
    model.mm_dropout.p = 0.1
    assert all(m.p == 0.0 for n, m in model.named_modules() if isinstance(m, torch.nn.Dropout) and n != "mm_dropout")
    seen = []
    inner = ops.pool_head_fwd_raw

    def spy(*a, **kw):
        out = inner(*a, **kw)
        seen.append(out[4])                                  # the keep mask: under capture, the buffer every replay rewrites
        return out
    monkeypatch.setattr(ops, "pool_head_fwd_raw", spy)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    batch = micro_batch(dev, 30)
    step = GraphedUnimodalStep(model, opt, None, cfg, batch)
    captured = seen[-1]
    losses, keeps = [], []
    for _ in range(3):
        losses.append(float(step(batch)))
        keeps.append(captured.clone())
    print(f"head dropout only, lr 0: losses of three replays of one batch {losses}; kept shares {[float((k != 0).float().mean()) for k in keeps]}")
    assert all(l == l and abs(l) < 1e4 for l in losses) and len(set(losses)) == 3
    assert not torch.equal(keeps[0], keeps[1]) and not torch.equal(keeps[1], keeps[2]) and not torch.equal(keeps[0], keeps[2])
    assert all(set(k.unique().tolist()) == {0.0, float(k.max())} for k in keeps)
    short = micro_batch(dev, 31, n=B - 1)
    with pytest.raises(ValueError):
        step(short)
    assert float(UnimodalStep(model, opt, None, cfg)(short)) > 0          # the caller's route for a short last batch
    assert isinstance(step.logits, torch.Tensor) and step.logits.shape == (B, 7)
    cfg2, model2 = build(dev, dtype=torch.bfloat16, dropout=0.1)          # the default: every dropout at 0.1
    step2 = GraphedUnimodalStep(model2, torch.optim.SGD(model2.parameters(), lr=0.0), None, cfg2, batch)
    losses2 = [float(step2(batch)) for _ in range(3)]
    print(f"default dropout 0.1, lr 0: {losses2}")
    assert all(l == l and abs(l) < 1e4 for l in losses2) and len(set(losses2)) == 3


# ------------------------------------------------------------------------------------------------ bf16 against the fp64 step
def stock_bf16_grads(dev, cfg, sd64, batch):
    """the oracle's own functional graph on the GPU under bf16 autocast: what stock PyTorch-ROCm gives for the same micro-step"""
    sd = TS.to_device_leaves(sd64, dev)
    lv = UO.trainable(sd)
    with torch.device(dev), torch.autocast("cuda", dtype=torch.bfloat16):
        loss = UO.step_loss(sd, cfg, *batch)
    return float(loss), dict(zip(lv, torch.autograd.grad(loss.float(), list(lv.values()), allow_unused=True)))


def test_one_micro_step_every_gradient_bf16(dev):
    """compute_dtype bf16, one micro-step: cosine >= 0.99 and relative L2 <= 0.10 for every gradient against the fp64 step; a tensor where STOCK bf16 misses that bar
    is held to 1.2 x stock's relative L2, and at most 5 % of the tensors may take that exit (that the cap can hold for these inputs is asserted on stock and the
    reference alone first).  The table goes to profiles/unimodal_step_grad_stats_bf16.txt (FMMT_STATS_DIR)."""
    from facialmmt_amd.train_step import UnimodalStep
    cfg, model = build(dev, accumulation=2, dtype=torch.bfloat16)
    sd = UO.leaves(model, torch.float64)
    batch = micro_batch(dev, 0)
    s_loss, stock = stock_bf16_grads(dev, cfg, sd, batch)
    ref = UO.run(sd, cfg, [to_ref(batch)], lr=LR)
    step = UnimodalStep(model, torch.optim.SGD(model.parameters(), lr=LR), None, cfg)
    loss = float(step(batch))
    torch.cuda.synchronize()
    ours = {k: p.grad for k, p in model.named_parameters()}
    want = ref["micro"][0]["loss"]
    print(f"bf16 loss ours {loss:.6f} stock {s_loss:.6f} reference {want:.6f}")
    table = TS.bf16_table(ours, stock, ref["pending_grads"])
    TS.write_table("unimodal_step_grad_stats_bf16.txt", f"# V-only step, B {B}, L {L} (ragged {LENGTHS}), two layers, dropout 0: cosine / relative L2 of every gradient against "
                   "the fp64 step reference -- ours | stock bf16 autocast", [f"{o[0]:.5f} {o[1]:.5f} | {s[0]:.5f} {s[1]:.5f} {k}" for k, (o, s) in table.items()])
    stock_misses = [k for k, (o, s) in table.items() if not (s[0] >= TS.COS_MIN and s[1] <= TS.REL_MAX)]
    print(f"stock misses the bar on {len(stock_misses)} of {len(table)} tensors: {stock_misses}")
    assert len(stock_misses) <= TS.EXIT_SHARE * len(table), stock_misses            # the inputs leave the exit cap room (reference and stock alone)
    assert abs(loss - want) <= 3e-2 * max(1.0, abs(want))
    print(f"ours worst cosine {min((o[0], k) for k, (o, s) in table.items())}, worst relative L2 {max((o[1], k) for k, (o, s) in table.items())}; "
          f"stock worst cosine {min((s[0], k) for k, (o, s) in table.items())}, worst relative L2 {max((s[1], k) for k, (o, s) in table.items())}")
    exits, bad = [], []
    for k, (o, s) in table.items():
        if o[0] >= TS.COS_MIN and o[1] <= TS.REL_MAX:
            continue
        if not (s[0] >= TS.COS_MIN and s[1] <= TS.REL_MAX) and o[1] <= TS.STOCK_MARGIN * s[1]:
            exits.append((k, o, s))
        else:
            bad.append((k, o, s))
    print(f"{len(exits)} of {len(table)} tensors judged against 1.2 x stock's relative L2: {exits}")
    assert not bad, bad[:10]
    assert len(exits) <= TS.EXIT_SHARE * len(table), exits
    assert len(table) >= 40
    assert all(g is not None and torch.isfinite(g).all() for g in ours.values())
