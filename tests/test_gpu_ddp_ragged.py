"""Ragged MELD batches on SEVERAL RANKS: two processes sharing the one GPU of the test box on gloo (RCCL refuses two ranks per device; the RCCL
variants need two GPUs), the construction of tests/test_gpu_ddp.py -- mp.spawn, results through files.  Three spawns, several scenarios per worker:

  1  GraphedTargetStep(frame_capacity=(8, 12), pad_rows=True) under GradientAverager: the ranks replay DIFFERENT capacities in the same step, then hold
     different numbers of real rows (global_rows), with accumulation 1 and 2; against a single-process reference that runs each rank's compact batch
     through the eager formulation one after the other (never concatenated: BatchNorm stays per replica), weights each loss by rows_r / sum(rows),
     divides by the accumulation and does clip + SGD.  Bound: 2e-4 * max(1, |w|), that of tests/test_gpu_ddp.py's two-rank tests.
  2  the fused AdamW update with skip_nonfinite=True: a NaN on ONE rank makes BOTH ranks skip (the norm is taken of the reduced buffers), the replica
     digest and parallel.replicas_agree see the ranks agree, and see it when one rank is nudged.  fp32 and bf16 on the wire.
  3  the weight word in GraphedUnimodalStep and GraphedAuxStep, B = 4, rows (3, 1), against the single-process weighted reference at the bars of
     tests/test_gpu_short_batch.py (losses 2e-4, parameters 1e-4 of scale); with global_rows=None and full batches the parameters are torch.equal to
     those of the same step built without pad_rows.

T+A+V shapes are those of tests/test_gpu_ragged_buckets.py, restated and not imported: B = 2, Lv = 6, buckets (8, 12), fp32 compute, tau = 1e5, threshold
0.1, DropPath and dropout off, stand-in text encoder, every padded frame slot random.  Every process group gets a 120 s timeout: a rank that falls out of
step ends as a failed test, not as a hang.  Every comparison prints its figures before it asserts (run with -s)."""
import os
import socket
import types
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from facialmmt_amd import synth

pytestmark = pytest.mark.gpu

B, LV, BUCKETS = 2, 6, (8, 12)
NUMS = (([3, 4], [6, 5], [2, 6], [6, 6], [3, 4], [6, 5]),        # rank 0: four full steps, then the loader batches the two padded calls are cut from
        ([6, 6], [3, 4], [6, 5], [3, 4], [6, 5], [2, 6]))        # rank 1
ROWS = ((2, 2), (2, 2), (2, 2), (2, 2), (2, 1), (1, 1))           # real rows (rank 0, rank 1) per call
GLOBAL = (None, None, None, None, 3, None)                        # what the call is told
RCCL = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one device per rank: two GPUs")
BACKENDS = ["gloo", pytest.param("nccl", marks=RCCL)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port, backend):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=timedelta(seconds=120), **({"device_id": dev} if backend == "nccl" else {}))
    return dev


def _models(dev, accumulation):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    cfg = default_args(get_vision_utt_max_lens=LV, get_audio_utt_max_lens=24, trg_accumulation_steps=accumulation, plm_module=synth.make_standin_plm(),
                       hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, crossmodal_attn_dropout_TA=0.0, crossmodal_attn_dropout_TA_V=0.0,
                       tau=1e5, FacialEmoImpor_threshold=0.1)
    cfg.compute_dtype = torch.float32
    swin = models.SwinForAffwildClassification(cfg)
    mm = models.MultiModalTransformerForClassification(cfg)
    synth.fill_state_dict(swin, seed=100)
    synth.fill_state_dict(mm, seed=200)
    for m in swin.modules():
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    swin.to(dev).train()
    mm.to(dev).train()
    return cfg, swin, mm


def _batch(dev, cfg, num_imgs, seed):
    """the loader's batch for the given frame counts: frames (B, Lv, 3, 224, 224) with EVERY slot random, num_imgs as the reference's collate yields it"""
    import bench
    args = types.SimpleNamespace(utts=B, frames=LV, dtype="fp32", plm="roberta-large", input="float", resize="pil")
    batch = list(bench.synth_batch(args, dev, seed, cfg))
    batch[0] = batch[0] % 1000
    vmask = torch.zeros(B, LV, device=dev)
    for u, k in enumerate(num_imgs):
        vmask[u, :k] = 1
    batch[6] = vmask
    batch[8], batch[9] = batch[8].view(B, LV, 3, 224, 224), list(num_imgs)
    return tuple(batch)


def _short(batch, b):
    """the loader's batch cut to its first b utterances"""
    return tuple(t[:b] for t in batch)


def _compact(batch):
    """what the eager formulation takes: the real frames concatenated, num_imgs on the device"""
    out = list(batch)
    out[8] = torch.cat([batch[8][u, :k] for u, k in enumerate(batch[9])], dim=0).contiguous()
    out[9] = torch.tensor(batch[9], device=batch[8].device)
    return tuple(out)


def _fed(dev, cfg, accumulation, rank, i):
    return _short(_batch(dev, cfg, NUMS[rank][i], 100 * accumulation + 10 * rank + i), ROWS[i][rank])


def _worst(a, b, bar):
    worst = (0.0, None)
    for k in a:
        err = float((a[k].double() - b[k].double()).abs().max()) / max(1.0, float(a[k].abs().max()))
        worst = (err, k) if worst[1] is None or err > worst[0] else worst
    print(f"  worst {worst} (bar {bar:.0e})")
    return worst


# ------------------------------------------------------------------------------------------------ spawn 1: capacities and rows differ between the ranks
def _worker_sgd(rank, world, port, out_dir, backend):
    dev = _init(rank, world, port, backend)
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep
    for accumulation in (1, 2):
        cfg, swin, mm = _models(dev, accumulation)
        params = [p for p in mm.parameters() if p.requires_grad]
        avg = GradientAverager(params, hooks=False, bucket_mb=1)
        step = GraphedTargetStep(swin, mm, torch.optim.SGD(params, lr=0.05), None, cfg, _fed(dev, cfg, accumulation, rank, 0), autocast_dtype=None,
                                 frame_capacity=BUCKETS, pad_rows=True, averager=avg)
        info = dict(split=step.split, buckets=len(avg.buckets), losses=[], caps=[], counts=[], rows=[], raised=None)
        for i in range(len(ROWS)):
            batch = _fed(dev, cfg, accumulation, rank, i)
            if i == 4:                                       # rows (2, 1) can never be 5 rows of 2 ranks with B = 2: refused before anything is launched
                before = (step.i_batch, dict(step.replays), step.static[9].clone(), step.padded_calls)
                try:
                    step(batch, global_rows=5)
                except ValueError as e:
                    info["raised"] = str(e)
                info["untouched"] = (step.i_batch, dict(step.replays), step.padded_calls) == (before[0], before[1], before[3]) and \
                    torch.equal(step.static[9], before[2])
            loss, _ = step(batch, global_rows=GLOBAL[i])
            info["losses"].append(float(loss))
            info["caps"].append(step.capacity)
            info["counts"].append(step.frame_counts.tolist())
            info["rows"].append((step.rows, step.padded_calls))
            if i == 3:
                info["replays4"] = dict(step.replays)
        torch.cuda.synchronize()
        info["params"] = {k: v.detach().cpu() for k, v in mm.named_parameters()}
        torch.save(info, os.path.join(out_dir, f"sgd_acc{accumulation}_rank{rank}.pt"))
    dist.destroy_process_group()


def _reference_sgd(dev, accumulation):
    import torch.nn.functional as F
    from facialmmt_amd.train_step import select_frames
    cfg, swin, mm = _models(dev, accumulation)
    params = [p for p in mm.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.05)
    losses = ([], [])
    for i, rows in enumerate(ROWS):
        for r in range(2):
            ids, am, sep, audio, amask, vis, vmask, labels, frames, num, utt = _compact(_fed(dev, cfg, accumulation, r, i))
            preds = swin(frames, is_trg_task=True)
            vc, nm = select_frames(preds.float(), vis, vmask, num, cfg.FacialEmoImpor_threshold)
            loss = F.cross_entropy(mm(ids, am, sep, audio, amask, vc, nm, utt).float(), labels) / accumulation
            losses[r].append(float(loss.detach()))
            (loss * (rows[r] / sum(rows))).backward()
            swin.zero_grad(set_to_none=True)
        if (i + 1) % accumulation == 0:
            torch.nn.utils.clip_grad_norm_(params, cfg.clip)
            opt.step()
            opt.zero_grad(set_to_none=True)
    return losses, {k: v.detach().cpu() for k, v in mm.named_parameters()}


@pytest.fixture(scope="module", params=BACKENDS)
def sgd_runs(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ddp_ragged_sgd"))
    mp.spawn(_worker_sgd, args=(2, _free_port(), d, request.param), nprocs=2, join=True)
    return {(a, r): torch.load(os.path.join(d, f"sgd_acc{a}_rank{r}.pt"), weights_only=False) for a in (1, 2) for r in range(2)}


@pytest.mark.parametrize("accumulation", [1, 2])
def test_ranks_replay_different_capacities_and_hold_different_rows(sgd_runs, accumulation):
    dev = torch.device("cuda:0")
    got = [sgd_runs[(accumulation, r)] for r in range(2)]
    for r in range(2):
        assert got[r]["split"] and got[r]["buckets"] >= 2
        assert got[r]["caps"][:4] == ([8, 12, 8, 12], [12, 8, 12, 8])[r] and got[r]["replays4"] == {8: 2, 12: 2}
        assert got[r]["caps"][4:] == [8, 8]                                                    # the padded calls: the bucket of the REAL frames
        assert got[r]["counts"] == [[sum(NUMS[r][i][:ROWS[i][r]])] * 2 for i in range(6)]
        assert got[r]["rows"] == ([(2, 0)] * 5 + [(1, 1)], [(2, 0)] * 4 + [(1, 1), (1, 2)])[r]
        assert got[r]["raised"] is not None and "global_rows" in got[r]["raised"] and got[r]["untouched"]
    for k, w in got[0]["params"].items():
        assert torch.equal(w, got[1]["params"][k]), k                                           # the replicas hold the same bits
    losses, want = _reference_sgd(dev, accumulation)
    for r in range(2):
        print(f"accumulation {accumulation}, rank {r}: losses reference", losses[r])
        print(f"accumulation {accumulation}, rank {r}: losses graphed  ", got[r]["losses"])
    worst = _worst(want, got[0]["params"], 2e-4)
    for r in range(2):
        for a, b in zip(losses[r], got[r]["losses"]):                                          # the loss handed back is the rank's own, unweighted
            assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (r, losses[r], got[r]["losses"])
    assert worst[0] <= 2e-4, worst
    init = {k: p.detach().cpu() for k, p in _models(dev, accumulation)[2].named_parameters()}
    assert sum(int((got[0]["params"][k] - v).abs().max() > 0) for k, v in init.items()) > 50   # the optimiser really stepped


# ------------------------------------------------------------------------------------------------ spawn 2: one rank's NaN, both ranks skip; the digest
def _worker_guard(rank, world, port, out_dir, backend):
    dev = _init(rank, world, port, backend)
    from facialmmt_amd.parallel import GradientAverager, replicas_agree
    from facialmmt_amd.train_step import GraphedTargetStep
    out = {}
    for name, comm in (("fp32", None), ("bf16", torch.bfloat16)):
        cfg, swin, mm = _models(dev, 1)
        params = [p for p in mm.parameters() if p.requires_grad]
        opt = torch.optim.AdamW(params, lr=torch.tensor(1e-3, device=dev), fused=True, capturable=True, weight_decay=0.01, eps=1e-6)
        avg = GradientAverager(params, hooks=False, bucket_mb=1, comm_dtype=comm)
        batches = [_batch(dev, cfg, NUMS[rank][i], 500 + 10 * rank + i) for i in range(3)]
        if rank == 1:
            batches[1][3][0, 0, 0] = float("nan")                                              # one NaN in rank 1's audio, step 2
        step = GraphedTargetStep(swin, mm, opt, None, cfg, batches[0], autocast_dtype=None, frame_capacity=BUCKETS, averager=avg, skip_nonfinite=True)
        info = dict(fused=step.fused is not None, caps=[])
        start = [p.detach().clone() for p in params]
        step(batches[0])
        info["caps"].append(step.capacity)
        after1, d1 = [p.detach().clone() for p in params], step.replica_digest().cpu()
        info["moved1"] = sum(int(not torch.equal(a, b)) for a, b in zip(start, after1))
        info["agree1"] = len(replicas_agree(step.replica_digest())) == world
        step(batches[1])
        info["caps"].append(step.capacity)
        torch.cuda.synchronize()
        d2 = step.replica_digest().cpu()
        info["same_bits2"] = all(torch.equal(a, p.detach()) for a, p in zip(after1, params))
        info["same_digest2"] = torch.equal(d1, d2)
        info["agree2"] = len(replicas_agree(step.replica_digest())) == world
        r = step.monitor.read()
        info["read2"] = (r.applied, r.skipped, r.nonfinite_losses, r.micro_steps)
        step(batches[2])
        info["caps"].append(step.capacity)
        d3 = step.replica_digest().cpu()
        info["moved_digest3"] = [int(a != b) for a, b in zip(d2.tolist(), d3.tolist())]
        info["agree3"] = len(replicas_agree(step.replica_digest())) == world
        r = step.monitor.read()
        info["read3"] = (r.applied, r.skipped, r.nonfinite_losses, r.micro_steps)
        info["finite3"] = all(bool(torch.isfinite(p).all()) for p in params)
        if rank == 1:
            with torch.no_grad():
                params[0].view(-1)[0] += 1e-3
        try:
            replicas_agree(step.replica_digest())
            info["nudged"] = None
        except RuntimeError as e:
            info["nudged"] = str(e)
        out[name] = info
    torch.save(out, os.path.join(out_dir, f"guard_rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_nan_on_one_rank_skips_the_update_on_both_and_the_digest_sees_the_replicas_agree(backend, tmp_path):
    mp.spawn(_worker_guard, args=(2, _free_port(), str(tmp_path), backend), nprocs=2, join=True)
    got = [torch.load(os.path.join(str(tmp_path), f"guard_rank{r}.pt"), weights_only=False) for r in range(2)]
    for name in ("fp32", "bf16"):
        for r in range(2):
            info = got[r][name]
            print(name, "rank", r, info)
            assert info["fused"] and info["moved1"] > 50 and info["agree1"]
            assert info["caps"] == ([8, 12, 8], [12, 8, 12])[r]
            assert info["same_bits2"] and info["same_digest2"] and info["agree2"]                # step 2 left every bit where step 1 put it
            assert info["read2"] == (1, 1, 1 if r == 1 else 0, 1 if r == 1 else 2)              # skipped on both; the bad loss was rank 1's alone
            assert info["read3"][:3] == (2, 1, 1 if r == 1 else 0) and info["agree3"] and info["finite3"]
            assert info["moved_digest3"] == [1] * 6                                              # parameters and both moments moved in step 3
            assert info["nudged"] is not None and "rank 1" in info["nudged"] and "parameters" in info["nudged"]


# ------------------------------------------------------------------------------------------------ spawn 3: the weight word in the other two steps
AUX_B = UNI_B = 4
ROWS3 = ((4, 4), (3, 1))                                          # call 1: full batches, global_rows=None; call 2: rows (3, 1), global_rows=4


def _aux_model(dev):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    cfg = default_args(aux_accumulation_steps=1)
    swin = models.SwinForAffwildClassification(cfg)
    synth.fill_state_dict(swin, seed=100)
    for m in swin.modules():
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    return cfg, swin.to(dev).train()


def _aux_batch(dev, rank, i, rows=AUX_B):
    import bench
    args = types.SimpleNamespace(aux_images=AUX_B, dtype="fp32", input="float")
    imgs, labels = bench.synth_aux_batch(args, torch.device("cpu"), 10 * rank + i)
    return imgs[:rows].to(dev), labels[:rows].to(dev)


def _uni_batch(dev, rank, i, rows=UNI_B):
    from tests import test_gpu_unimodal_step as US
    return tuple(t[:rows] for t in US.micro_batch(dev, 80 + 10 * rank + i))


def _worker_weight(rank, world, port, out_dir, backend):
    dev = _init(rank, world, port, backend)
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedAuxStep, GraphedUnimodalStep
    from tests import test_gpu_unimodal_step as US
    out = {}
    for pad in (True, False):
        cfg, model = US.build(dev, accumulation=1)
        params = list(model.parameters())
        step = GraphedUnimodalStep(model, torch.optim.SGD(params, lr=US.LR), None, cfg, _uni_batch(dev, rank, 0), pad_rows=pad,
                                   averager=GradientAverager(params, hooks=False, bucket_mb=1))
        info = dict(word=step.row_weight is not None, losses=[float(step(_uni_batch(dev, rank, 0)))])
        torch.cuda.synchronize()
        info["params1"] = {k: v.detach().cpu() for k, v in model.named_parameters()}
        if pad:
            info["losses"].append(float(step(_uni_batch(dev, rank, 1, ROWS3[1][rank]), global_rows=4)))
            torch.cuda.synchronize()
            info["params2"] = {k: v.detach().cpu() for k, v in model.named_parameters()}
            info["rows"] = (step.rows, step.padded_calls)
        else:
            try:
                step(_uni_batch(dev, rank, 1), global_rows=8)
                info["raised"] = None
            except ValueError as e:
                info["raised"] = str(e)
        out[("uni", pad)] = info
        cfg, swin = _aux_model(dev)
        params = [p for p in swin.parameters() if p.requires_grad]
        step = GraphedAuxStep(swin, torch.optim.SGD(params, lr=0.02), None, cfg, *_aux_batch(dev, rank, 0), pad_rows=pad,
                              averager=GradientAverager(params, hooks=False, bucket_mb=8))
        info = dict(word=step.row_weight is not None, losses=[float(step(*_aux_batch(dev, rank, 0)))])
        torch.cuda.synchronize()
        info["params1"] = {k: v.detach().cpu() for k, v in swin.named_parameters()}
        if pad:
            info["losses"].append(float(step(*_aux_batch(dev, rank, 1, ROWS3[1][rank]), global_rows=4)))
            torch.cuda.synchronize()
            info["params2"] = {k: v.detach().cpu() for k, v in swin.named_parameters()}
            info["rows"] = (step.rows, step.padded_calls)
        out[("aux", pad)] = info
    torch.save(out, os.path.join(out_dir, f"weight_rank{rank}.pt"))
    dist.destroy_process_group()


def _reference_weight(dev, kind):
    """two updates of plain SGD on sum_r (rows_r / sum rows) * (mean loss of rank r's real rows); the parameters after each, the ranks' own losses"""
    import torch.nn.functional as F
    from tests import test_gpu_unimodal_step as US
    if kind == "uni":
        cfg, model = US.build(dev, accumulation=1)
        params, lr = list(model.parameters()), US.LR
    else:
        cfg, model = _aux_model(dev)
        params, lr = [p for p in model.parameters() if p.requires_grad], 0.02
    opt = torch.optim.SGD(params, lr=lr)
    losses, states = ([], []), []
    for i, rows in enumerate(ROWS3):
        for r in range(2):
            if kind == "uni":
                loss = model.forward_loss(*_uni_batch(dev, r, i, rows[r]))[0]
            else:
                imgs, labels = _aux_batch(dev, r, i, rows[r])
                loss = model(imgs, False, labels, F.cross_entropy)
            losses[r].append(float(loss.detach()))
            (loss * (rows[r] / sum(rows))).backward()
        torch.nn.utils.clip_grad_norm_(params, cfg.clip)
        opt.step()
        opt.zero_grad(set_to_none=True)
        states.append({k: v.detach().cpu() for k, v in model.named_parameters()})
    return losses, states


@pytest.fixture(scope="module", params=BACKENDS)
def weight_runs(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ddp_ragged_weight"))
    mp.spawn(_worker_weight, args=(2, _free_port(), d, request.param), nprocs=2, join=True)
    return [torch.load(os.path.join(d, f"weight_rank{r}.pt"), weights_only=False) for r in range(2)]


@pytest.mark.parametrize("kind", ["uni", "aux"])
def test_the_weight_word_in_the_unimodal_and_auxiliary_steps(weight_runs, kind):
    dev = torch.device("cuda:0")
    pad, plain = [weight_runs[r][(kind, True)] for r in range(2)], [weight_runs[r][(kind, False)] for r in range(2)]
    for r in range(2):
        assert pad[r]["word"] and not plain[r]["word"]                                          # the word exists only with pad_rows under the exchange
        assert pad[r]["rows"] == ((3, 1), (1, 1))[r]
        for k, w in pad[r]["params1"].items():                                                  # global_rows=None on full batches: the parent's bits
            assert torch.equal(w, plain[r]["params1"][k]), (k, r)
        assert pad[r]["losses"][0] == plain[r]["losses"][0]
    if kind == "uni":
        assert all(p["raised"] is not None and "pad_rows" in p["raised"] for p in plain)        # global_rows without pad_rows: ValueError
    for which in ("params1", "params2"):
        for k, w in pad[0][which].items():
            assert torch.equal(w, pad[1][which][k]), (which, k)                                 # the replicas hold the same bits
    losses, states = _reference_weight(dev, kind)
    for r in range(2):
        print(f"{kind} rank {r}: losses reference", losses[r], "graphed", pad[r]["losses"])
    print(f"{kind}: parameters after the full step")
    w1 = _worst(states[0], pad[0]["params1"], 1e-4)
    print(f"{kind}: parameters after the step with rows (3, 1), global_rows=4")
    w2 = _worst(states[1], pad[0]["params2"], 1e-4)
    for r in range(2):
        for a, b in zip(losses[r], pad[r]["losses"]):
            assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (r, losses[r], pad[r]["losses"])
    assert w1[0] <= 1e-4 and w2[0] <= 1e-4, (w1, w2)
    moved = sum(int(not torch.equal(states[0][k], states[1][k])) for k in states[0])
    assert moved > 0.5 * len(states[0])
