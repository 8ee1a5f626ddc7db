"""Target-task training step on RAGGED batches UNDER A GRADIENT EXCHANGE, one captured capacity against three, and the price of one replica digest.
One process: RCCL (backend nccl) at world size 1 with GradientAverager(always=True) -- every bucket goes through dist.all_reduce between the two
forward/backward graphs, the route of tests/test_gpu_ddp.py::test_rccl_world_size_one_runs_the_exchange_path -- so the per-capacity PAIRS of graphs
(A1_c, A2_c) are what is replayed.  Geometry and the eight frame-count patterns are tools/bench_ragged_buckets.py's (bench.py's headline geometry:
bf16, 4 utterances, Lv = 160, uint8 112x112 crops, RoBERTa-large, HF AdamW, accumulation 1; 358 / 454 / 483 / 516 / 384 / 411 / 403 / 425 real frames
of 640 slots), bf16 on the wire as bench.py's default.  Two legs alternate `--rounds` times:
  (a) GraphedTargetStep(frame_capacity=640, averager=...);
  (b) GraphedTargetStep(frame_capacity=(384, 512, 640), averager=...).
Prints one JSON line: ms per step of both legs (the median round, every round beside it), `capture_reserved_bytes` per capacity, the bucket histogram of
(b), and the time of one step.replica_digest() (two launches over 435 M parameters and their moments; median of `--digests` calls between device
synchronisations, and the six words of the two legs, whose parameters have seen the same batches).  Reported figures: nothing here is a bar.

    python tools/bench_rank_buckets.py [--steps 16] [--warmup 3] [--rounds 3] [--digests 5] [--time-limit 900]"""
import argparse
import faulthandler
import json
import os
import socket
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import bench_ragged_buckets as RB  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16, help="timed steps per round and leg")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps per leg (at least one per frame-count pattern is run)")
    ap.add_argument("--rounds", type=int, default=3, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--digests", type=int, default=5, help="timed replica_digest() calls; the median is reported")
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the process ends itself")
    return ap.parse_args()


def make_leg(frame_capacity, bench, bargs, dev, sample):
    """bench_ragged_buckets.make_leg under an exchange that is always issued"""
    import bench_ragged
    from facialmmt_amd.config import default_args
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, step_parameters
    cfg = default_args(get_vision_utt_max_lens=bench_ragged.LV, trg_accumulation_steps=1)
    swin, mm = bench.build_models(bargs, dev, cfg)
    masters = MasterWeights(mm.roberta, torch.bfloat16)
    params = step_parameters(mm, masters)
    flat = GradientAverager(params, hooks=False, comm_dtype=torch.bfloat16, always=True)
    assert flat.active
    opt = HFAdamW(params, lr=torch.tensor(cfg.trg_lr, device=dev), weight_decay=cfg.weight_decay)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(1.0, (s + 1) / 100.0))
    step = GraphedTargetStep(swin, mm, opt, sched, cfg, sample, autocast_dtype=torch.bfloat16, averager=flat, masters=masters, frame_capacity=frame_capacity)
    assert step.split
    return step


def main():
    a = parse()
    faulthandler.dump_traceback_later(a.time_limit, exit=True)
    assert torch.cuda.is_available(), "bench_rank_buckets.py needs an MI355X"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    bench, bargs, dev, padded, counts = RB.setup()
    legs = {name: make_leg(cap, bench, bargs, dev, padded[0]) for name, cap in RB.LEGS.items()}
    for step in legs.values():
        RB.timed(step, padded, max(a.warmup, len(padded)))       # every graph the timed window replays has run
    for step in legs.values():
        step.replays = {c: 0 for c in step.capacities}
    rounds = []
    for r in range(a.rounds):                                    # alternate: clock and thermal drift reach both legs alike
        rounds.append([RB.timed(legs[name], padded, a.steps, start=r * a.steps) for name in ("single", "buckets")])
    med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(2)]
    step = legs["buckets"]
    step.replica_digest()                                        # the first call allocates the per-block scratch
    digest_ms = []
    for _ in range(a.digests):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        words = step.replica_digest()
        torch.cuda.synchronize()
        digest_ms.append((time.perf_counter() - t0) * 1e3)
    other = legs["single"].replica_digest()
    print(json.dumps({
        "metric": "rank_buckets_target_step_ms",
        "config": f"bf16, {bargs.utts} utterances, Lv = {bargs.frames}, uint8 112x112 crops, roberta-large, HF AdamW, accumulation 1; RCCL world size 1, "
                  f"GradientAverager(always=True, bf16 wire), {len(step.flat.buckets)} buckets; frame totals {[sum(n) for n in counts]} cycled, num_imgs as lists",
        "steps_per_round": a.steps, "rounds_ms": [[round(x, 3) for x in r] for r in rounds],
        "legs": [f"GraphedTargetStep(frame_capacity={RB.BUCKETS[-1]}, averager)", f"GraphedTargetStep(frame_capacity={RB.BUCKETS}, averager)"],
        "single_ms": round(med[0], 3), "buckets_ms": round(med[1], 3), "buckets_over_single": round(med[1] / med[0], 4),
        "bucket_histogram": {str(c): step.replays[c] for c in RB.BUCKETS},
        "capture_reserved_bytes": {name: {str(c): int(v) for c, v in leg.capture_reserved_bytes.items()} for name, leg in legs.items()},
        "replica_digest_ms": round(sorted(digest_ms)[len(digest_ms) // 2], 3), "replica_digest_all_ms": [round(x, 3) for x in digest_ms],
        "digest_blocks": step.fused.blocks, "digest_tensors": step.fused.n,
        "digest_words": {"buckets": [f"{int(w) & 0xFFFFFFFFFFFFFFFF:#018x}" for w in words.tolist()],
                         "single": [f"{int(w) & 0xFFFFFFFFFFFFFFFF:#018x}" for w in other.tolist()]},
        "device": torch.cuda.get_device_name(0)}))
    faulthandler.cancel_dump_traceback_later()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
