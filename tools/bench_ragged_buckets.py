"""Target-task training step on RAGGED batches, one captured capacity against three: tools/bench_ragged.py's geometry (bf16, 4 utterances, Lv = 160, uint8
112x112 crops in, RoBERTa-large, HF AdamW, accumulation 1) and its eight frame-count patterns (seed 20240: 358 / 454 / 483 / 516 / 384 / 411 / 403 / 425
real frames of 640 slots), two legs in ONE process and ONE call, alternating:
  (a) train_step.GraphedTargetStep(frame_capacity=640): one capture, Swin runs forward and backward on all 640 slots whatever the batch holds;
  (b) GraphedTargetStep(frame_capacity=(384, 512, 640)): one forward/backward graph per capacity, per batch the smallest that holds it is replayed
      (by the bucket rule eight consecutive steps replay 384 twice, 512 five times, 640 once: 4032 Swin rows where (a) computes 5120).
Both legs get the batches as the loader pads them, (4, 160, 112, 112, 3), with num_imgs as a LIST (the reference's collate; a device tensor would make
(b) replay 640 every time).  Each leg owns models with the same initial values.  Inputs stay on the device; wall clock between device synchronisations,
`--rounds` alternating rounds of `--steps` steps, the median round reported with every round beside it.  Prints one JSON line: ms per step of both legs,
their ratio, whether (b) was the faster leg in every round, the bucket histogram of (b)'s timed steps, the bytes each capture added
(`capture_bytes`: torch.cuda.memory_allocated; `capture_reserved_bytes`: memory_reserved, which is what the private pool of a capture holds on to), and,
with --census, kernel launches per step of both legs (the script re-runs itself under `rocprofv3 --kernel-trace --stats`, a child process per leg and
length, as tools/bench_eval_ragged.py does; tools/count_launches.py prints the per-kernel table of such a directory).

    python tools/bench_ragged_buckets.py [--steps 16] [--warmup 3] [--rounds 3] [--census] [--time-limit 900]

--time-limit: the process ends itself (stack traces on stderr, exit status 1) when the whole run takes longer; every census child has its own limit."""
import argparse
import csv
import faulthandler
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

BUCKETS = (384, 512, 640)
LEGS = {"single": BUCKETS[-1], "buckets": BUCKETS}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16, help="timed steps per round and leg")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps per leg (at least one per frame-count pattern is run)")
    ap.add_argument("--rounds", type=int, default=3, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--census", action="store_true", help="also count kernel launches per step (four profiled child processes)")
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the process ends itself")
    ap.add_argument("--census-leg", choices=sorted(LEGS), default=None, help="internal: `--steps` steps of one leg and exit (profiled child)")
    return ap.parse_args()


def setup():
    """(bench module, its default arguments, device, the eight padded batches with num_imgs as lists, their frame counts)"""
    import bench_ragged
    from facialmmt_amd.config import default_args
    bench, bargs = bench_ragged.bench_args()
    assert (bargs.utts, bargs.frames) == (bench_ragged.UTTS, bench_ragged.LV) and bench_ragged.CAP == BUCKETS[-1]
    dev = torch.device("cuda:0")
    counts = bench_ragged.frame_counts(8, 20240)
    cfg = default_args(get_vision_utt_max_lens=bench_ragged.LV, trg_accumulation_steps=1)
    pairs = bench_ragged.make_batches(bench, bargs, dev, cfg, counts)
    padded = [p[:9] + (list(n),) + p[10:] for (p, _), n in zip(pairs, counts)]
    return bench, bargs, dev, padded, counts


def make_leg(frame_capacity, bench, bargs, dev, sample):
    """bench_ragged.make_leg's graphed leg with the given frame_capacity"""
    import bench_ragged
    from facialmmt_amd.config import default_args
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, step_parameters
    cfg = default_args(get_vision_utt_max_lens=bench_ragged.LV, trg_accumulation_steps=1)
    swin, mm = bench.build_models(bargs, dev, cfg)
    masters = MasterWeights(mm.roberta, torch.bfloat16)
    params = step_parameters(mm, masters)
    flat = GradientAverager(params, hooks=False)
    opt = HFAdamW(params, lr=torch.tensor(cfg.trg_lr, device=dev), weight_decay=cfg.weight_decay)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(1.0, (s + 1) / 100.0))
    return GraphedTargetStep(swin, mm, opt, sched, cfg, sample, autocast_dtype=torch.bfloat16, averager=flat, masters=masters, frame_capacity=frame_capacity)


def timed(step, batches, n, start=0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        step(batches[(start + i) % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def census(leg, steps, limit):
    """kernel launches per step of one leg, from rocprofv3 kernel traces of two child processes of different length: the difference is free of set-up,
    warm-up and capture launches"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    out = tempfile.mkdtemp(prefix="fmmt_ragged_buckets_census_")
    try:
        calls = []
        for n in (steps, 2 * steps):
            d = os.path.join(out, str(n))
            cmd = [prof, "--kernel-trace", "--stats", "-d", d, "-o", "r", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                   "--census-leg", leg, "--steps", str(n), "--time-limit", str(limit)]
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=limit + 60)
            if r.returncode != 0:
                raise RuntimeError(f"census child ({leg}) exited with {r.returncode}: {r.stderr[-400:]}")
            f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
            calls.append(sum(int(row["Calls"]) for row in csv.DictReader(open(f))))
        return (calls[1] - calls[0]) / steps
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    a = parse()
    faulthandler.dump_traceback_later(a.time_limit, exit=True)
    assert torch.cuda.is_available(), "bench_ragged_buckets.py needs an MI355X"
    bench, bargs, dev, padded, counts = setup()
    if a.census_leg:
        step = make_leg(LEGS[a.census_leg], bench, bargs, dev, padded[0])
        timed(step, padded, a.steps)
        return
    legs = {name: make_leg(cap, bench, bargs, dev, padded[0]) for name, cap in LEGS.items()}
    for step in legs.values():
        timed(step, padded, max(a.warmup, len(padded)))          # every graph the timed window replays has run
    for step in legs.values():
        step.replays = {c: 0 for c in step.capacities}
    rounds = []
    for r in range(a.rounds):                                    # alternate: clock and thermal drift reach both legs alike
        rounds.append([timed(legs[name], padded, a.steps, start=r * a.steps) for name in ("single", "buckets")])
    med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(2)]
    hist = dict(legs["buckets"].replays)
    mem = {name: {"capture_bytes": {str(c): int(v) for c, v in step.capture_bytes.items()},
                  "capture_reserved_bytes": {str(c): int(v) for c, v in step.capture_reserved_bytes.items()}} for name, step in legs.items()}
    last = legs["buckets"].frame_counts.tolist()
    launches = {"single": None, "buckets": None}
    if a.census:
        del legs, step
        torch.cuda.empty_cache()
        for leg in launches:
            launches[leg] = census(leg, 8, a.time_limit)
    totals = [sum(n) for n in counts]
    rows = sum(c * k for c, k in hist.items())
    print(json.dumps({
        "metric": "ragged_buckets_target_step_ms",
        "config": f"bf16, {bargs.utts} utterances, Lv = {bargs.frames}, uint8 112x112 crops, roberta-large, HF AdamW, accumulation 1; frame totals {totals} cycled, num_imgs as lists",
        "steps_per_round": a.steps, "rounds_ms": [[round(x, 3) for x in r] for r in rounds],
        "legs": [f"GraphedTargetStep(frame_capacity={BUCKETS[-1]})", f"GraphedTargetStep(frame_capacity={BUCKETS})"],
        "single_ms": round(med[0], 3), "buckets_ms": round(med[1], 3), "buckets_over_single": round(med[1] / med[0], 4),
        "buckets_faster_in_every_round": all(r[1] < r[0] for r in rounds),
        "bucket_histogram": {str(c): hist[c] for c in BUCKETS}, "swin_rows": {"single": BUCKETS[-1] * a.steps * a.rounds, "buckets": rows},
        "memory": mem, "launches_per_step": launches, "last_frame_counts": last, "device": torch.cuda.get_device_name(0)}))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
