"""Evaluation on RAGGED batches at configs[1]'s geometry (4 utterances, Lv = 160, RoBERTa-large, bf16, text encoder as the benchmark's step has it), two
legs in ONE process and ONE call, alternating:
  (a) eval_step.GraphedEvalStep WITHOUT frame_capacity, captured on a full batch and fed the batches compacted to (sum num_imgs, ...) frames: the
      compact tensor has another first dimension in every batch, so every call takes the launch-by-launch fallback -- what a split of real MELD
      data did before frame_capacity existed -- and evaluate() clones logits and labels per batch.  The compaction is outside the timed window;
  (b) GraphedEvalStep(frame_capacity=(384, 512, 640)) on the batches as the loader pads them, (4, 160, ...) + num_imgs as a list, with
      MeldMetrics(collect_rows=...): one graph replay per batch in the smallest bucket that holds it, no per-batch clone.
Frame counts: tools/bench_ragged.py's (seed 20240: totals 358 / 454 / 483 / 516 / 384 / 411 / 403 / 425 of 640 slots).  A "split" is `--batches`
batches through eval_step.evaluate(); wall clock around it, the final copy of the accumulators included; `--rounds` alternating rounds, the median
reported.  Prints one JSON line: ms per batch of both legs, the bucket histogram of leg (b), replays / fallbacks, launches per batch.

    python tools/bench_eval_ragged.py [--batches 40] [--warmup 1] [--rounds 3] [--no-census]

Launch counts: as tools/bench_eval.py, the script re-runs itself under `rocprofv3 --kernel-trace --stats` (a child process per leg)."""
import argparse
import collections
import csv
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


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40, help="batches per split (the eight frame-count patterns, cycled)")
    ap.add_argument("--warmup", type=int, default=1, help="untimed splits per leg")
    ap.add_argument("--rounds", type=int, default=3, help="the two legs alternate this many times; the median round is reported")
    ap.add_argument("--no-census", action="store_true")
    ap.add_argument("--census-leg", choices=["compact", "bucketed"], default=None, help="internal: one split of one leg and exit (profiled child)")
    return ap.parse_args()


def setup():
    import bench
    import bench_ragged
    from facialmmt_amd.config import default_args
    from facialmmt_amd.train_step import MasterWeights
    saved, sys.argv = sys.argv, [sys.argv[0]]
    args = bench.parse()                                       # configs[1] defaults
    sys.argv = saved
    args.plm = args.plm or "roberta-large"
    assert (args.utts, args.frames) == (bench_ragged.UTTS, bench_ragged.LV)
    dev = torch.device("cuda:0")
    cfg = default_args(get_vision_utt_max_lens=args.frames, trg_accumulation_steps=1)
    swin, mm = bench.build_models(args, dev, cfg)
    MasterWeights(mm.roberta, torch.bfloat16)                   # the benchmark's text encoder: bf16 parameters, fused sublayers
    counts = bench_ragged.frame_counts(8, 20240)
    pairs = bench_ragged.make_batches(bench, args, dev, cfg, counts)
    padded = [p[:9] + (n,) + p[10:] for (p, _), n in zip(pairs, counts)]      # num_imgs as the reference's collate yields it: a list
    full = bench.synth_batch(args, dev, 0, cfg)                 # leg (a)'s sample batch: every slot real
    return args, dev, cfg, swin, mm, counts, padded, [c for _, c in pairs], full


def make_legs(swin, mm, cfg, dev, padded, full, rows):
    from facialmmt_amd.eval_step import GraphedEvalStep, MeldMetrics
    act = torch.bfloat16
    compact = GraphedEvalStep(swin, mm, cfg, full, autocast_dtype=act, gumbel="sample")
    bucketed = GraphedEvalStep(swin, mm, cfg, padded[0], autocast_dtype=act, gumbel="sample", frame_capacity=BUCKETS,
                               metrics=MeldMetrics(swin.num_labels, dev, collect_rows=rows))
    return compact, bucketed


def split_ms(step, batches, n):
    from facialmmt_amd.eval_step import evaluate
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, results, truths = evaluate(step, [batches[i % len(batches)] for i in range(n)])
    torch.cuda.synchronize()
    assert results.shape[0] == truths.shape[0] == n * batches[0][7].shape[0]
    return (time.perf_counter() - t0) * 1e3 / n


def census(leg, batches):
    """kernel launches per batch of one leg, from a rocprofv3 kernel trace of a child process"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    out = tempfile.mkdtemp(prefix="fmmt_eval_ragged_census_")
    try:
        counts = []
        for n in (batches, 2 * batches):                        # two runs: the difference is free of set-up, warm-up and capture launches
            d = os.path.join(out, str(n))
            cmd = [prof, "--kernel-trace", "--stats", "-d", d, "-o", "r", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--census-leg", leg, "--batches", str(n)]
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"census child ({leg}) exited with {r.returncode}: {r.stderr[-400:]}")
            f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
            counts.append(sum(int(row["Calls"]) for row in csv.DictReader(open(f))))
        return (counts[1] - counts[0]) / batches
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    a = parse()
    assert torch.cuda.is_available(), "bench_eval_ragged.py needs an MI355X"
    args, dev, cfg, swin, mm, counts, padded, compact_batches, full = setup()
    compact, bucketed = make_legs(swin, mm, cfg, dev, padded, full, a.batches * args.utts)
    legs = {"compact": (compact, compact_batches), "bucketed": (bucketed, padded)}
    if a.census_leg:
        split_ms(*legs[a.census_leg], a.batches)
        return
    for _ in range(a.warmup):
        for step, bs in legs.values():
            split_ms(step, bs, len(bs))                         # every shape the timed window uses
    compact.fallbacks = compact.replays = bucketed.fallbacks = bucketed.replays = 0
    rounds = []
    for _ in range(a.rounds):                                   # alternate: clock and thermal drift reach both legs alike
        rounds.append([split_ms(*legs[name], a.batches) for name in ("compact", "bucketed")])
    from facialmmt_amd.eval_step import pick_bucket
    hist = collections.Counter(pick_bucket(counts[i % len(counts)], args.frames, BUCKETS) for i in range(a.batches))
    med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(2)]
    r = bucketed.metrics.result()
    launches = {"compact": None, "bucketed": None}
    stats = {name: (legs[name][0].replays, legs[name][0].fallbacks) for name in legs}
    if not a.no_census:
        del compact, bucketed, legs
        for leg in launches:
            launches[leg] = census(leg, 8)
    totals = [sum(n) for n in counts]
    print(json.dumps({
        "metric": "eval_ragged_ms_per_batch", "config": f"{args.utts} utterances x Lv = {args.frames}, {args.plm}, bf16; frame totals {totals} cycled", "batches_per_split": a.batches,
        "rounds": [[round(x, 3) for x in rr] for rr in rounds],
        "compact": {"ms_per_batch": round(med[0], 3), "launches_per_batch": launches["compact"], "replays": stats["compact"][0], "fallbacks": stats["compact"][1],
                    "what": "GraphedEvalStep without frame_capacity on compact frames: falls back launch by launch, evaluate() clones per batch"},
        "bucketed": {"ms_per_batch": round(med[1], 3), "launches_per_batch": launches["bucketed"], "replays": stats["bucketed"][0], "fallbacks": stats["bucketed"][1],
                     "buckets": list(BUCKETS), "bucket_histogram_per_split": {str(k): hist[k] for k in BUCKETS},
                     "what": "GraphedEvalStep(frame_capacity=(384, 512, 640)), MeldMetrics(collect_rows): one replay per batch, no clone"},
        "compact_over_bucketed": round(med[0] / med[1], 3), "rows_counted_last_split": r.count, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
