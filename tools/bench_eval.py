"""Evaluation throughput at configs[1] (4 utterances x 160 frames, RoBERTa-large, bf16), two legs in ONE process and ONE call:
  (a) the eager evaluation a user assembles from the public API without eval_step: modules in eval(), no_grad, Swin -> frame filter -> multimodal
      forward, `F.cross_entropy(...).item()` per batch as the reference does (train.py:154-243);
  (b) eval_step.GraphedEvalStep: the same batch as one HIP-graph replay, metrics accumulated on the device.
Models and batch are built the way bench.py builds them (bf16 text encoder through MasterWeights, as the benchmark's step has it).  Prints one
JSON line: ms per batch, utterances/s and kernel launches per batch for both legs.

    python tools/bench_eval.py [--batches 40] [--warmup 5] [--rounds 3]

Launch counts: the script re-runs itself under `rocprofv3 --kernel-trace --stats` (a child process per leg, `--census-leg`) and reads the census
with tools/count_launches.py's arithmetic; `--no-census` skips that (launch counts null)."""
import argparse
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

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40, help="timed batches per round and leg")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="the two legs alternate this many times; the median round is reported")
    ap.add_argument("--no-census", action="store_true")
    ap.add_argument("--census-leg", choices=["eager", "graphed"], default=None, help="internal: run `--batches` batches of one leg and exit (profiled child)")
    return ap.parse_args()


def setup():
    import bench
    from facialmmt_amd.config import default_args
    from facialmmt_amd.train_step import MasterWeights
    saved, sys.argv = sys.argv, [sys.argv[0]]
    args = bench.parse()                                       # configs[1] defaults
    sys.argv = saved
    args.plm = args.plm or "roberta-large"
    dev = torch.device("cuda:0")
    cfg = default_args(get_vision_utt_max_lens=args.frames, trg_accumulation_steps=1)
    swin, mm = bench.build_models(args, dev, cfg)
    MasterWeights(mm.roberta, torch.bfloat16)                   # the benchmark's text encoder: bf16 parameters, fused sublayers
    batches = [bench.synth_batch(args, dev, r, cfg) for r in range(2)]
    return args, dev, cfg, swin, mm, batches


def eager_leg(swin, mm, cfg, act):
    from facialmmt_amd.train_step import select_frames

    def run(batch):
        (ids, attn_mask, sep_mask, audio, audio_mask, vision, vision_mask, labels, frames, num_imgs, utt_idx) = batch
        with torch.no_grad():
            preds = swin(frames, is_trg_task=True)
            vis, new_mask = select_frames(preds.float(), vision, vision_mask, num_imgs, cfg.FacialEmoImpor_threshold)
            with torch.autocast("cuda", dtype=act):
                logits = mm(ids, attn_mask, sep_mask, audio, audio_mask, vis, new_mask, utt_idx)
            return F.cross_entropy(logits.float(), labels).item() * labels.shape[0]
    return run


def timed(fn, batches, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def census(leg, batches):
    """kernel launches per batch of one leg, from a rocprofv3 kernel trace of a child process"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    out = tempfile.mkdtemp(prefix="fmmt_eval_census_")
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
    assert torch.cuda.is_available(), "bench_eval.py needs an MI355X"
    args, dev, cfg, swin, mm, batches = setup()
    act = torch.bfloat16
    swin.eval()
    mm.eval()
    eager = eager_leg(swin, mm, cfg, act)
    if a.census_leg == "eager":
        for i in range(a.batches):
            eager(batches[i % 2])
        torch.cuda.synchronize()
        return
    from facialmmt_amd.eval_step import GraphedEvalStep
    graphed = GraphedEvalStep(swin, mm, cfg, batches[0], autocast_dtype=act, gumbel="sample")
    if a.census_leg == "graphed":
        for i in range(a.batches):
            graphed(batches[i % 2])
        torch.cuda.synchronize()
        return
    for _ in range(a.warmup):
        eager(batches[0])
        graphed(batches[0])
    rounds = []
    for _ in range(a.rounds):                                   # alternate: clock and thermal drift reach both legs alike
        rounds.append((timed(eager, batches, a.batches), timed(lambda b: graphed(b), batches, a.batches)))
    r = graphed.metrics.result()                                # the split's one device-to-host copy
    e_ms = sorted(x[0] for x in rounds)[len(rounds) // 2]
    g_ms = sorted(x[1] for x in rounds)[len(rounds) // 2]
    utts = args.utts
    launches = {"eager": None, "graphed": None}
    if not a.no_census:
        del graphed
        for leg in launches:
            launches[leg] = census(leg, 6)
    print(json.dumps({
        "metric": "eval_ms_per_batch", "config": f"configs[1]: {utts} utterances x {args.frames} frames, {args.plm}, bf16", "batches_per_round": a.batches,
        "rounds": [[round(x, 3), round(y, 3)] for x, y in rounds],
        "eager": {"ms_per_batch": round(e_ms, 3), "utterances_per_s": round(utts * 1e3 / e_ms, 2), "launches_per_batch": launches["eager"],
                  "what": "modules in eval(), no_grad, F.cross_entropy(...).item() per batch"},
        "graphed": {"ms_per_batch": round(g_ms, 3), "utterances_per_s": round(utts * 1e3 / g_ms, 2), "launches_per_batch": launches["graphed"],
                    "what": "eval_step.GraphedEvalStep: one graph replay per batch, metrics on the device"},
        "speedup": round(e_ms / g_ms, 3), "rows_counted": r.count, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
