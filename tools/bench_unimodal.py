"""V-only training step time at configs[0] shapes (B = 4 and 16 utterances x 160 frames of 512-d face features, bf16 kernels, AdamW, accumulation 1), three
legs in ONE process and ONE call, alternating:
  (a) the eager step assembled from the existing modules as train.py:245-273 writes it: model(feature, mask), F.cross_entropy, backward, clip_grad_norm_,
      optimizer.step(), zero_grad -- what the project could do before train_step.UnimodalStep existed;
  (b) train_step.UnimodalStep (the tail behind the encoder as ops.pool_head_loss);
  (c) train_step.GraphedUnimodalStep (two HIP-graph replays per step, fused clip + AdamW).
Each leg owns a model with the same initial values.  Inputs stay on the device; wall clock between device synchronisations.  Prints one JSON line.

    python tools/bench_unimodal.py [--steps 40] [--warmup 5] [--rounds 3]

Launch counts: the script re-runs itself under `rocprofv3 --kernel-trace --stats` (a child process per leg and run, `--census-leg`, the program after `--`,
no counters collected) for 6 and 12 steps; the difference over 6 is the launches per step, and the rows of the new head's kernels (ph_fwd_* / ph_bwd_*) give
its launches per step by name.  `--no-census` skips that."""
import argparse
import csv
import glob
import json
import os
import re
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

FRAMES = 160


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed steps per round and leg")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--utts", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--no-census", action="store_true")
    ap.add_argument("--census-leg", choices=["eager", "step", "graphed"], default=None, help="internal: run `--steps` steps of one leg at --utts[0] and exit")
    return ap.parse_args()


def build(dev, utts):
    from facialmmt_amd import models, synth
    from facialmmt_amd.config import default_args
    cfg = default_args(get_vision_utt_max_lens=FRAMES, trg_accumulation_steps=1, compute_dtype=torch.bfloat16)
    model = models.meld_utt_transformer(cfg)
    synth.fill_state_dict(model, seed=201)
    model.to(dev).train()
    from facialmmt_amd.train_step import HFAdamW                  # transformers.AdamW's update, the class the reference constructs (train.py:307,333)
    opt = HFAdamW(model.parameters(), lr=torch.tensor(cfg.trg_lr, device=dev), weight_decay=cfg.weight_decay)
    return cfg, model, opt


def batches(dev, utts, n=2):
    from facialmmt_amd import synth
    out = []
    for r in range(n):
        x = synth.tensor("vfeat_bench", (utts, FRAMES, 512), seed=500 + r).to(dev)
        mask = torch.ones(utts, FRAMES, device=dev)
        for u in range(utts):
            mask[u, FRAMES - (13 * u + 7 * r) % 60:] = 0
        labels = torch.from_numpy(synth.randint("labels_bench", (utts,), 0, 7, seed=600 + r)).to(dev)
        out.append((x, mask, labels))
    return out


def make_leg(name, dev, utts, sample):
    cfg, model, opt = build(dev, utts)
    if name == "eager":
        def run(batch):
            feature, mask, labels = batch
            loss = F.cross_entropy(model(feature, mask), labels) / cfg.trg_accumulation_steps
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.clip)
            opt.step()
            opt.zero_grad()
            return loss.detach()
        return run
    from facialmmt_amd.train_step import GraphedUnimodalStep, UnimodalStep
    if name == "step":
        return UnimodalStep(model, opt, None, cfg)
    return GraphedUnimodalStep(model, opt, None, cfg, sample)


def timed(fn, bs, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(bs[i % len(bs)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def census(leg, utts, steps=6):
    """(kernel launches per step, {head kernel name: launches per step}) of one leg from two rocprofv3 kernel traces of child processes"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, None
    out = tempfile.mkdtemp(prefix="fmmt_unimodal_census_")
    try:
        totals, heads = [], []
        for n in (steps, 2 * steps):                            # two runs: the difference is free of set-up, warm-up and capture launches
            d = os.path.join(out, str(n))
            cmd = [prof, "--kernel-trace", "--stats", "-d", d, "-o", "r", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                   "--census-leg", leg, "--steps", str(n), "--utts", str(utts)]
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"census child ({leg}) exited with {r.returncode}: {r.stderr[-400:]}")
            f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
            rows = list(csv.DictReader(open(f)))
            totals.append(sum(int(row["Calls"]) for row in rows))
            hd = {}
            for row in rows:
                m = re.search(r"ph_(?:fwd|bwd)_\w+", row["Name"])
                if m:
                    hd[m.group(0)] = hd.get(m.group(0), 0) + int(row["Calls"])
            heads.append(hd)
        head = {k: (heads[1].get(k, 0) - heads[0].get(k, 0)) / steps for k in heads[1]}
        return (totals[1] - totals[0]) / steps, head
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    a = parse()
    assert torch.cuda.is_available(), "bench_unimodal.py needs an MI355X"
    dev = torch.device("cuda:0")
    if a.census_leg:
        bs = batches(dev, a.utts[0])
        leg = make_leg(a.census_leg, dev, a.utts[0], bs[0])
        for i in range(a.steps):
            leg(bs[i % 2])
        torch.cuda.synchronize()
        return
    results = []
    for utts in a.utts:
        bs = batches(dev, utts)
        legs = {name: make_leg(name, dev, utts, bs[0]) for name in ("eager", "step", "graphed")}
        for _ in range(a.warmup):
            for leg in legs.values():
                leg(bs[0])
        rounds = []
        for _ in range(a.rounds):                               # alternate: clock and thermal drift reach every leg alike
            rounds.append([timed(legs[name], bs, a.steps) for name in ("eager", "step", "graphed")])
        med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(3)]
        spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in range(3)]
        launches, head = {"eager": None, "graphed": None}, None
        del legs
        if not a.no_census:
            launches["eager"], _ = census("eager", utts)
            launches["graphed"], head = census("graphed", utts)
        results.append({"utterances": utts, "rounds_ms": [[round(x, 3) for x in r] for r in rounds],
                        "eager_ms": round(med[0], 3), "unimodal_step_ms": round(med[1], 3), "graphed_ms": round(med[2], 3),
                        "spread_ms": [round(x, 3) for x in spread], "graphed_vs_eager": round(med[0] / med[2], 3),
                        "launches_per_step": launches, "head_launches_per_step": head})
    print(json.dumps({"metric": "unimodal_train_step_ms", "config": f"configs[0] shapes: {a.utts} utterances x {FRAMES} frames x 512, two layers, bf16 kernels, AdamW, "
                      "accumulation 1", "steps_per_round": a.steps, "legs": ["eager (train.py:245-273 on the existing modules)", "UnimodalStep", "GraphedUnimodalStep"],
                      "results": results, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
