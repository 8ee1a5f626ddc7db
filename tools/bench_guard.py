"""What skip_nonfinite=True costs where it would show: the V-only training step at configs[0] shapes (4 utterances x 160 frames of 512-d face features,
bf16 kernels, HF AdamW through the fused update, accumulation 1) -- the launch-bound step, to which the option adds two one-workgroup launches per
step (ops.monitor_loss behind the loss, ops.guard_commit behind the update), one scalar load and a uniform branch per block of the update.  Two legs in ONE
process and ONE call, alternating, each a GraphedUnimodalStep over a model of its own with the same initial values:
  (a) the default step,
  (b) skip_nonfinite=True.
Inputs stay on the device and are clean, so (b) applies every update; wall clock between device synchronisations.  Prints one JSON line: the median
round of each leg, each leg's spread over the rounds (max - min), and the monitor's counters as a check that the guarded leg really ran guarded.

    python tools/bench_guard.py [--steps 200] [--warmup 20] [--rounds 7] [--utts 4]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import bench_unimodal as BU  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed steps per round and leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--utts", type=int, default=4)
    return ap.parse_args()


def main():
    a = parse()
    assert torch.cuda.is_available(), "bench_guard.py needs an MI355X"
    from facialmmt_amd.train_step import GraphedUnimodalStep
    dev = torch.device("cuda:0")
    bs = BU.batches(dev, a.utts)
    legs = {}
    for name, guard in (("default", False), ("skip_nonfinite", True)):
        cfg, model, opt = BU.build(dev, a.utts)
        legs[name] = GraphedUnimodalStep(model, opt, None, cfg, bs[0], skip_nonfinite=guard)
        assert legs[name].fused is not None
    for _ in range(a.warmup):
        for leg in legs.values():
            leg(bs[0])
    rounds = []
    for r in range(a.rounds):                                   # alternate, and swap who goes first: drift reaches both legs alike
        order = list(legs) if r % 2 == 0 else list(legs)[::-1]
        t = {name: BU.timed(legs[name], bs, a.steps) for name in order}
        rounds.append([t["default"], t["skip_nonfinite"]])
    med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(2)]
    spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in range(2)]
    mon = legs["skip_nonfinite"].monitor.read()
    total = a.warmup + a.rounds * a.steps
    assert (mon.applied, mon.skipped, mon.micro_steps, mon.nonfinite_losses) == (total, 0, total, 0), vars(mon)
    print(json.dumps({"metric": "unimodal_train_step_ms_skip_nonfinite", "config": f"configs[0] shapes: {a.utts} utterances x {BU.FRAMES} frames x 512, two layers, "
                      "bf16 kernels, HF AdamW (fused update), accumulation 1, GraphedUnimodalStep", "steps_per_round": a.steps, "rounds": a.rounds,
                      "legs": ["default", "skip_nonfinite=True"], "rounds_ms": [[round(x, 4) for x in r] for r in rounds],
                      "default_ms": round(med[0], 4), "skip_nonfinite_ms": round(med[1], 4), "difference_ms": round(med[1] - med[0], 4),
                      "spread_ms": [round(x, 4) for x in spread],
                      "monitor": {"applied": mon.applied, "skipped": mon.skipped, "micro_steps": mon.micro_steps, "avg_loss": mon.avg_loss, "last_norm": mon.last_norm},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
