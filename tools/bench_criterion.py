"""What the criterion (train_step.Criterion: class weights, label smoothing; csrc/ce_loss.hip) costs or gains.  One process, one call, two parts:

  kernel  forward + backward of ops.ce_loss against autograd through F.cross_entropy(logits.float(), labels, weight=, label_smoothing=) on (4, 7) and
          (150, 7) bf16 logits -- the target and the auxiliary step's shapes: the launches of one forward + backward (torch.profiler), the wall time per
          pair issued eagerly, and for ops.ce_loss the time per pair inside a replayed graph of `--pairs` pairs (what a captured step pays; torch's weighted
          cross_entropy is not captured here: under stream capture it raises hipErrorStreamCaptureUnsupported).  Legs alternate over rounds.
  step    the graphed T+A+V step and the graphed auxiliary step (150 images) with criterion=None and with a weighted, smoothed criterion, legs over
          models of their own, alternating over the rounds; wall clock between device synchronisations.

Prints one JSON line.

    python tools/bench_criterion.py [--part kernel|step|both] [--pairs 50] [--rounds 5] [--steps 20] [--aux-steps 10] [--warmup 5] [--time-limit 900]"""
import argparse
import faulthandler
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_param_groups import count_launches, median  # noqa: E402

WEIGHTS = [0.4, 2.1, 2.6, 1.9, 1.2, 2.9, 1.5]                 # neutral down, the rare classes up: the edit a run on MELD makes
EPS = 0.1


def kernel_part(a, dev):
    from facialmmt_amd import ops
    from facialmmt_amd.graph_capture import _KEEP_GRAPHS, capture_window
    w = torch.tensor(WEIGHTS, device=dev)
    out = {}
    for B in (4, 150):
        g = torch.Generator(device=dev).manual_seed(B)
        x = torch.randn(B, 7, device=dev, generator=g).bfloat16().requires_grad_(True)
        y = torch.randint(0, 7, (B,), device=dev, generator=g)

        def ours():
            return torch.autograd.grad(ops.ce_loss(x, y, w, EPS), x)[0]

        def stock():
            return torch.autograd.grad(F.cross_entropy(x.float(), y, weight=w, label_smoothing=EPS), x)[0]
        legs = {"ce_loss": ours, "torch": stock}
        graphs = {}
        for name, fn in legs.items():
            if name == "torch":
                for _ in range(3):
                    fn()
                continue
            s = torch.cuda.Stream(dev)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with capture_window(), torch.cuda.graph(graphs[name], stream=s):
                for _ in range(a.pairs):
                    fn()
            graphs[name].replay()
        torch.cuda.synchronize()
        eager, replay = {k: [] for k in legs}, {k: [] for k in legs}
        for r in range(a.rounds):
            for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.pairs):
                    legs[name]()
                torch.cuda.synchronize()
                eager[name].append((time.perf_counter() - t0) / a.pairs * 1e6)
                if name not in graphs:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[name].replay()
                e1.record()
                e1.synchronize()
                replay[name].append(e0.elapsed_time(e1) / a.pairs * 1e3)
        diff = float((ours().float() - stock().float()).abs().max())
        out[f"{B}x7"] = {"launches_fwd_bwd": {k: count_launches(fn) for k, fn in legs.items()},
                         "eager_us_per_pair": {k: round(median(v), 2) for k, v in eager.items()},
                         "replayed_us_per_pair": {k: round(median(v), 2) for k, v in replay.items() if v},
                         "replayed_min_max_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in replay.items() if v},
                         "max_abs_gradient_difference": diff}
        _KEEP_GRAPHS.append(tuple(graphs.values()))
    return dict(out, pairs_per_leg_and_round=a.pairs, rounds=a.rounds, dtype="bf16 logits", weights=WEIGHTS, label_smoothing=EPS)


def _timed(call, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def _alternate(a, calls, steps):
    for c in calls.values():
        _timed(c, a.warmup)
    ms = {k: [] for k in calls}
    for r in range(a.rounds):
        for name in (list(calls) if r % 2 == 0 else list(calls)[::-1]):
            ms[name].append(_timed(calls[name], steps))
    med = {k: median(v) for k, v in ms.items()}
    return {"median_ms": {k: round(v, 3) for k, v in med.items()}, "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            "difference_ms": round(med["criterion"] - med["none"], 3), "steps_per_leg_and_round": steps, "rounds": a.rounds}


def step_part(a, bench, bargs, dev, cfg):
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import Criterion, GraphedAuxStep, GraphedTargetStep, HFAdamW, MasterWeights, step_parameters
    crit = Criterion(WEIGHTS, EPS, device=dev)
    batch = bench.synth_batch(bargs, dev, 0, cfg)
    target, keep = {}, []
    for name, c in (("none", None), ("criterion", crit)):
        swin, mm = bench.build_models(bargs, dev, cfg)
        masters = MasterWeights(mm.roberta if mm.text_pretrained_model == "roberta" else mm.bert, torch.bfloat16)
        params = step_parameters(mm, masters)
        opt = HFAdamW(params, lr=torch.tensor(cfg.trg_lr, device=dev), weight_decay=cfg.weight_decay)
        step = GraphedTargetStep(swin, mm, opt, None, cfg, batch, autocast_dtype=torch.bfloat16, averager=GradientAverager(params, hooks=False), masters=masters,
                                 criterion=c)
        assert step.fused is not None
        keep.append(step)
        target[name] = lambda step=step: step(batch)
    out = {"target": _alternate(a, target, a.steps)}
    out["target"]["last_loss"] = {k: float(c()[0]) for k, c in target.items()}
    del target, keep
    torch.cuda.empty_cache()
    bargs.aux_images = 150
    images, labels = bench.synth_aux_batch(bargs, dev, 0)
    aux, keep = {}, []
    for name, c in (("none", None), ("criterion", crit)):
        swin, _ = bench.build_models(bargs, dev, cfg)
        opt = HFAdamW(swin.parameters(), lr=torch.tensor(cfg.aux_lr, device=dev))
        step = GraphedAuxStep(swin, opt, None, cfg, images, labels, averager=GradientAverager(swin.parameters(), hooks=False), criterion=c)
        keep.append(step)
        aux[name] = lambda step=step: step(images, labels)
    out["auxiliary"] = _alternate(a, aux, a.aux_steps)
    out["auxiliary"]["last_loss"] = {k: float(c()) for k, c in aux.items()}
    out["auxiliary"]["images"] = 150
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["kernel", "step", "both"])
    ap.add_argument("--pairs", type=int, default=50, help="kernel part: forward + backward pairs per leg and round (and per captured graph)")
    ap.add_argument("--rounds", type=int, default=5, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--steps", type=int, default=20, help="step part: timed target steps per leg and round")
    ap.add_argument("--aux-steps", type=int, default=10, help="step part: timed auxiliary steps per leg and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the process ends itself")
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.time_limit, exit=True)
    assert torch.cuda.is_available(), "bench_criterion.py needs an MI355X"
    import bench_ragged
    from facialmmt_amd.config import default_args
    bench, bargs = bench_ragged.bench_args()
    dev = torch.device("cuda:0")
    cfg = default_args(get_vision_utt_max_lens=bargs.frames, trg_accumulation_steps=1)
    out = {"metric": "criterion", "config": f"bf16, {bargs.utts} utterances, Lv = {bargs.frames}, roberta-large with fp32 masters, HF AdamW",
           "device": torch.cuda.get_device_name(0)}
    if a.part in ("kernel", "both"):
        out["kernel"] = kernel_part(a, dev)
    if a.part in ("step", "both"):
        out["step"] = step_part(a, bench, bargs, dev, cfg)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
