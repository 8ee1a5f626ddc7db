"""What the per-tensor gradient report costs, on the benchmark's own parameter set (bench.py's headline configuration: bf16, 4 utterances, Lv = 160,
RoBERTa-large in bf16 with fp32 masters -- step_parameters(mm, masters), about 435 M fp32 values).  One process, one call, two parts:

  kernel  fmmt_table_stats over the gradient field (with the norm word and the snapshot buffers, as the captured update calls it) and over the first
          moments (on demand: no norm word), beside fmmt_param_digest and fmmt_adamw_batch (learning rate 0: the parameters keep their bits) on the
          SAME descriptor table.  Legs alternate over the rounds; each leg of a round is `--launches` calls between two device events.  Bytes per
          call: 4 per element for the statistics, 12 for the digest, 28 plus 2 per bf16 twin for the update.
  step    the graphed T+A+V step with grad_report off and on, two legs over models of their own, alternating over the rounds; wall clock between
          device synchronisations.  The launches of the update are counted with torch.profiler over one eager tail.update() behind the timing.

Prints one JSON line.

    python tools/bench_grad_report.py [--part kernel|step|both] [--launches 50] [--rounds 5] [--steps 20] [--warmup 5] [--time-limit 900]"""
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

from bench_param_groups import count_launches, median  # noqa: E402


def kernel_part(a, bench, bargs, dev, cfg):
    from facialmmt_amd import _lib, ops
    from facialmmt_amd.train_step import FusedClipAdamW, GradReport, HFAdamW, MasterWeights, named_step_parameters, step_parameters
    _, mm = bench.build_models(bargs, dev, cfg)
    masters = MasterWeights(mm.roberta if mm.text_pretrained_model == "roberta" else mm.bert, torch.bfloat16)
    params = step_parameters(mm, masters)
    low_of = {id(m): l for l, m in masters.pairs()}
    g = torch.Generator(device=dev).manual_seed(1)
    grads = {p: 1e-3 * torch.randn(p.shape, device=dev, generator=g) for p in params}
    base = HFAdamW(params, lr=torch.tensor(0.0, device=dev), weight_decay=cfg.weight_decay)
    report = GradReport(named_step_parameters(mm, masters))
    fused = FusedClipAdamW(base, params, grads, low_of, cfg.clip, report=report)     # the table, the moments, the norm: built the product's way
    fused.update()                                                                   # one real update (lr 0): a norm in the norm word, moments non-zero
    elements = sum(p.numel() for p in params)
    twins = sum(p.numel() for p in params if id(p) in low_of)
    b1, b2 = base.param_groups[0]["betas"]
    eps, wd = base.param_groups[0]["eps"], base.param_groups[0]["weight_decay"]
    on_demand = torch.empty((fused.n, 4), dtype=torch.int32, device=dev)
    legs = [("stats_g_a", lambda: report.record(fused.norm), 4 * elements),
            ("stats_m", lambda: ops.table_stats(_lib.STATS_M, fused.n, fused.blocks, fused.desc, report.partial, on_demand), 4 * elements),
            ("digest", lambda: fused.digest(), 12 * elements),
            ("adamw_batch", lambda: ops.adamw_batch(fused.n, fused.blocks, fused.desc, fused.lr, fused.step, fused.norm, b1, b2, eps, wd, fused.max_norm, True),
             28 * elements + 2 * twins),
            ("stats_g_b", lambda: report.record(fused.norm), 4 * elements)]
    before = [p.detach().clone() for p in params[:4]]
    for _, fn, _ in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in legs}
    for r in range(a.rounds):
        for name, fn, _ in (legs if r % 2 == 0 else legs[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.launches)
    assert all(torch.equal(x, p.detach()) for x, p in zip(before, params))           # lr 0: nothing moved
    r = report.read()
    want = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads.values())))
    med = {k: median(v) for k, v in ms.items()}
    nbytes = {name: b for name, _, b in legs}
    return {"parameters": len(params), "elements": elements, "elements_with_bf16_twin": twins, "blocks": fused.blocks, "bytes_per_call": nbytes,
            "launches_per_leg_and_round": a.launches, "rounds": a.rounds,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "TB_per_s": {k: round(nbytes[k] / (v * 1e-3) / 1e12, 3) for k, v in med.items()},
            "report_total_norm": r.total_norm, "fp64_total_norm": want, "norm_word": float(fused.norm), "bad_updates": r.bad_updates}


def step_part(a, bench, bargs, dev, cfg):
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, step_parameters
    batch = bench.synth_batch(bargs, dev, 0, cfg)
    legs = {}
    for name, on in (("off", False), ("on", True)):
        swin, mm = bench.build_models(bargs, dev, cfg)
        masters = MasterWeights(mm.roberta if mm.text_pretrained_model == "roberta" else mm.bert, torch.bfloat16)
        params = step_parameters(mm, masters)
        opt = HFAdamW(params, lr=torch.tensor(cfg.trg_lr, device=dev), weight_decay=cfg.weight_decay)
        legs[name] = GraphedTargetStep(swin, mm, opt, None, cfg, batch, autocast_dtype=torch.bfloat16, averager=GradientAverager(params, hooks=False), masters=masters,
                                       grad_report=on)
        assert legs[name].fused is not None and (legs[name].grad_report is not None) == on

    def timed(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for step in legs.values():
        timed(step, a.warmup)
    ms = {name: [] for name in legs}
    for r in range(a.rounds):
        for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            ms[name].append(timed(legs[name], a.steps))
    losses = {name: float(step(batch)[0]) for name, step in legs.items()}
    rep = legs["on"].grad_report.read()
    worst = rep.worst(3)
    launches = {name: count_launches(step.tail.update) for name, step in legs.items()}
    med = {k: median(v) for k, v in ms.items()}
    return {"optimizer": "HFAdamW, one group, device learning rate", "steps_per_leg_and_round": a.steps, "rounds": a.rounds,
            "median_ms": {k: round(v, 3) for k, v in med.items()}, "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            "difference_ms": round(med["on"] - med["off"], 3), "update_launches": launches, "last_loss": losses,
            "report": {"tensors": len(rep.names), "total_norm": rep.total_norm, "norm_word": float(legs["on"].fused.norm), "bad_updates": rep.bad_updates,
                       "nonfinite": int(rep.nonfinite.sum()), "worst": worst}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["kernel", "step", "both"])
    ap.add_argument("--launches", type=int, default=50, help="kernel part: calls per leg and round")
    ap.add_argument("--rounds", type=int, default=5, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--steps", type=int, default=20, help="step part: timed steps per leg and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the process ends itself")
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.time_limit, exit=True)
    assert torch.cuda.is_available(), "bench_grad_report.py needs an MI355X"
    import bench_ragged
    from facialmmt_amd.config import default_args
    bench, bargs = bench_ragged.bench_args()
    dev = torch.device("cuda:0")
    cfg = default_args(get_vision_utt_max_lens=bargs.frames, trg_accumulation_steps=1)
    out = {"metric": "grad_report", "config": f"bf16, {bargs.utts} utterances, Lv = {bargs.frames}, roberta-large with fp32 masters, HF AdamW",
           "device": torch.cuda.get_device_name(0)}
    if a.part in ("kernel", "both"):
        out["kernel"] = kernel_part(a, bench, bargs, dev, cfg)
        torch.cuda.empty_cache()
    if a.part in ("step", "both"):
        out["step"] = step_part(a, bench, bargs, dev, cfg)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
