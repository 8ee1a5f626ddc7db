"""What parameter groups cost and what the fused update over them saves, on the benchmark's own parameter set (bench.py's headline configuration: bf16,
4 utterances, Lv = 160, RoBERTa-large in bf16 with fp32 masters -- step_parameters(mm, masters), about 435 M fp32 values, the text encoder's with a
bf16 twin).  One process, one call, two parts:

  kernel  fmmt_adamw_batch against fmmt_adamw_groups with n_groups = 1, 2 (decay / no decay) and 26 (embeddings, the 24 encoder layers, the rest)
          on the SAME descriptor table, gradients, moments and twins; every learning rate 0, so the parameters keep their bits while the arithmetic
          and the traffic are the full update's.  Legs alternate over the rounds (batch, groups1, groups2, groups26, batch again); each leg of a
          round is `--launches` launches between two device events.  The two fmmt_adamw_batch legs span the interval the n_groups = 1 leg is held
          to: inside [min - gap, max + gap] with gap = their difference (`groups1_inside`).
  step    the graphed T+A+V step with a decay / no-decay HFAdamW (two groups, two device learning rates, a LambdaLR with two lambdas) under
          train_step.FUSED_ADAMW True (one fused launch, fmmt_adamw_groups) and False (clip_grad_norm_ + optimizer.step() + masters.sync_low(),
          what the step did for such an optimizer before), alternating over the rounds; wall clock between device synchronisations.  The launches
          of the update are counted with torch.profiler over one eager tail.update() behind the timing.

Prints one JSON line.  The kernels' register counts and occupancy are the compiler's (-Rpass-analysis=kernel-resource-usage), not measured here.

    python tools/bench_param_groups.py [--part kernel|step|both] [--launches 50] [--rounds 7] [--steps 20] [--warmup 5] [--time-limit 900]"""
import argparse
import faulthandler
import json
import os
import re
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402


def no_decay(name):
    return name.endswith("bias") or "LayerNorm" in name


LAYER = re.compile(r"(?:roberta|bert)\.encoder\.layer\.(\d+)\.")


def layer_groups(named):
    """(group index by name, number of groups) of a layer-wise split: 0 = the text encoder's embeddings, 1..L its layers, L + 1 everything else
    (pooler, fusion stack, heads) -- 26 groups for RoBERTa-large"""
    layers = 1 + max(int(m.group(1)) for m in (LAYER.search(n) for n, _ in named) if m)

    def index(name):
        m = LAYER.search(name)
        if m:
            return 1 + int(m.group(1))
        return 0 if re.match(r"(?:roberta|bert)\.embeddings\.", name) else layers + 1
    return index, layers + 2


def grouped_optimizer(named, group_index, n_groups, dev, cfg, lr=None):
    from facialmmt_amd.train_step import HFAdamW
    members = [[] for _ in range(n_groups)]
    for name, p in named:
        members[group_index(name)].append(p)
    assert all(members), [len(m) for m in members]
    return HFAdamW([dict(params=ps, lr=torch.tensor(cfg.trg_lr if lr is None else lr, device=dev),
                         weight_decay=0.0 if (n_groups == 2 and j == 1) else cfg.weight_decay) for j, ps in enumerate(members)])


def median(xs):
    return sorted(xs)[len(xs) // 2]


def kernel_part(a, bench, bargs, dev, cfg):
    from facialmmt_amd import ops
    from facialmmt_amd.train_step import FusedClipAdamW, HFAdamW, MasterWeights, group_plan, group_tables, named_step_parameters, step_parameters
    _, mm = bench.build_models(bargs, dev, cfg)
    masters = MasterWeights(mm.roberta if mm.text_pretrained_model == "roberta" else mm.bert, torch.bfloat16)
    params = step_parameters(mm, masters)
    named = list(named_step_parameters(mm, masters))
    assert [id(p) for _, p in named] == [id(p) for p in params]
    low_of = {id(m): l for l, m in masters.pairs()}
    g = torch.Generator(device=dev).manual_seed(1)
    grads = {p: 1e-3 * torch.randn(p.shape, device=dev, generator=g) for p in params}
    base = HFAdamW(params, lr=torch.tensor(0.0, device=dev), weight_decay=cfg.weight_decay)
    fused = FusedClipAdamW(base, params, grads, low_of, cfg.clip)          # the table, the moments, the norm: built the product's way
    assert fused.group_table is None
    fused.update()                                                          # one real update (lr 0): step = 1, a norm in the norm word, moments non-zero
    elements = sum(p.numel() for p in params)
    twins = sum(p.numel() for p in params if id(p) in low_of)
    nbytes = 28 * elements + 2 * twins
    tables = {}
    by_layer, n_layerwise = layer_groups(named)
    for n_groups, index in ((1, lambda n: 0), (2, lambda n: int(no_decay(n))), (n_layerwise, by_layer)):
        opt = grouped_optimizer(named, index, n_groups, dev, cfg, lr=0.0)
        plan = group_plan(opt, params)
        tables[n_groups] = group_tables(plan, dev) + (opt,)
    b1, b2 = base.param_groups[0]["betas"]
    eps, wd = base.param_groups[0]["eps"], base.param_groups[0]["weight_decay"]

    def batch():
        ops.adamw_batch(fused.n, fused.blocks, fused.desc, fused.lr, fused.step, fused.norm, b1, b2, eps, wd, fused.max_norm, True)

    def groups(n):
        group_of, table, _ = tables[n]
        return lambda: ops.adamw_groups(fused.n, fused.blocks, fused.desc, n, group_of, table, fused.step, fused.norm, fused.max_norm, True)
    legs = [("batch_a", batch), ("groups1", groups(1)), ("groups2", groups(2)), ("groups26", groups(n_layerwise)), ("batch_b", batch)]
    before = [p.detach().clone() for p in params[:4]]
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for r in range(a.rounds):
        for name, fn in (legs if r % 2 == 0 else legs[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.launches)
    assert all(torch.equal(x, p.detach()) for x, p in zip(before, params))   # lr 0: nothing moved
    med = {k: median(v) for k, v in ms.items()}
    lo, hi = sorted((med["batch_a"], med["batch_b"]))
    gap = hi - lo
    return {"parameters": len(params), "elements": elements, "elements_with_bf16_twin": twins, "blocks": fused.blocks, "bytes_per_launch": nbytes,
            "launches_per_leg_and_round": a.launches, "rounds": a.rounds,
            "n_groups": {"groups1": 1, "groups2": 2, "groups26": n_layerwise},
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
            "GB_per_s": {k: round(nbytes / (v * 1e-3) / 1e9, 1) for k, v in med.items()},
            "batch_interval_ms": [round(lo - gap, 4), round(hi + gap, 4)], "groups1_inside": bool(lo - gap <= med["groups1"] <= hi + gap)}


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def step_part(a, bench, bargs, dev, cfg):
    from facialmmt_amd import train_step
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep, MasterWeights, named_step_parameters, step_parameters
    batch = bench.synth_batch(bargs, dev, 0, cfg)
    lr_of = lambda s: min(1.0, (s + 1) / 100.0)
    legs = {}
    for name, fused in (("fused", True), ("stock", False)):
        train_step.FUSED_ADAMW = fused
        swin, mm = bench.build_models(bargs, dev, cfg)
        masters = MasterWeights(mm.roberta if mm.text_pretrained_model == "roberta" else mm.bert, torch.bfloat16)
        params = step_parameters(mm, masters)
        opt = grouped_optimizer(list(named_step_parameters(mm, masters)), lambda n: int(no_decay(n)), 2, dev, cfg)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, [lr_of, lr_of])
        legs[name] = GraphedTargetStep(swin, mm, opt, sched, cfg, batch, autocast_dtype=torch.bfloat16, averager=GradientAverager(params, hooks=False), masters=masters)
        assert (legs[name].fused is not None) == fused
    train_step.FUSED_ADAMW = True

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
    launches = {name: count_launches(step.tail.update) for name, step in legs.items()}
    med = {k: median(v) for k, v in ms.items()}
    return {"optimizer": "HFAdamW, two groups (decay / no decay on biases and LayerNorm weights), two device learning rates, LambdaLR with two lambdas",
            "steps_per_leg_and_round": a.steps, "rounds": a.rounds, "median_ms": {k: round(v, 3) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}, "difference_ms": round(med["stock"] - med["fused"], 3),
            "update_launches": launches, "last_loss": losses}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["kernel", "step", "both"])
    ap.add_argument("--launches", type=int, default=50, help="kernel part: launches per leg and round")
    ap.add_argument("--rounds", type=int, default=7, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--steps", type=int, default=20, help="step part: timed steps per leg and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the process ends itself")
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.time_limit, exit=True)
    assert torch.cuda.is_available(), "bench_param_groups.py needs an MI355X"
    import bench_ragged
    from facialmmt_amd.config import default_args
    bench, bargs = bench_ragged.bench_args()
    dev = torch.device("cuda:0")
    cfg = default_args(get_vision_utt_max_lens=bargs.frames, trg_accumulation_steps=1)
    out = {"metric": "param_groups", "config": f"bf16, {bargs.utts} utterances, Lv = {bargs.frames}, roberta-large with fp32 masters, HF AdamW",
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
