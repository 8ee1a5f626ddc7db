"""What the on-device MELD ColorJitter costs, in ONE process and ONE call (same-call A/B):
  1. the fused uint8 pre-step alone at 640 crops of 160 x 160, bf16, 'cv2' resize, inference form (no patch matrix written), device events over
     back-to-back launches straight through the C ABI on preallocated buffers:
       plain     fmmt_patch_embed_u8_ln_fwd                                  (one launch; the kernel every earlier commit has)
       none      fmmt_patch_embed_u8_jitter_ln_fwd, every record "none"      (two launches; the statistic's launch leaves at once)
       jitter    the same with all four operations in a random order         (two launches; the resize is done twice)
       draw      augment.ColorJitter.draw(640) into a static table           (the launches a captured step adds in front of Swin)
  2. train_step.GraphedTargetStep on bench.py's headline batch (4 utterances x 160 frames of 112 x 112 uint8 crops, bf16, RoBERTa-large, HF AdamW),
     with and without color_jitter=ColorJitter(), each leg over models of its own with the same initial values, alternating rounds, wall clock
     between device synchronisations, the median round reported with the spread over rounds.
Launches are counted with torch.profiler over one eager call.  Prints one JSON line.

    python tools/bench_color_jitter.py [--steps 16] [--warmup 3] [--rounds 5] [--reps 200] [--size 160]"""
import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import bench_ragged as BR  # noqa: E402

N = 640


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16, help="timed steps per round and leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--reps", type=int, default=200, help="launches per single-op timing")
    ap.add_argument("--size", type=int, default=160, help="edge of the uint8 crops of part 1")
    ap.add_argument("--skip-steps", action="store_true", help="part 1 only")
    return ap.parse_args()


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def pre_step(dev, S, reps):
    from facialmmt_amd import _lib, ops, synth
    from facialmmt_amd.augment import ColorJitter
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as SW
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randint(0, 256, (N, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
    pe = SW.PatchEmbed(224, 4, 3, 96, torch.nn.LayerNorm)
    synth.fill_state_dict(pe, seed=31, prefix="pe.")
    pe.to(dev)
    code, tab, lut = ops.resize_tables("cv2", S, dev)
    w = pe.proj.weight.detach().view(96, 48).to(torch.bfloat16).contiguous()
    bias, gam, bet = pe.proj.bias.detach().float(), pe.norm.weight.detach().float(), pe.norm.bias.detach().float()
    y = torch.empty(N * 3136, 96, dtype=torch.bfloat16, device=dev)
    partial = torch.empty(N, _lib.JITTER_BANDS, dtype=torch.int32, device=dev)
    cj = ColorJitter()
    torch.manual_seed(3)
    table = cj.draw(N, dev)
    none = table.clone()
    none[:, 4:] = _lib.JITTER_NONE
    P = lambda t: t.data_ptr()

    def plain():
        _lib.check(lib.fmmt_patch_embed_u8_ln_fwd(_lib.BF16, code, N, S, P(x), P(tab), P(lut), P(w), P(bias), P(gam), P(bet), 1e-5, None, None, P(y), None, None, st), "plain")

    def jittered(t):
        _lib.check(lib.fmmt_patch_embed_u8_jitter_ln_fwd(_lib.BF16, code, N, S, P(x), P(tab), P(lut), P(t), P(partial), P(w), P(bias), P(gam), P(bet), 1e-5,
                                                         None, None, P(y), None, None, st), "jitter")
    static = torch.empty_like(table)

    def draw():
        static.copy_(cj.draw(N, dev))
    out = {"plain_us": BR.event_us(plain, reps), "none_us": BR.event_us(lambda: jittered(none), reps), "jitter_us": BR.event_us(lambda: jittered(table), reps),
           "draw_us": BR.event_us(draw, reps)}
    out = {k: round(v, 2) for k, v in out.items()}
    out["crop_bytes"] = N * S * S * 3
    out["launches"] = {"plain": count_kernels(plain), "jitter": count_kernels(lambda: jittered(table)), "draw": count_kernels(draw)}
    return out


def make_leg(bench, bargs, dev, sample, color_jitter):
    from facialmmt_amd.config import default_args
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, step_parameters
    cfg = default_args(get_vision_utt_max_lens=BR.LV, trg_accumulation_steps=1)
    swin, mm = bench.build_models(bargs, dev, cfg)
    masters = MasterWeights(mm.roberta, torch.bfloat16)
    params = step_parameters(mm, masters)
    flat = GradientAverager(params, hooks=False)
    opt = HFAdamW(params, lr=torch.tensor(cfg.trg_lr, device=dev), weight_decay=cfg.weight_decay)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(1.0, (s + 1) / 100.0))
    return GraphedTargetStep(swin, mm, opt, sched, cfg, sample, autocast_dtype=torch.bfloat16, averager=flat, masters=masters, color_jitter=color_jitter)


def main():
    a = parse()
    assert torch.cuda.is_available(), "bench_color_jitter.py needs an MI355X"
    from facialmmt_amd.augment import ColorJitter
    from facialmmt_amd.config import default_args
    dev = torch.device("cuda:0")
    res = {"metric": "color_jitter_cost", "pre_step": dict(pre_step(dev, a.size, a.reps), config=f"{N} crops {a.size}x{a.size} uint8, cv2 resize, bf16, inference form"),
           "device": torch.cuda.get_device_name(0)}
    if not a.skip_steps:
        bench, bargs = BR.bench_args()
        cfg = default_args(get_vision_utt_max_lens=BR.LV, trg_accumulation_steps=1)
        bs = [bench.synth_batch(bargs, dev, i, cfg) for i in range(2)]
        legs = {"default": make_leg(bench, bargs, dev, bs[0], None), "color_jitter": make_leg(bench, bargs, dev, bs[0], ColorJitter())}
        for _ in range(a.warmup):
            for leg in legs.values():
                leg(bs[0])
        rounds = []
        for r in range(a.rounds):                               # alternate, and swap who goes first: drift reaches both legs alike
            order = list(legs) if r % 2 == 0 else list(legs)[::-1]
            t = {name: BR.timed(legs[name], bs, a.steps) for name in order}
            rounds.append([t["default"], t["color_jitter"]])
        med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(2)]
        spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in range(2)]
        t0 = legs["color_jitter"].last_jitter.clone()
        legs["color_jitter"](bs[0])
        assert legs["default"].last_jitter is None and not torch.equal(t0, legs["color_jitter"].last_jitter)      # the jittered leg really jitters
        res["step"] = {"config": "bench.py headline batch: 4 utterances x 160 frames of 112x112 uint8 crops, bf16, RoBERTa-large, HF AdamW, GraphedTargetStep",
                       "steps_per_round": a.steps, "rounds_ms": [[round(x, 3) for x in r] for r in rounds], "default_ms": round(med[0], 3),
                       "color_jitter_ms": round(med[1], 3), "difference_ms": round(med[1] - med[0], 3), "spread_ms": [round(x, 3) for x in spread]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
