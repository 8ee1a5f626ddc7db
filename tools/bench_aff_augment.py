"""What the on-device Aff-Wild2 augmentation of the auxiliary step costs, in ONE process and ONE call (same-call A/B):
  1. the fused uint8 pre-step alone at the benchmark's auxiliary batch (150 crops of 112 x 112, bf16, 'pil' resize, inference form: no patch matrix
     written), device events over back-to-back launches straight through the C ABI on preallocated buffers:
       plain     fmmt_patch_embed_u8_ln_fwd                              (one launch; the kernel every earlier commit has)
       off       fmmt_patch_embed_u8_aug_ln_fwd, every stage off         (three launches; the statistic's launch leaves at once)
       drawn     the same on a table AffWildAugment().draw made           (the reference's probabilities: 0.8 / 0.2 / 0.5 / 0.25)
       all       the same with every stage on in every frame             (grayscale, four jitter operations, blur at r = 1, a rectangle)
       draw      augment.AffWildAugment.draw(150) into a static table    (the launches a captured step adds in front of Swin)
  2. train_step.GraphedAuxStep on that batch (bf16 autocast of the model's own dtype, HF AdamW), with and without augment=AffWildAugment(), each leg
     over a model of its own with the same initial values, alternating rounds, wall clock between device synchronisations, the median round reported
     with the spread over rounds.
  3. (--host) the same chain with Pillow on ONE core of the machine this runs on, per image: a CPU figure, for scale.
Launches are counted with torch.profiler over one eager call.  Prints one JSON line.

    python tools/bench_aff_augment.py [--steps 16] [--warmup 3] [--rounds 5] [--reps 200] [--host]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, S = 150, 112


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16, help="timed steps per round and leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--reps", type=int, default=200, help="launches per single-op timing")
    ap.add_argument("--skip-steps", action="store_true", help="part 1 only")
    ap.add_argument("--host", action="store_true", help="part 3 only: Pillow on one core (needs no GPU)")
    return ap.parse_args()


def host_chain_ms(images=40):
    """the reference's chain per image with Pillow and numpy on one core: Resize(224, BICUBIC), Grayscale / ColorJitter / GaussianBlur at the
    reference's probabilities, ToTensor / Normalize, RandomErasing"""
    import random

    import numpy as np
    from PIL import Image, ImageEnhance, ImageFilter
    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    crops = [Image.fromarray(rng.integers(0, 256, (S, S, 3), dtype=np.uint8), "RGB") for _ in range(images)]
    random.seed(0)
    t0 = time.perf_counter()
    for im in crops:
        im = im.resize((224, 224), Image.BICUBIC)
        if random.random() < 0.8:
            im = im.convert("L").convert("RGB")
        if random.random() < 0.2:
            ops = [lambda i: ImageEnhance.Brightness(i).enhance(random.uniform(0.6, 1.4)), lambda i: ImageEnhance.Contrast(i).enhance(random.uniform(0.6, 1.4)),
                   lambda i: ImageEnhance.Color(i).enhance(random.uniform(0.6, 1.4))]

            def hue(i):
                h, s, v = i.convert("HSV").split()
                a = np.array(h, dtype=np.uint8)
                with np.errstate(over="ignore"):
                    a += np.uint8(int(random.uniform(-0.4, 0.4) * 255) % 256)
                return Image.merge("HSV", (Image.fromarray(a, "L"), s, v)).convert("RGB")
            ops.append(hue)
            random.shuffle(ops)
            for op in ops:
                im = op(im)
        if random.random() < 0.5:
            im = im.filter(ImageFilter.GaussianBlur(radius=random.uniform(0.1, 2.0)))
        t = (torch.from_numpy(np.array(im)).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5
        if random.random() < 0.25:
            h, w = random.randint(17, 120), random.randint(17, 120)
            top, left = random.randint(0, 224 - h), random.randint(0, 224 - w)
            t[:, top:top + h, left:left + w] = torch.empty(3, h, w).normal_()
    return (time.perf_counter() - t0) * 1e3 / images


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def kernel_shares(fn, reps=20):
    """device time per kernel name over `reps` calls, from one profiler trace: {name prefix: us per call}"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            key = next((k for k in ("jitter_stats_kernel", "aug_pixels_kernel", "aug_finish_kernel") if k in e.name), e.name[:40])
            out[key] = out.get(key, 0.0) + e.device_time / reps
    return {k: round(v, 2) for k, v in out.items()}


def pre_step(dev, reps):
    from facialmmt_amd import _lib, ops, synth
    from facialmmt_amd.augment import AffWildAugment, ColorJitter
    from facialmmt_amd.modules.SwinTransformer import Swin_Transformer as SW
    from tools import bench_ragged as BR
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randint(0, 256, (N, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
    pe = SW.PatchEmbed(224, 4, 3, 96, torch.nn.LayerNorm)
    synth.fill_state_dict(pe, seed=31, prefix="pe.")
    pe.to(dev)
    code, tab, lut = ops.resize_tables("pil", S, dev)
    w = pe.proj.weight.detach().view(96, 48).to(torch.bfloat16).contiguous()
    bias, gam, bet = pe.proj.bias.detach().float(), pe.norm.weight.detach().float(), pe.norm.bias.detach().float()
    y = torch.empty(N * 3136, 96, dtype=torch.bfloat16, device=dev)
    partial = torch.empty(N, _lib.JITTER_BANDS, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.fmmt_aug_workspace_bytes(N), dtype=torch.uint8, device=dev)
    aug = AffWildAugment()
    torch.manual_seed(3)
    drawn = aug.draw(N, dev)
    off = AffWildAugment(grayscale_p=0, jitter_p=0, blur_p=0, erase_p=0).draw(N, dev)
    every = AffWildAugment.table([True] * N, jitter=ColorJitter(0.4, 0.4, 0.4, 0.4).draw(N, "cpu"), sigma=[2.0] * N, rect=[[10, 20, 100, 120]] * N,
                                 key=[[i, 7] for i in range(N)], device=dev)
    P = lambda t: t.data_ptr()

    def plain():
        _lib.check(lib.fmmt_patch_embed_u8_ln_fwd(_lib.BF16, code, N, S, P(x), P(tab), P(lut), P(w), P(bias), P(gam), P(bet), 1e-5, None, None, P(y), None, None, st), "plain")

    def augmented(t):
        _lib.check(lib.fmmt_patch_embed_u8_aug_ln_fwd(_lib.BF16, code, N, S, P(x), P(tab), P(lut), P(t), P(partial), P(ws), ws.numel(), P(w), P(bias), P(gam),
                                                      P(bet), 1e-5, None, None, P(y), None, None, st), "augmented")
    static = torch.empty_like(drawn)

    def draw():
        static.copy_(aug.draw(N, dev))
    out = {}
    for _ in range(2):                                          # alternating: plain, off, drawn, all, and again
        for name, fn in (("plain_us", plain), ("off_us", lambda: augmented(off)), ("drawn_us", lambda: augmented(drawn)), ("all_us", lambda: augmented(every))):
            out.setdefault(name, []).append(round(BR.event_us(fn, reps), 2))
    out["draw_us"] = round(BR.event_us(draw, reps), 2)
    out["workspace_bytes"], out["crop_bytes"] = ws.numel(), N * S * S * 3
    out["launches"] = {"plain": count_kernels(plain), "augmented": count_kernels(lambda: augmented(drawn)), "draw": count_kernels(draw)}
    out["kernel_us"] = {"drawn": kernel_shares(lambda: augmented(drawn)), "all": kernel_shares(lambda: augmented(every))}
    return out


def make_leg(bench, bargs, dev, sample, augment):
    from facialmmt_amd.config import default_args
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedAuxStep, HFAdamW
    cfg = default_args(trg_accumulation_steps=1)
    swin, _ = bench.build_models(bargs, dev, cfg)
    flat = GradientAverager(swin.parameters(), hooks=False)
    opt = HFAdamW(swin.parameters(), lr=torch.tensor(cfg.aux_lr, device=dev))
    kw = {} if augment is None else {"augment": augment}
    return GraphedAuxStep(swin, opt, None, cfg, *sample, averager=flat, **kw)


def main():
    a = parse()
    if a.host:
        import PIL
        print(json.dumps({"metric": "aff_augment_host_chain", "ms_per_image_one_core": round(host_chain_ms(), 2), "pillow": PIL.__version__,
                          "note": "CPU figure: Pillow + torch on one core of the machine this ran on"}))
        return
    assert torch.cuda.is_available(), "bench_aff_augment.py needs an MI355X"
    from facialmmt_amd.augment import AffWildAugment
    from tools import bench_ragged as BR
    dev = torch.device("cuda:0")
    res = {"metric": "aff_augment_cost", "pre_step": dict(pre_step(dev, a.reps), config=f"{N} crops {S}x{S} uint8, pil resize, bf16, inference form"),
           "device": torch.cuda.get_device_name(0)}
    if not a.skip_steps:
        bench, bargs = BR.bench_args()
        bargs.aux_images = N
        bs = [bench.synth_aux_batch(bargs, dev, i) for i in range(2)]
        legs = {"default": make_leg(bench, bargs, dev, bs[0], None), "augment": make_leg(bench, bargs, dev, bs[0], AffWildAugment())}
        call = {name: (lambda b, leg=leg: leg(*b)) for name, leg in legs.items()}
        for _ in range(a.warmup):
            for fn in call.values():
                fn(bs[0])
        rounds = []
        for r in range(a.rounds):                               # alternate, and swap who goes first: drift reaches both legs alike
            order = list(legs) if r % 2 == 0 else list(legs)[::-1]
            t = {name: BR.timed(call[name], bs, a.steps) for name in order}
            rounds.append([t["default"], t["augment"]])
        med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(2)]
        spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in range(2)]
        t0 = legs["augment"].last_augment.clone()
        legs["augment"](*bs[0])
        assert legs["default"].last_augment is None and not torch.equal(t0, legs["augment"].last_augment)       # the augmented leg really augments
        res["step"] = {"config": f"bench.py's auxiliary batch: {N} crops of {S}x{S} uint8, {bargs.dtype}, HF AdamW, GraphedAuxStep",
                       "steps_per_round": a.steps, "rounds_ms": [[round(x, 3) for x in r] for r in rounds], "default_ms": round(med[0], 3),
                       "augment_ms": round(med[1], 3), "difference_ms": round(med[1] - med[0], 3), "spread_ms": [round(x, 3) for x in spread]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
