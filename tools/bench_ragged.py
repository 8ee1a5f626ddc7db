"""Target-task training step on RAGGED batches (bf16, 4 utterances, Lv = 160, uint8 112x112 crops in, RoBERTa-large, HF AdamW -- bench.py's headline
geometry with MELD-like frame counts instead of 160 everywhere), two legs in ONE process and ONE call, alternating:
  (a) train_step.GraphedTargetStep(frame_capacity=640) on the batches as the loader pads them, (4, 160, 112, 112, 3) + num_imgs: one capture, Swin runs
      on all 640 slots whatever the counts are;
  (b) the eager train_step.TargetStep on the same batches compacted to (sum num_imgs, 112, 112, 3) -- the only way to train on such batches before
      frame_capacity existed.  The compaction itself is done outside the timed window (in favour of (b)).
num_imgs is drawn once from a fixed seed: every utterance uniform in [8, 160], one utterance per batch full (Lv is the loader's mean + 3 sigma cap: most
utterances are far shorter).  Each leg owns models with the same initial values.  Inputs stay on the device; wall clock between device synchronisations,
`--rounds` alternating rounds of `--steps` steps, the median round reported with the spread over rounds.  Also timed alone (device events, mean over
`--reps` back-to-back launches after a warm-up, straight through the C ABI): fmmt_pack_frames of one batch, and the head's BatchNorm1d (640 x 512, bf16) forward + backward launch
pair unmasked against masked (n_valid = 640 and the batch's real count).  Prints one JSON line.

    python tools/bench_ragged.py [--steps 16] [--warmup 3] [--rounds 3] [--batches 8]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

UTTS, LV, CAP = 4, 160, 640


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16, help="timed steps per round and leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="the legs alternate this many times; the median round is reported")
    ap.add_argument("--batches", type=int, default=8, help="distinct batches (frame counts) the steps cycle through")
    ap.add_argument("--reps", type=int, default=200, help="launches per single-op timing")
    ap.add_argument("--seed", type=int, default=20240)
    return ap.parse_args()


def frame_counts(n_batches, seed):
    """(n_batches, UTTS) frame counts: uniform in [8, LV], one utterance per batch full"""
    rng = np.random.RandomState(seed)
    n = rng.randint(8, LV + 1, size=(n_batches, UTTS))
    n[np.arange(n_batches), rng.randint(0, UTTS, size=n_batches)] = LV
    return n.tolist()


def bench_args():
    """bench.py's own defaults (the headline configuration), without reading this script's command line"""
    import bench
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        return bench, bench.parse()
    finally:
        sys.argv = argv


def make_batches(bench, bargs, dev, cfg, counts):
    """[(padded batch, compact batch)]: one synthetic batch per entry of `counts`, every frame slot holding data"""
    out = []
    for i, n in enumerate(counts):
        b = list(bench.synth_batch(bargs, dev, i, cfg))
        frames = b[8].view(UTTS, LV, *b[8].shape[1:])
        vmask = torch.zeros(UTTS, LV, device=dev)
        for u, k in enumerate(n):
            vmask[u, :k] = 1
        b[6] = vmask
        padded, compact = list(b), list(b)
        padded[8], padded[9] = frames, torch.tensor(n, device=dev)
        compact[8] = torch.cat([frames[u, :k] for u, k in enumerate(n)], dim=0).contiguous()
        compact[9] = torch.tensor(n, device=dev)
        out.append((tuple(padded), tuple(compact)))
    return out


def make_leg(name, bench, bargs, dev, sample):
    from facialmmt_amd.config import default_args
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, TargetStep, step_parameters
    cfg = default_args(get_vision_utt_max_lens=LV, trg_accumulation_steps=1)
    swin, mm = bench.build_models(bargs, dev, cfg)
    lr_of = lambda s: min(1.0, (s + 1) / 100.0)
    if name == "graphed":
        masters = MasterWeights(mm.roberta, torch.bfloat16)
        params = step_parameters(mm, masters)
        flat = GradientAverager(params, hooks=False)
        opt = HFAdamW(params, lr=torch.tensor(cfg.trg_lr, device=dev), weight_decay=cfg.weight_decay)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_of)
        return GraphedTargetStep(swin, mm, opt, sched, cfg, sample, autocast_dtype=torch.bfloat16, averager=flat, masters=masters, frame_capacity=CAP)
    opt = HFAdamW(mm.parameters(), lr=cfg.trg_lr, weight_decay=cfg.weight_decay)
    return TargetStep(swin, mm, opt, torch.optim.lr_scheduler.LambdaLR(opt, lr_of), cfg, autocast_dtype=torch.bfloat16)


def timed(fn, bs, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(bs[i % len(bs)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def event_us(fn, reps):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def single_ops(dev, padded, reps):
    """us per call, straight through the C ABI on preallocated buffers (the same host cost on every side): fmmt_pack_frames of one loader batch;
    BatchNorm1d forward + backward of the 640 x 512 bf16 head, unmasked / masked"""
    from facialmmt_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    frames, num_imgs = padded[8].contiguous(), padded[9].to(torch.int64)
    n_real, row_bytes = int(num_imgs.sum()), frames[0, 0].numel() * frames.element_size()
    packed = torch.empty((CAP,) + tuple(frames.shape[2:]), dtype=frames.dtype, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)

    def pack():
        _lib.check(lib.fmmt_pack_frames(UTTS, LV, CAP, row_bytes, frames.data_ptr(), num_imgs.data_ptr(), packed.data_ptr(), counts.data_ptr(), st), "fmmt_pack_frames")
    out = {"pack_frames_us": round(event_us(pack, reps), 2), "pack_frames_bytes_moved": (CAP + n_real) * row_bytes}
    out["pack_frames_GBps"] = round(out["pack_frames_bytes_moved"] / out["pack_frames_us"] / 1e3, 1)
    x = torch.randn(CAP, 512, device=dev).to(torch.bfloat16)
    dy = torch.randn(CAP, 512, device=dev).to(torch.bfloat16)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    g, b = torch.ones(512, device=dev), torch.zeros(512, device=dev)
    rm, rv = torch.zeros(512, device=dev), torch.ones(512, device=dev)
    sm, si, dg, db = (torch.empty(512, device=dev) for _ in range(4))
    P = lambda t: t.data_ptr()

    def plain():
        _lib.check(lib.fmmt_batchnorm1d_fwd(_lib.BF16, CAP, 512, P(x), P(g), P(b), P(rm), P(rv), 0.1, 1e-5, 1, P(y), P(sm), P(si), st), "bn fwd")
        _lib.check(lib.fmmt_batchnorm1d_bwd(_lib.BF16, CAP, 512, P(dy), P(x), P(g), P(sm), P(si), 1, P(dx), P(dg), P(db), st), "bn bwd")

    def masked(n):
        nv = torch.tensor([n], dtype=torch.int32, device=dev)

        def run():
            _lib.check(lib.fmmt_batchnorm1d_fwd_n(_lib.BF16, CAP, 512, P(nv), P(x), P(g), P(b), P(rm), P(rv), 0.1, 1e-5, 1, P(y), P(sm), P(si), st), "bn fwd_n")
            _lib.check(lib.fmmt_batchnorm1d_bwd_n(_lib.BF16, CAP, 512, P(nv), P(dy), P(x), P(g), P(sm), P(si), 1, P(dx), P(dg), P(db), st), "bn bwd_n")
        return run
    out["bn_fwd_bwd_unmasked_us"] = round(event_us(plain, reps), 2)
    out["bn_fwd_bwd_masked_full_us"] = round(event_us(masked(CAP), reps), 2)
    out["bn_fwd_bwd_masked_real_us"] = round(event_us(masked(n_real), reps), 2)
    out["bn_fwd_bwd_unmasked_again_us"] = round(event_us(plain, reps), 2)      # the spread of the method
    out["bn_masked_real_rows"] = n_real
    return out


def main():
    a = parse()
    assert torch.cuda.is_available(), "bench_ragged.py needs an MI355X"
    dev = torch.device("cuda:0")
    bench, bargs = bench_args()
    from facialmmt_amd.config import default_args
    counts = frame_counts(a.batches, a.seed)
    pairs = make_batches(bench, bargs, dev, default_args(get_vision_utt_max_lens=LV, trg_accumulation_steps=1), counts)
    padded, compact = [p for p, _ in pairs], [c for _, c in pairs]
    legs = {"graphed": (make_leg("graphed", bench, bargs, dev, padded[0]), padded), "eager": (make_leg("eager", bench, bargs, dev, None), compact)}
    for leg, bs in legs.values():
        for i in range(max(a.warmup, len(bs))):                 # every shape the timed window uses (the eager leg sees a new frame count per batch)
            leg(bs[i % len(bs)])
    rounds = []
    for _ in range(a.rounds):                                   # alternate: clock and thermal drift reach both legs alike
        rounds.append([timed(*legs[name], a.steps) for name in ("graphed", "eager")])
    seen = legs["graphed"][0].frame_counts.tolist()
    med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(2)]
    spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in range(2)]
    ops_us = single_ops(dev, padded[0], a.reps)
    n_valid = [sum(n) for n in counts]
    print(json.dumps({"metric": "ragged_target_step_ms",
                      "config": f"bf16, {UTTS} utterances, Lv = {LV}, uint8 112x112 crops, roberta-large, HF AdamW, accumulation 1; num_imgs uniform in [8, {LV}] with one "
                                f"full utterance per batch, seed {a.seed}", "steps_per_round": a.steps, "num_imgs": counts, "n_valid_per_step": n_valid,
                      "mean_n_valid": round(sum(n_valid) / len(n_valid), 1), "frame_capacity": CAP, "last_frame_counts": seen,
                      "legs": ["GraphedTargetStep(frame_capacity=640), padded batches", "eager TargetStep, compact batches"],
                      "rounds_ms": [[round(x, 3) for x in r] for r in rounds], "graphed_ragged_ms": round(med[0], 3), "eager_compact_ms": round(med[1], 3),
                      "spread_ms": [round(x, 3) for x in spread], "eager_over_graphed": round(med[1] / med[0], 3), **ops_us,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
