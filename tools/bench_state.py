"""Wall time and file size of saving and resuming the benchmark's training step: bench.py's headline configuration (bf16, 4 utterances, Lv = 160, uint8
112x112 crops, RoBERTa-large in bf16 with fp32 masters, HF AdamW through the fused update, the target step as HIP graphs), a few steps, then
  save:   step.state_dict() + checkpoint.save_training(file)         (device -> host tensor by tensor, then torch.save)
  resume: checkpoint.load_training(file) + step.load_state_dict()    (torch.load with weights_only=True, then host -> device in place)
each timed once between device synchronisations, and one more step behind the load.  Nothing is compared here (tests/test_gpu_step_state.py holds the
resumed run to the uninterrupted one's bits); the numbers have no bar.  Prints one JSON line.

    python tools/bench_state.py [--steps 3] [--dir DIR] [--time-limit 600]

--dir: where the file is written (default: a temporary directory, removed afterwards); --time-limit: the process ends itself (stack traces on stderr,
exit status 1) when the whole run takes longer."""
import argparse
import faulthandler
import json
import os
import sys
import tempfile
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="training steps in front of the save")
    ap.add_argument("--dir", default=None, help="directory for the file (default: a temporary one)")
    ap.add_argument("--time-limit", type=int, default=600, help="seconds after which the process ends itself")
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.time_limit, exit=True)
    assert torch.cuda.is_available(), "bench_state.py needs an MI355X"
    import bench_ragged
    from facialmmt_amd import checkpoint
    from facialmmt_amd.config import default_args
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, step_parameters
    bench, bargs = bench_ragged.bench_args()
    dev = torch.device("cuda:0")
    cfg = default_args(get_vision_utt_max_lens=bargs.frames, trg_accumulation_steps=1)
    swin, mm = bench.build_models(bargs, dev, cfg)
    batch = bench.synth_batch(bargs, dev, 0, cfg)
    masters = MasterWeights(mm.roberta if mm.text_pretrained_model == "roberta" else mm.bert, torch.bfloat16)
    params = step_parameters(mm, masters)
    opt = HFAdamW(params, lr=torch.tensor(cfg.trg_lr, device=dev), weight_decay=cfg.weight_decay)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(1.0, (s + 1) / 100.0))
    step = GraphedTargetStep(swin, mm, opt, sched, cfg, batch, autocast_dtype=torch.bfloat16, averager=GradientAverager(params, hooks=False), masters=masters)
    assert step.fused is not None
    for _ in range(a.steps):
        loss, _ = step(batch)
    torch.cuda.synchronize()
    before = float(loss)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        path = os.path.join(d, "run.pt")
        t0 = time.perf_counter()
        state = step.state_dict()
        t1 = time.perf_counter()
        checkpoint.save_training(path, extra={"epoch": 0}, target=state)
        t2 = time.perf_counter()
        size = os.path.getsize(path)
        tensors = sum(t.numel() * t.element_size() for part in (state["models"]["swin"], state["models"]["mm"]) for t in part.values())
        moments = sum(s[k].numel() * 4 for s in state["optimizer"]["state"].values() for k in ("exp_avg", "exp_avg_sq"))
        del state
        t3 = time.perf_counter()
        states, extra = checkpoint.load_training(path)
        t4 = time.perf_counter()
        step.load_state_dict(states["target"])
        torch.cuda.synchronize()
        t5 = time.perf_counter()
    loss, _ = step(batch)
    torch.cuda.synchronize()
    assert extra == {"epoch": 0} and torch.isfinite(loss) and not step.opt.state
    print(json.dumps({
        "metric": "save_resume_seconds",
        "config": f"bf16, {bargs.utts} utterances, Lv = {bargs.frames}, roberta-large with fp32 masters, HF AdamW (fused), GraphedTargetStep; saved after {a.steps} steps",
        "state_dict_s": round(t1 - t0, 3), "save_training_s": round(t2 - t1, 3), "save_s": round(t2 - t0, 3),
        "load_training_s": round(t4 - t3, 3), "load_state_dict_s": round(t5 - t4, 3), "resume_s": round(t5 - t3, 3),
        "file_bytes": size, "model_bytes": tensors, "moment_bytes": moments, "optimizer_parameters": len(params),
        "loss_before_save": before, "loss_behind_load": float(loss), "device": torch.cuda.get_device_name(0)}))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
