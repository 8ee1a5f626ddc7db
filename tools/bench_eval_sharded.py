"""A split that ends in a SHORT batch, and the gather-and-merge of a sharded split, at configs[1]'s geometry (4 utterances, Lv = 160, RoBERTa-large,
bf16; tools/bench_eval_ragged.py's set-up, frame counts and buckets), world size 1, three legs in ONE process and ONE call, alternating:
  (a) GraphedEvalStep(frame_capacity=(384, 512, 640), pad_rows=False): `--batches` full batches replay, the short last batch (2 of 4 utterances) takes
      the launch-by-launch fallback, EvalStep(frame_capacity=640);
  (b) the same with pad_rows=True: the short batch is padded to 4 rows and replayed in the bucket of its real frames, the captured metric update
      reads the row count from a device word (ops.eval_accumulate_rows);
  (c) leg (b)'s step through evaluate(sharded=True): the same batches, then MeldMetrics.gather_merge -- without a process group no collective, the
      merge kernel with W = 1 -- and results / truths from the merged buffers.  (c) - (b) is what gather-and-merge costs on one rank.
A "split" is one eval_step.evaluate() call, wall clock around it, the final copy of the accumulators included; `--rounds` alternating rounds, the median
reported.  No threshold is set on these times: they are reported against leg (a) of the same run.  A speed-up over several ranks is NOT measured here
or anywhere: no machine with two GPUs has been available to this project.  Prints one JSON line.

    python tools/bench_eval_sharded.py [--batches 40] [--warmup 1] [--rounds 5]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

SHORT_ROWS = 2


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=40, help="full batches per split (the eight frame-count patterns, cycled); one short batch follows")
    ap.add_argument("--warmup", type=int, default=1, help="untimed splits per leg")
    ap.add_argument("--rounds", type=int, default=5, help="the three legs alternate this many times; the median round is reported")
    return ap.parse_args()


def split_ms(step, batches, rows, sharded):
    from facialmmt_amd.eval_step import evaluate
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, results, truths = evaluate(step, batches, sharded=sharded)
    torch.cuda.synchronize()
    assert results.shape[0] == truths.shape[0] == rows
    return (time.perf_counter() - t0) * 1e3


def main():
    a = parse()
    assert torch.cuda.is_available(), "bench_eval_sharded.py needs an MI355X"
    import bench_eval_ragged as R
    from facialmmt_amd.eval_step import GraphedEvalStep, MeldMetrics
    args, dev, cfg, swin, mm, counts, padded, _, _ = R.setup()
    short = tuple(t[:SHORT_ROWS] for t in padded[0])
    split = [padded[i % len(padded)] for i in range(a.batches)] + [short]
    rows = a.batches * args.utts + SHORT_ROWS
    steps = {pad: GraphedEvalStep(swin, mm, cfg, padded[0], autocast_dtype=torch.bfloat16, gumbel="sample", frame_capacity=R.BUCKETS, pad_rows=pad,
                                  metrics=MeldMetrics(swin.num_labels, dev, collect_rows=rows)) for pad in (False, True)}
    legs = (("fallback", steps[False], False), ("pad_rows", steps[True], False), ("pad_rows_sharded", steps[True], True))
    for _ in range(a.warmup):
        for _, step, sharded in legs:
            split_ms(step, split, rows, sharded)
    for step in steps.values():
        step.replays = step.fallbacks = step.padded_calls = 0
    rounds = [[split_ms(step, split, rows, sharded) for _, step, sharded in legs] for _ in range(a.rounds)]     # alternate: drift reaches all legs alike
    med = [sorted(r[i] for r in rounds)[len(rounds) // 2] for i in range(len(legs))]
    merged = steps[True].metrics.merged.result()
    what = {"fallback": "GraphedEvalStep(frame_capacity=(384, 512, 640)): the short batch runs launch by launch through EvalStep(frame_capacity=640)",
            "pad_rows": "the same with pad_rows=True: the short batch is padded and replayed, eval_accumulate_rows counts its real rows",
            "pad_rows_sharded": "leg pad_rows through evaluate(sharded=True): + gather_merge (no collective at world size 1, eval_merge with W = 1)"}
    out = {"metric": "eval_sharded_ms_per_split", "world_size": 1,
           "config": f"{args.utts} utterances x Lv = {args.frames}, {args.plm}, bf16; {a.batches} full batches + one of {SHORT_ROWS} utterances per split",
           "rows_per_split": rows, "rounds": [[round(x, 3) for x in rr] for rr in rounds]}
    for i, (name, step, _) in enumerate(legs):
        out[name] = {"ms_per_split": round(med[i], 3), "ms_per_batch": round(med[i] / len(split), 3), "over_fallback": round(med[i] / med[0], 4), "what": what[name]}
    out["fallback"].update(replays=steps[False].replays, fallbacks=steps[False].fallbacks, padded_calls=steps[False].padded_calls)
    out["pad_rows"].update(replays=steps[True].replays, fallbacks=steps[True].fallbacks, padded_calls=steps[True].padded_calls,
                           note="counters of legs pad_rows and pad_rows_sharded together: they share the step")
    out["gather_merge_ms_per_split"] = round(med[2] - med[1], 3)
    out["rows_counted_merged"] = merged.count
    out["multi_rank_speedup"] = "not measured: no machine with two GPUs has been available"
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
