"""An evaluation split SHARDED over ranks: two spawned processes sharing the one GPU of the test box on gloo (RCCL refuses two ranks per device; the RCCL
variant needs two GPUs), the construction of tests/test_gpu_ddp_ragged.py -- mp.spawn, results through files, a 120 s process-group timeout.

Scenario 1: a split of 9 rows at B = 2.  parallel.eval_shard gives rank 0 rows [0, 6) and rank 1 rows [6, 9), so rank 1 ends in a short batch, which
GraphedEvalStep(frame_capacity=(8, 12), pad_rows=True) replays padded.  evaluate(sharded=True) gathers and merges: both ranks hold the same bits, and
against the single-process evaluate() of the whole split with the same step configuration results, truths, count and confusion are EQUAL -- the batches
are the same batches -- while avg_loss agrees to 1e-12 relative: the loss sum is (sum of rank 0's batches) + (sum of rank 1's) against one running sum,
another association of fewer than 10^4 fp64 terms, n * eps.  Scenario 2 (same spawn): 2 rows, so rank 1's shard is empty and it runs no batch.
One more spawn of ONE process on backend nccl at world size 1 (the route of tests/test_gpu_rank_buckets_rccl1.py): evaluate(sharded=True) == evaluate()."""
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import support_eval_pad as SP

pytestmark = pytest.mark.gpu

B, NL, BUCKETS = SP.B, SP.NL, SP.BUCKETS
COUNTS = ([5, 2], [6, 6], [1, 3], [4, 4], [3])                  # 9 rows in 5 batches, the last short
RCCL = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one device per rank: two GPUs")
BACKENDS = ["gloo", pytest.param("nccl", marks=RCCL)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port, backend):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", rank if backend == "nccl" and world > 1 else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=timedelta(seconds=120), **({"device_id": dev} if backend == "nccl" else {}))
    return dev


def _step(dev, models, sample, collect_rows):
    from facialmmt_amd.eval_step import GraphedEvalStep, MeldMetrics
    swin, mm, cfg = models
    return GraphedEvalStep(swin, mm, cfg, sample, autocast_dtype=None, gumbel="off", frame_capacity=BUCKETS, pad_rows=True,
                           metrics=MeldMetrics(NL, dev, collect_rows=collect_rows))


def _record(step, out):
    loss, results, truths = out
    m = step.metrics
    return dict(loss=loss, results=results.cpu(), truths=truths.cpu(), own=m.result(), own_cursor=int(m.cursor.item()),
                merged=None if m.merged is None else m.merged.result(), merged_words=None if m.merged is None else m.merged.words.cpu(),
                counters=(step.replays, step.fallbacks, step.padded_calls))


def _worker(rank, world, port, out_dir, backend):
    dev = _init(rank, world, port, backend)
    from facialmmt_amd import parallel
    from facialmmt_amd.eval_step import evaluate
    models = SP.build(dev)                                      # the same weights on every rank, from the seeds
    out = {}
    for name, counts in (("nine", COUNTS), ("two", COUNTS[:1])):
        batches = SP.split(dev, models[2], counts, 300)
        n = sum(len(c) for c in counts)
        shard = parallel.eval_shard(n, B)                       # rank and world of the process group
        mine = batches[shard.start // B:(shard.stop + B - 1) // B] if len(shard) else []
        assert sum(len(x[7]) for x in mine) == len(shard)
        step = _step(dev, models, batches[0], parallel.eval_collect_rows(n, B, world))
        out[name] = _record(step, evaluate(step, mine, sharded=True))
        out[name]["shard"] = (shard.start, shard.stop)
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.fixture(scope="module", params=BACKENDS)
def runs(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("eval_sharded"))
    mp.spawn(_worker, args=(2, _free_port(), d, request.param), nprocs=2, join=True)
    return [torch.load(os.path.join(d, f"rank{r}.pt"), weights_only=False) for r in range(2)]


@pytest.fixture(scope="module")
def single():
    """the whole split in this process, one rank, the same step configuration"""
    from facialmmt_amd.eval_step import evaluate
    dev = torch.device("cuda:0")
    models = SP.build(dev)
    out = {}
    for name, counts in (("nine", COUNTS), ("two", COUNTS[:1])):
        batches = SP.split(dev, models[2], counts, 300)
        step = _step(dev, models, batches[0], 2 * len(batches))
        out[name] = _record(step, evaluate(step, batches))
    return out


def _same(a, b):
    return a["loss"] == b["loss"] and torch.equal(a["results"], b["results"]) and torch.equal(a["truths"], b["truths"]) and \
        torch.equal(a["merged_words"], b["merged_words"])


def test_two_ranks_merge_to_the_split_one_rank_evaluates(runs, single):
    from facialmmt_amd.eval_step import eval_meld
    r0, r1, one = runs[0]["nine"], runs[1]["nine"], single["nine"]
    assert r0["shard"] == (0, 6) and r1["shard"] == (6, 9)
    assert r0["counters"] == (3, 0, 0) and r1["counters"] == (2, 0, 1)          # rank 1 ends short: a padded replay, no fallback
    assert r0["own"].count == 6 and r1["own"].count == 3 and (r0["own_cursor"], r1["own_cursor"]) == (6, 3)     # step.metrics stays the rank's own
    assert _same(r0, r1)                                                        # bit-identical on both ranks
    assert r0["results"].shape == (9, NL) and int(r0["merged_words"][-1]) == 9
    assert torch.equal(r0["results"], one["results"]) and torch.equal(r0["truths"], one["truths"])
    assert r0["merged"].count == one["own"].count == 9 and np.array_equal(r0["merged"].confusion, one["own"].confusion)
    rel = abs(r0["loss"] - one["loss"]) / abs(one["loss"])
    print(f"avg_loss sharded {r0['loss']!r} against one rank {one['loss']!r}: rel {rel:.2e}")
    assert rel <= 1e-12
    assert r0["merged"].loss_sum == r0["own"].loss_sum + r1["own"].loss_sum     # the ranks' doubles in rank order
    assert r0["merged"].weighted_f1 == eval_meld(r0["results"], r0["truths"])


def test_an_empty_shard_runs_no_batch_and_gets_the_merged_split(runs, single):
    r0, r1, one = runs[0]["two"], runs[1]["two"], single["two"]
    assert r0["shard"] == (0, 2) and r1["shard"][1] - r1["shard"][0] <= 0
    assert r0["counters"] == (1, 0, 0) and r1["counters"] == (0, 0, 0) and r1["own"].count == 0 and r1["own_cursor"] == 0
    assert _same(r0, r1) and r1["results"].shape == (2, NL) and r1["merged"].count == 2
    assert torch.equal(r1["results"], one["results"]) and torch.equal(r1["truths"], one["truths"]) and r1["loss"] == one["loss"]


def _worker_rccl1(rank, port, out_dir):
    dev = _init(0, 1, port, "nccl")
    from facialmmt_amd.eval_step import evaluate
    models = SP.build(dev)
    batches = SP.split(dev, models[2], COUNTS, 300)
    step = _step(dev, models, batches[0], 10)
    plain = _record(step, tuple(t.clone() if torch.is_tensor(t) else t for t in evaluate(step, batches)))
    plain["words"] = step.metrics.words.cpu()
    sharded = _record(step, evaluate(step, batches, sharded=True))
    sharded["words"] = step.metrics.words.cpu()
    torch.save(dict(plain=plain, sharded=sharded), os.path.join(out_dir, "rccl1.pt"))
    dist.destroy_process_group()


def test_rccl_world_size_one_sharded_equals_plain(tmp_path):
    mp.spawn(_worker_rccl1, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    got = torch.load(os.path.join(str(tmp_path), "rccl1.pt"), weights_only=False)
    plain, sharded = got["plain"], got["sharded"]
    assert plain["loss"] == sharded["loss"] and torch.equal(plain["results"], sharded["results"]) and torch.equal(plain["truths"], sharded["truths"])
    assert torch.equal(plain["words"], sharded["words"]) and torch.equal(sharded["merged_words"], sharded["words"])      # accumulators and cursor, bit for bit
    assert sharded["results"].shape == (9, NL) and sharded["counters"][1] == 0 and sharded["merged"].count == 9
