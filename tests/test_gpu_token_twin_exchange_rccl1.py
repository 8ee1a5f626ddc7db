"""A PADDED TWIN UNDER A GRADIENT EXCHANGE, on one GPU: GraphedTargetStep with token packing on (train_step PACK_NOTE) and an active averager -- backend
nccl (= RCCL) at world size 1 with GradientAverager(always=True, hooks=False, bucket_mb=1), the route of tests/test_gpu_rank_buckets_rccl1.py.  Every
forward/backward capture is then a pair (A1, A2) and the twin is a pair of its own: a call whose text mask has a hole must replay the twin's A1, issue
the exchange, and replay the TWIN's A2 -- the packed pair's A2 would run Swin's backward from the activations of another forward.

The tiny models of tests/test_gpu_token_packing.py::_step (B = 2, Lv = 6, frame_capacity 12, two-layer bf16 RoBERTa under MasterWeights, SGD); three
calls -- packed, a mask with one hole, packed again -- against the same calls of the step built WITHOUT an averager (one graph per capture, no
collective).  fp32 on the wire at world size 1 leaves the gradients as they are, so the two sides differ only in where the graph is cut; the bars are
that file's: loss to 2e-4 x max(1, |loss|), equal kept-frame masks, the parameter sample to 1e-4 x max(1, max|p|).  One spawned process runs both
sides; results travel through a file."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from tests.test_gpu_token_packing import CAP, _sample, _step
    out = {}
    for exchange in (False, True):
        step, mm, masters, batch = _step(dev, None, exchange=exchange)
        assert step.split == exchange and step.token_capacity > 0 and sorted(step._captures) == [(CAP, False), (CAP, True)]
        packed, twin = step._captures[CAP, True], step._captures[CAP, False]
        assert packed.a1 is step.graph_a and packed.a2 is step.graph_a2 and twin.a1 is not packed.a1
        assert (packed.a2 is not None) == exchange and (twin.a2 is not None) == exchange
        holed_mask = batch[1].clone()
        holed_mask[0, 3] = 0
        losses, kept, replayed = [], [], []
        for b in (batch, batch[:1] + (holed_mask,) + batch[2:], batch):
            loss, k = step(b)
            losses.append(float(loss))
            kept.append(k.cpu().clone())
            replayed.append([key for key, r in step._captures.items() if r.loss is step.loss and r.mask is step.new_mask])
        torch.cuda.synchronize()
        assert replayed == [[(CAP, True)], [(CAP, False)], [(CAP, True)]], replayed
        if exchange:                                                             # the holed batch ran the twin's own second piece
            a2 = step._captures[replayed[1][0]].a2
            assert a2 is not None and a2 is not packed.a2
        out[exchange] = dict(losses=losses, kept=kept, token_replays=dict(step.token_replays), replays=dict(step.replays),
                             params={k: v.cpu() for k, v in _sample(mm, masters).items()}, buckets=len(step.flat.buckets))
    torch.save(out, os.path.join(out_dir, "token_twin_exchange.pt"))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("token_twin_exchange"))
    mp.spawn(_worker, args=(_free_port(), d), nprocs=1, join=True)
    return torch.load(os.path.join(d, "token_twin_exchange.pt"), weights_only=False)


def test_padded_twin_under_the_exchange_follows_the_single_graph_twin(runs):
    ref, got = runs[False], runs[True]
    print("losses reference", ref["losses"])
    print("losses exchange ", got["losses"])
    worst = max(((got["params"][k] - ref["params"][k]).abs().max().item() / max(1.0, ref["params"][k].abs().max().item()), k) for k in ref["params"])
    print(f"parameters after three updates: worst {worst[1]} {worst[0]:.3e} of max(1, max|p|)")
    assert got["buckets"] >= 2                                                   # several collectives between A1 and A2
    for side in (ref, got):
        assert side["token_replays"] == {"packed": 2, "padded": 1} and side["replays"] == {12: 3}
    assert ref["losses"][0] != ref["losses"][-1]                                 # the optimiser moved something
    for a, b in zip(ref["losses"], got["losses"]):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (ref["losses"], got["losses"])
    for a, b in zip(ref["kept"], got["kept"]):
        assert torch.equal(a, b) and float(a.sum()) > 0
    assert worst[0] <= 1e-4, worst
