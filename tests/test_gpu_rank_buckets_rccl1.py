"""GraphedTargetStep(frame_capacity=(8, 12)) UNDER A GRADIENT EXCHANGE, on one GPU: backend nccl (= RCCL) at world size 1 with
GradientAverager(always=True), the route of tests/test_gpu_ddp.py::test_rccl_world_size_one_runs_the_exchange_path.  With an active averager the
forward/backward of every capacity is a pair of graphs (A1_c, A2_c) and every bucket goes through dist.all_reduce between them; the reference is the
same step WITHOUT an averager -- one graph A per capacity, no collective.  fp32 on the wire at world size 1 leaves the gradients as they are, so the
two sides differ only in where the graph is cut.

Shapes, sequence and tolerances are those of tests/test_gpu_ragged_buckets.py, restated and not imported: B = 2, Lv = 6, buckets (8, 12), fp32 compute,
tau = 1e5, threshold 0.1, DropPath and dropout off, stand-in text encoder, SGD at 0.05, every padded frame slot random; six micro-steps over
[3, 4] -> [6, 5] -> [2, 6] -> [6, 6] (cycled), accumulation 1 and 2; losses to 2e-4 relative, parameters and the BatchNorm running statistics to 1e-4
of scale, kept-frame masks equal.  One spawned process runs all four trajectories; results travel through a file."""
import os
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from facialmmt_amd import synth

pytestmark = pytest.mark.gpu

B, LV, BUCKETS = 2, 6, (8, 12)
SEQ = ([3, 4], [6, 5], [2, 6], [6, 6])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _models(dev, accumulation):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    cfg = default_args(get_vision_utt_max_lens=LV, get_audio_utt_max_lens=24, trg_accumulation_steps=accumulation, plm_module=synth.make_standin_plm(),
                       hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, crossmodal_attn_dropout_TA=0.0, crossmodal_attn_dropout_TA_V=0.0,
                       tau=1e5, FacialEmoImpor_threshold=0.1)
    cfg.compute_dtype = torch.float32
    swin = models.SwinForAffwildClassification(cfg)
    mm = models.MultiModalTransformerForClassification(cfg)
    synth.fill_state_dict(swin, seed=100)
    synth.fill_state_dict(mm, seed=200)
    for m in swin.modules():
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    swin.to(dev).train()
    mm.to(dev).train()
    return cfg, swin, mm


def _padded(dev, cfg, num_imgs):
    """the loader's batch for the given frame counts: frames (B, Lv, 3, 224, 224) with EVERY slot random, num_imgs as the reference's collate yields it"""
    import bench
    args = types.SimpleNamespace(utts=B, frames=LV, dtype="fp32", plm="roberta-large", input="float", resize="pil")
    batch = list(bench.synth_batch(args, dev, 0, cfg))
    batch[0] = batch[0] % 1000
    vmask = torch.zeros(B, LV, device=dev)
    for u, k in enumerate(num_imgs):
        vmask[u, :k] = 1
    batch[6] = vmask
    batch[8], batch[9] = batch[8].view(B, LV, 3, 224, 224), list(num_imgs)
    return tuple(batch)


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from facialmmt_amd.parallel import GradientAverager
    from facialmmt_amd.train_step import GraphedTargetStep
    out = {}
    for accumulation in (1, 2):
        for exchange in (False, True):
            cfg, swin, mm = _models(dev, accumulation)
            opt = torch.optim.SGD(mm.parameters(), lr=0.05)
            batches = [_padded(dev, cfg, n) for n in SEQ]
            avg = GradientAverager([p for p in mm.parameters() if p.requires_grad], hooks=False, bucket_mb=1, always=True) if exchange else None
            step = GraphedTargetStep(swin, mm, opt, None, cfg, batches[0], autocast_dtype=None, frame_capacity=BUCKETS, averager=avg)
            assert step.split == exchange and step.capacities == BUCKETS and step.replays == {8: 0, 12: 0}
            assert sorted(step._captures) == [(c, True) for c in BUCKETS] and all((r.a2 is not None) == exchange for r in step._captures.values())
            losses, kept, counts, caps = [], [], [], []
            for i in range(6):
                loss, k = step(batches[i % len(batches)])
                losses.append(float(loss))
                kept.append(k.cpu())
                counts.append(step.frame_counts.tolist())
                caps.append(step.capacity)
            torch.cuda.synchronize()
            bn = swin.swin.output_layer[3]
            out[(accumulation, exchange)] = dict(losses=losses, kept=kept, counts=counts, caps=caps, replays=dict(step.replays),
                                                 params={k: v.detach().cpu() for k, v in mm.named_parameters()}, mean=bn.running_mean.cpu(),
                                                 var=bn.running_var.cpu(), tracked=int(bn.num_batches_tracked),
                                                 reserved=dict(step.capture_reserved_bytes), buckets=len(avg.buckets) if exchange else 0)
    torch.save(out, os.path.join(out_dir, "rank_buckets.pt"))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rank_buckets"))
    mp.spawn(_worker, args=(_free_port(), d), nprocs=1, join=True)
    return torch.load(os.path.join(d, "rank_buckets.pt"), weights_only=False)


@pytest.mark.parametrize("accumulation", [1, 2])
def test_capacity_pairs_under_the_exchange_follow_the_single_graph_buckets(runs, accumulation):
    ref, got = runs[(accumulation, False)], runs[(accumulation, True)]
    print("losses reference", ref["losses"])
    print("losses exchange ", got["losses"])
    print("running mean max|diff|", float((ref["mean"] - got["mean"]).abs().max()), "running var max|diff|", float((ref["var"] - got["var"]).abs().max()))
    print("parameters max|diff| / scale", max(float((ref["params"][k] - got["params"][k]).abs().max()) / max(1.0, float(ref["params"][k].abs().max()))
                                              for k in ref["params"]))
    assert got["buckets"] >= 2                                                   # several collectives between A1 and A2
    for side in (ref, got):
        assert side["caps"] == [8, 12, 8, 12, 8, 12] and side["replays"] == {8: 3, 12: 3}
        assert side["counts"] == [[sum(SEQ[i % len(SEQ)])] * 2 for i in range(6)]
        assert set(side["reserved"]) == set(BUCKETS) and side["tracked"] == 6
    assert ref["losses"][0] != ref["losses"][-1]                                 # the optimiser moved something
    for a, b in zip(ref["losses"], got["losses"]):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (ref["losses"], got["losses"])
    for a, b in zip(ref["kept"], got["kept"]):
        assert torch.equal(a, b) and float(a.sum()) > 0
    assert (ref["mean"] - got["mean"]).abs().max().item() <= 1e-4 * max(1.0, ref["mean"].abs().max().item())
    assert (ref["var"] - got["var"]).abs().max().item() <= 1e-4 * max(1.0, ref["var"].abs().max().item())
    for k in ref["params"]:
        assert (ref["params"][k] - got["params"][k]).abs().max().item() <= 1e-4 * max(1.0, ref["params"][k].abs().max().item()), k
