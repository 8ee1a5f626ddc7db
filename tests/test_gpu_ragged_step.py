"""GPU test of the target-task step on RAGGED batches: GraphedTargetStep(frame_capacity=12) fed the loader's (B, Lv, ...) padded frames and the real
counts -- one capture, device-side packing, the head's BatchNorm and the frame filter restricted to the real rows -- against the eager TargetStep
fed the compact (sum num_imgs, ...) frames, which is the code path that existed before the feature.

The noise-free configuration of tests/test_gpu_train_step.py::_run_six (fp32 compute, tau = 1e5, threshold 0.1, DropPath and dropout off, stand-in
text encoder, SGD) and the assertions of its test_whole_step_graphs_equal_eager_step: losses to 2e-4, parameters and the BatchNorm running mean to
1e-4 of scale, num_batches_tracked equal, kept-frame masks equal and non-empty.  The padded frame slots of the loader batch hold random data, not
zeros: packing, not luck, has to remove them."""
import types

import pytest
import torch

from facialmmt_amd import synth

pytestmark = pytest.mark.gpu

B, LV, CAP = 2, 6, 12
_REF = {}


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


def _batches(dev, cfg, num_imgs):
    """(loader batch, compact batch) for the given frame counts: the same synthetic batch, frames (B, Lv, 3, 224, 224) with EVERY slot random"""
    import bench
    args = types.SimpleNamespace(utts=B, frames=LV, dtype="fp32", plm="roberta-large", input="float", resize="pil")
    batch = list(bench.synth_batch(args, dev, 0, cfg))
    batch[0] = batch[0] % 1000
    frames = batch[8].view(B, LV, 3, 224, 224)
    vmask = torch.zeros(B, LV, device=dev)
    for u, k in enumerate(num_imgs):
        vmask[u, :k] = 1
    batch[6] = vmask
    padded, compact = list(batch), list(batch)
    padded[8], padded[9] = frames, list(num_imgs)                                 # num_imgs as the reference's collate yields it
    compact[8] = torch.cat([frames[u, :k] for u, k in enumerate(num_imgs)], dim=0).contiguous()
    compact[9] = torch.tensor(num_imgs, device=dev)
    return tuple(padded), tuple(compact)


def _run(dev, side, accumulation, sequence, swin_gradients="compute"):
    """six micro-steps over `sequence` of frame counts (cycled); side: 'graphed' (padded batches, frame_capacity) or 'eager' (compact batches)"""
    from facialmmt_amd.train_step import GraphedTargetStep, TargetStep
    key = (side, accumulation, tuple(map(tuple, sequence)), swin_gradients)
    if side == "eager" and key in _REF:
        return _REF[key]
    cfg, swin, mm = _models(dev, accumulation)
    opt = torch.optim.SGD(mm.parameters(), lr=0.05)
    pairs = [_batches(dev, cfg, n) for n in sequence]
    if side == "graphed":
        step = GraphedTargetStep(swin, mm, opt, None, cfg, pairs[0][0], autocast_dtype=None, discarded_swin_gradients=swin_gradients, frame_capacity=CAP)
        assert step.text_stream is not None
    else:
        step = TargetStep(swin, mm, opt, None, cfg, autocast_dtype=None, discarded_swin_gradients=swin_gradients)
    losses, kept, counts = [], [], []
    for i in range(6):
        padded, compact = pairs[i % len(pairs)]
        if side == "graphed" and i % 2:                                          # alternately a list and a device tensor
            padded = padded[:9] + (torch.tensor(padded[9], device=dev),) + padded[10:]
        loss, k = step(padded if side == "graphed" else compact)
        losses.append(float(loss))
        kept.append(k.clone())
        if side == "graphed":
            counts.append(step.frame_counts.tolist())
    torch.cuda.synchronize()
    bn = swin.swin.output_layer[3]
    out = (losses, {k: v.detach().clone() for k, v in mm.named_parameters()}, bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked), kept, counts)
    if side == "eager":
        _REF[key] = out
    return out


def _same_trajectory(dev, accumulation, sequence, swin_gradients="compute"):
    l0, p0, rm0, rv0, nb0, k0, _ = _run(dev, "eager", accumulation, sequence, swin_gradients)
    l1, p1, rm1, rv1, nb1, k1, counts = _run(dev, "graphed", accumulation, sequence, swin_gradients)
    print("losses eager  ", l0)
    print("losses graphed", l1)
    print("running mean max|diff|", float((rm0 - rm1).abs().max()), "running var max|diff|", float((rv0 - rv1).abs().max()))
    assert counts == [[sum(sequence[i % len(sequence)])] * 2 for i in range(6)]
    assert l0[0] != l0[-1]                                       # the optimiser moved something
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (l0, l1)
    assert nb0 == nb1 == 6
    for a, b in zip(k0, k1):
        assert torch.equal(a, b) and float(a.sum()) > 0
    assert (rm0 - rm1).abs().max().item() <= 1e-4 * max(1.0, rm0.abs().max().item())
    assert (rv0 - rv1).abs().max().item() <= 1e-4 * max(1.0, rv0.abs().max().item())
    for k in p0:
        assert (p0[k] - p1[k]).abs().max().item() <= 1e-4 * max(1.0, p0[k].abs().max().item()), k


@pytest.mark.parametrize("accumulation", [1, 2])
def test_graphed_step_on_padded_batch_equals_eager_step_on_compact_frames(accumulation):
    """num_imgs = [5, 2]: 7 real frames in a capacity of 12, six micro-steps"""
    _same_trajectory(torch.device("cuda:0"), accumulation, [[5, 2]])


@pytest.mark.parametrize("swin_gradients", ["compute", "skip"])
def test_frame_counts_change_between_replays_without_a_recapture(swin_gradients):
    """[5, 2] -> [6, 6] (every slot real) -> [1, 3] (a one-frame utterance) and round again through ONE captured graph: every step matches the eager
    step on the corresponding compact frames; also with Swin's discarded backward skipped"""
    _same_trajectory(torch.device("cuda:0"), 1, [[5, 2], [6, 6], [1, 3]], swin_gradients)


def test_padded_frames_leave_no_trace_in_swin_weight_gradients():
    """One eager micro-step: TargetStep(frame_capacity=12) on the padded batch against TargetStep on the compact frames, the gradient of Swin's
    patch_embed.proj.weight caught by a hook -- every padded frame's contribution to it has to be an exact zero, which is what the masked BatchNorm
    backward is for.  Tolerance of tests/test_gpu_step_oracle.py::compare_fp32_gradients: max|g - ref| <= 1e-3 max|ref|, relative L2 <= 1e-3."""
    from facialmmt_amd.train_step import TargetStep
    from tests.support_step_oracle import grad_stats
    dev = torch.device("cuda:0")
    got = {}
    for side in ("compact", "packed"):
        cfg, swin, mm = _models(dev, 1)
        padded, compact = _batches(dev, cfg, [5, 2])
        step = TargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=0.05), None, cfg, autocast_dtype=None,
                          frame_capacity=CAP if side == "packed" else None)
        box = []
        swin.swin.patch_embed.proj.weight.register_hook(lambda g, box=box: box.append(g.detach().clone()))
        loss, kept = step(padded if side == "packed" else compact)
        torch.cuda.synchronize()
        assert len(box) == 1
        got[side] = (float(loss), box[0], kept.clone())
    mx, l2, _ = grad_stats(got["packed"][1], got["compact"][1])
    print(f"d(patch_embed.proj.weight): max|g - ref| / max|ref| = {mx:.3e}, relative L2 = {l2:.3e}, max|ref| = {float(got['compact'][1].abs().max()):.3e}")
    assert float(got["compact"][1].abs().max()) > 0
    assert mx <= 1e-3 and l2 <= 1e-3
    assert abs(got["packed"][0] - got["compact"][0]) <= 2e-4 * max(1.0, abs(got["compact"][0])) and torch.equal(got["packed"][2], got["compact"][2])


def test_more_frames_than_the_capacity_raise_before_anything_is_launched():
    """num_imgs = [6, 6] as a list into a step captured for frame_capacity = 8: ValueError from the host-side check, the step's state untouched"""
    from facialmmt_amd.train_step import GraphedTargetStep
    dev = torch.device("cuda:0")
    cfg, swin, mm = _models(dev, 1)
    fits, _ = _batches(dev, cfg, [5, 2])
    full, _ = _batches(dev, cfg, [6, 6])
    opt = torch.optim.SGD(mm.parameters(), lr=0.05)
    with pytest.raises(ValueError, match="frame_capacity=8"):                    # the constructor's sample batch is checked the same way
        GraphedTargetStep(swin, mm, opt, None, cfg, full, autocast_dtype=None, frame_capacity=8)
    with pytest.raises(NotImplementedError):
        GraphedTargetStep(swin, mm, opt, None, cfg, fits, autocast_dtype=None, frame_capacity=8, pipeline_swin=True)
    step = GraphedTargetStep(swin, mm, opt, None, cfg, fits, autocast_dtype=None, frame_capacity=8)
    bn = swin.swin.output_layer[3]
    before = (int(bn.num_batches_tracked), bn.running_mean.clone(), step.static[9].clone())
    with pytest.raises(ValueError, match="frame_capacity=8"):
        step(full)
    torch.cuda.synchronize()
    assert step.i_batch == 0 and int(bn.num_batches_tracked) == before[0] and torch.equal(bn.running_mean, before[1]) and torch.equal(step.static[9], before[2])
    loss, kept = step(fits)                                                      # and the step still works
    assert step.frame_counts.tolist() == [7, 7] and torch.isfinite(loss) and float(kept.sum()) > 0
