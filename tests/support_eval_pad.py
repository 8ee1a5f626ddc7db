"""Models and loader batches for the tests of a short last evaluation batch and of a sharded split (tests/test_gpu_eval_pad_rows.py,
tests/test_gpu_eval_sharded.py): the shapes of tests/test_gpu_ragged_eval.py, restated and not imported -- B = 2, Lv = 6, stand-in text encoder, fp32
compute, seeded weights with the head's classifier scaled so that the frame filter has something to decide, every padded frame slot random."""
import types

import torch

from facialmmt_amd import synth

B, LV, NL, BUCKETS = 2, 6, 7, (8, 12)
CLASSIFIER_SCALE = 4.0


def build(dev, **kw):
    from facialmmt_amd import models
    from facialmmt_amd.config import default_args
    cfg = default_args(get_vision_utt_max_lens=LV, get_audio_utt_max_lens=24, trg_accumulation_steps=1, plm_module=synth.make_standin_plm(),
                       hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, crossmodal_attn_dropout_TA=0.0, crossmodal_attn_dropout_TA_V=0.0, **kw)
    cfg.compute_dtype = torch.float32
    swin = models.SwinForAffwildClassification(cfg)
    mm = models.MultiModalTransformerForClassification(cfg)
    synth.fill_state_dict(swin, seed=100)
    synth.fill_state_dict(mm, seed=200)
    with torch.no_grad():
        swin.classifier.weight.mul_(CLASSIFIER_SCALE)
    swin.to(dev).train()
    mm.to(dev).train()
    return swin, mm, cfg


def loader_batch(dev, cfg, counts, seed):
    """the loader's batch of B utterances for the given frame counts (frames (B, Lv, 3, 224, 224), num_imgs a list, as the reference's collate),
    cut to its first len(counts) utterances: a short last batch has every other dimension of a full one"""
    import bench
    full = list(counts) + [LV] * (B - len(counts))
    args = types.SimpleNamespace(utts=B, frames=LV, dtype="fp32", plm="roberta-large", input="float", resize="pil")
    batch = list(bench.synth_batch(args, dev, seed, cfg))
    batch[0] = batch[0] % 1000                                  # ids within the stand-in encoder's vocabulary
    vmask = torch.zeros(B, LV, device=dev)
    for u, k in enumerate(full):
        vmask[u, :k] = 1
    batch[6] = vmask
    batch[8], batch[9] = batch[8].view(B, LV, 3, 224, 224), full
    return tuple(t[:len(counts)] for t in batch)


def split(dev, cfg, counts_per_batch, seed0):
    return [loader_batch(dev, cfg, counts, seed0 + i) for i, counts in enumerate(counts_per_batch)]
