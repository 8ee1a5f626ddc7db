"""fp64 restatement of the pooling head's loss as a MEAN OVER THE ROWS THAT HAVE A LABEL (csrc/pool_head.hip's _rows entry points), assembled from
tests/support_unimodal_oracle.head_reference: the rows whose label lies in [0, NL) go through head_reference as a batch of their own -- its
loss / B and dloss / B are then the valid mean --, the rows without a label get zeros in every gradient, and logits / alpha / pooled come from
head_reference over all rows (they do not depend on the labels).  Validated against autograd through F.cross_entropy(ignore_index=-100) in
tests/test_pad_rows_cpu.py; used by tests/test_gpu_pool_head_rows.py."""
import torch

from tests import support_unimodal_oracle as UO


def head_reference_rows(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, keep, dloss=1.0):
    NL = cls_w.shape[0]
    valid = (labels >= 0) & (labels < NL)
    full = UO.head_reference(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, torch.where(valid, labels, torch.zeros_like(labels)), keep, dloss)
    out = dict(logits=full["logits"], alpha=full["alpha"], pooled=full["pooled"], n_rows=int(valid.sum()))
    zero = {k: torch.zeros_like(full[k]) for k in ("dh", "dph", "dqq", "dv", "dvb", "dW", "db", "dscore")}
    if not valid.any():
        return dict(out, loss=torch.zeros((), dtype=torch.float64), **zero)
    sub = UO.head_reference(h[valid], ph[valid], qq, value_w, value_b, mask[valid], cls_w, cls_b, labels[valid], keep[valid], dloss)
    for k in ("dh", "dph", "dscore"):
        zero[k][valid] = sub[k]
    for k in ("dqq", "dv", "dvb", "dW", "db"):
        zero[k] = sub[k]
    return dict(out, loss=sub["loss"], **zero)


def pad_head_inputs(cpu, n_unlabelled):
    """the head's inputs (UO.head_inputs) with the LAST n_unlabelled rows turned into padded rows: h, ph and mask copies of row 0, label -100"""
    out = {k: v.clone() for k, v in cpu.items()}
    B = out["h"].shape[0]
    for r in range(B - n_unlabelled, B):
        for k in ("h", "ph", "mask"):
            out[k][r] = out[k][0]
        out["labels"][r] = -100
    return out
