"""CPU tests of the short-last-batch feature (pad_rows=True on the graphed steps): the ABI surface of include/fmmt_pool_head_rows.h, the three padding
functions of train_step (PAD_NOTE: what a padded row holds), the argument the padding rule of the T+A+V batch rests on -- the reference's literal
frame-selection loop (oracle.train_glue.select_frames_loop) leaves the real rows untouched when utterances without frames trail them -- and the fp64
restatement of the valid-mean loss (tests/support_pad_rows.py) against autograd through F.cross_entropy(ignore_index=-100).

An utterance without frames in the MIDDLE of a batch, num_imgs = (3, 0, 2), is a batch the loader never produces and the padding never builds (padded
rows trail).  It is HANDLED, not refused: train_step.select_frames computes what the literal loop computes for it (the loop's margin drops by one at
the empty utterance, which then owns nothing, and the utterance behind it loses the faces below the largest boundary so far -- the reference's quirk,
kept)."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import support_pad_rows as PR
from tests import support_unimodal_oracle as UO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the ABI surface
def test_pool_head_rows_header_signatures_and_library_agree():
    """include/fmmt_pool_head_rows.h (included by fmmt.h) == _lib.POOL_HEAD_ROWS_SIGNATURES == the symbols of the built library, as
    tests/test_ragged_cpu.py checks its header; the _rows pair is the plain pair with the row-count pointer added behind `keep`, and answers the
    limits with the plain pair's codes (argument validation happens before any launch: no GPU needed)"""
    from facialmmt_amd import _lib, build
    assert '#include "fmmt_pool_head_rows.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    raw = open(os.path.join(ROOT, "include", "fmmt_pool_head_rows.h")).read()
    assert "train.py:256-258" in raw
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.POOL_HEAD_ROWS_SIGNATURES) == ["fmmt_pool_head_bwd_rows", "fmmt_pool_head_fwd_rows"]
    for other in (_lib.SIGNATURES, _lib.POOL_HEAD_SIGNATURES, _lib.RAGGED_SIGNATURES, _lib.EVAL_COLLECT_SIGNATURES):
        assert not set(_lib.POOL_HEAD_ROWS_SIGNATURES) & set(other)

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    for name, args in protos.items():
        res, got = _lib.POOL_HEAD_ROWS_SIGNATURES[name]
        assert got == [ctype_of(a) for a in args.split(",") if a.strip()] and res is C.c_int, name
    for rows, plain, at in (("fmmt_pool_head_fwd_rows", "fmmt_pool_head_fwd", 22), ("fmmt_pool_head_bwd_rows", "fmmt_pool_head_bwd", 16)):
        a = list(_lib.POOL_HEAD_ROWS_SIGNATURES[rows][1])
        assert a.pop(at) is C.c_void_p and a == _lib.POOL_HEAD_SIGNATURES[plain][1], rows
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in protos) and "fmmt_pool_head_rows.h" in text
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in protos)
    none9, none7, none19 = [None] * 9, [None] * 7, [None] * 19
    for bad in ((2, 4, 160, 768, 7), (0, 0, 160, 768, 7), (0, 1025, 160, 768, 7), (0, 4, 1, 768, 7), (0, 4, 1025, 768, 7), (0, 4, 160, 12, 7), (0, 4, 160, 1032, 7),
                (0, 4, 160, 768, 0), (1, 4, 160, 768, 9)):
        assert lib.fmmt_pool_head_fwd_rows(*bad, *none9, 0.0, 0, *none7, None, 0, None) == lib.fmmt_pool_head_fwd(*bad, *none9, 0.0, 0, *none7, 0, None) == _lib.FMMT_EINVAL
        assert lib.fmmt_pool_head_bwd_rows(*bad, *none19, None, 0, None) == lib.fmmt_pool_head_bwd(*bad, *none19, 0, None) == _lib.FMMT_EINVAL, bad
    # a valid shape: no row-count word, null buffers, a misaligned h, a workspace that is too small -- the codes of the plain pair
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    p += -p % 16
    ok = (0, 2, 4, 64, 7)
    assert lib.fmmt_pool_head_fwd_rows(*ok, *([p] * 9), 0.0, 0, None, *([p] * 5), None, p, 1 << 20, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_pool_head_bwd_rows(*ok, *([p] * 11), None, *([p] * 7), p, 1 << 20, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_pool_head_fwd_rows(*ok, *none9, 0.0, 0, None, *([None] * 5), p, p, 1 << 20, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_pool_head_fwd_rows(*ok, p + 8, *([p] * 8), 0.0, 0, None, *([p] * 5), p, p, 1 << 20, None) \
        == lib.fmmt_pool_head_fwd(*ok, p + 8, *([p] * 8), 0.0, 0, None, *([p] * 5), p, 1 << 20, None) == _lib.FMMT_EALIGN
    assert lib.fmmt_pool_head_bwd_rows(*ok, p, p + 8, *([p] * 9), p, *([p] * 7), p, 1 << 20, None) \
        == lib.fmmt_pool_head_bwd(*ok, p, p + 8, *([p] * 9), *([p] * 7), p, 1 << 20, None) == _lib.FMMT_EALIGN
    assert lib.fmmt_pool_head_fwd_rows(*ok, *([p] * 9), 0.0, 0, None, *([p] * 5), p, p, 16, None) \
        == lib.fmmt_pool_head_fwd(*ok, *([p] * 9), 0.0, 0, None, *([p] * 5), p, 16, None) == _lib.FMMT_EWORKSPACE
    assert lib.fmmt_pool_head_bwd_rows(*ok, *([p] * 11), p, *([p] * 7), p, 16, None) == lib.fmmt_pool_head_bwd(*ok, *([p] * 11), *([p] * 7), p, 16, None) \
        == _lib.FMMT_EWORKSPACE
    assert lib.fmmt_pool_head_fwd_rows(*ok, *([p] * 9), 1.0, 0, None, *([p] * 5), p, p, 1 << 20, None) == _lib.FMMT_EINVAL      # p outside [0, 1)


# ------------------------------------------------------------------------------------------------ the padding functions
def _target_batch(b, Lv=4, lists=True):
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, 50, (b, 9), generator=g)
    num_imgs = [1 + (i % Lv) for i in range(b)]
    vmask = torch.zeros(b, Lv)
    for u, k in enumerate(num_imgs):
        vmask[u, :k] = 1
    utt = list(range(b))
    return (ids, torch.ones(b, 9), (ids % 7 == 0).float(), torch.randn(b, 5, 6, generator=g), torch.ones(b, 5), torch.randn(b, Lv, 8, generator=g), vmask,
            torch.arange(b) % 7, torch.randn(b, Lv, 3, 2, 2, generator=g), num_imgs if lists else torch.tensor(num_imgs), utt if lists else torch.tensor(utt))


@pytest.mark.parametrize("lists", [True, False], ids=["lists", "tensors"])
def test_pad_target_batch_follows_the_rule_field_by_field(lists):
    from facialmmt_amd.train_step import pad_target_batch
    batch = _target_batch(2, lists=lists)
    out = pad_target_batch(batch, 4)
    assert len(out) == 11
    for i in (0, 1, 2, 3, 4):                                  # text and audio: the real rows, then copies of row 0
        assert out[i].shape == (4, *batch[i].shape[1:]) and out[i].dtype == batch[i].dtype
        assert torch.equal(out[i][:2], batch[i]) and torch.equal(out[i][2], batch[i][0]) and torch.equal(out[i][3], batch[i][0])
    for i in (5, 6, 8):                                        # vision_inputs, vision_mask, frames: zeros
        assert out[i].shape == (4, *batch[i].shape[1:]) and torch.equal(out[i][:2], batch[i]) and float(out[i][2:].abs().max()) == 0.0
    assert out[7].tolist() == batch[7].tolist() + [-100, -100] and out[7].dtype == torch.int64
    if lists:
        assert out[9] == batch[9] + [0, 0] and out[10] == batch[10] + [batch[10][0]] * 2 and isinstance(out[9], list)
    else:
        assert out[9].tolist() == batch[9].tolist() + [0, 0] and out[10].tolist() == batch[10].tolist() + [int(batch[10][0])] * 2
    assert sum(out[9] if lists else out[9].tolist()) == sum(_target_batch(2)[9])       # the padded counts sum to the real frames
    same = pad_target_batch(batch, 2)                          # b == rows: the identity
    assert all(a is b for a, b in zip(same, batch))
    for bad in (_target_batch(0, lists=lists) if not lists else tuple(t[:0] for t in batch), _target_batch(5, lists=lists)):
        with pytest.raises(ValueError):
            pad_target_batch(bad, 4)
    with pytest.raises(ValueError):
        pad_target_batch(batch[:10], 4)


def test_pad_unimodal_and_aux_batches():
    from facialmmt_amd.train_step import pad_aux_batch, pad_unimodal_batch
    g = torch.Generator().manual_seed(6)
    feature, mask, labels = torch.randn(3, 5, 8, generator=g), (torch.rand(3, 5, generator=g) > 0.3).float(), torch.tensor([4, 0, 6])
    f, m, l = pad_unimodal_batch((feature, mask, labels), 5)
    assert f.shape == (5, 5, 8) and m.shape == (5, 5) and l.tolist() == [4, 0, 6, -100, -100]
    assert torch.equal(f[:3], feature) and torch.equal(m[:3], mask)
    for r in (3, 4):
        assert torch.equal(f[r], feature[0]) and torch.equal(m[r], mask[0])
    f, m, l = pad_unimodal_batch((feature, mask, labels), 3)
    assert f is feature and m is mask and l is labels
    for bad, rows in (((feature[:0], mask[:0], labels[:0]), 4), ((feature, mask, labels), 2)):
        with pytest.raises(ValueError):
            pad_unimodal_batch(bad, rows)
    images, ilab = torch.randn(3, 3, 4, 4, generator=g), torch.tensor([1, 2, 3])
    x, y = pad_aux_batch(images, ilab, 8)
    assert x.shape == (8, 3, 4, 4) and torch.equal(x[:3], images) and float(x[3:].abs().max()) == 0.0 and y.tolist() == [1, 2, 3] + [-100] * 5
    x, y = pad_aux_batch(images, ilab, 3)
    assert x is images and y is ilab
    for bad, rows in (((images[:0], ilab[:0]), 8), ((images, ilab), 2)):
        with pytest.raises(ValueError):
            pad_aux_batch(*bad, rows)


# ------------------------------------------------------------------------------------------------ the frame filter with trailing empty utterances
def _filter_inputs(num_imgs, passes, Lv=4, D=6, NL=7, seed=21):
    g = torch.Generator().manual_seed(seed)
    b, n = len(num_imgs), sum(num_imgs)
    near_uniform = torch.softmax(0.05 * torch.randn(n, NL, generator=g), dim=1)           # sum p^2 ~ 1 / 7
    one_hot = torch.eye(NL)[torch.randint(0, NL, (n,), generator=g)] * 0.97 + 0.03 / NL   # sum p^2 ~ 0.95
    preds = torch.where(torch.tensor(passes, dtype=torch.bool).view(-1, 1), one_hot, near_uniform)
    vin = torch.randn(b, Lv, D, generator=g)
    vmask = torch.zeros(b, Lv)
    for u, k in enumerate(num_imgs):
        vmask[u, :k] = 1
    return preds, vin, vmask


@pytest.mark.parametrize("branch", ["some_pass", "none_passes", "all_pass"])
@pytest.mark.parametrize("num_imgs", [(3, 2, 0, 0), (1, 0, 0, 0)], ids=lambda n: "-".join(map(str, n)))
def test_trailing_rows_without_frames_leave_the_real_rows_alone(num_imgs, branch):
    """the literal loop on the padded batch against the literal loop on the compact batch: real rows bit-equal in both branches (threshold above
    every face: keep everything; below every face / between: selection), padded rows' masks all zero; and train_step.select_frames (the torch
    formulation the kernel restates) equals the loop on the padded batch, values, mask and the gradient of preds"""
    from facialmmt_amd.train_step import pad_target_batch, select_frames
    from oracle.train_glue import select_frames_loop
    real = [n for n in num_imgs if n > 0]
    b, rows, n = len(real), len(num_imgs), sum(real)
    passes = {"some_pass": [1, 0, 1, 1, 0][:n], "none_passes": [0] * n, "all_pass": [1] * n}[branch]
    thr = 0.5
    preds, vin, vmask = _filter_inputs(real, passes)
    want, want_mask = select_frames_loop(preds, vin, vmask, list(real), thr)
    dummy = torch.zeros(b, 1)
    padded = pad_target_batch((dummy, dummy, dummy, dummy, dummy, vin, vmask, torch.zeros(b, dtype=torch.int64), torch.zeros(b, 4, 1), list(real), [0] * b), rows)
    pvin, pmask, pnum = padded[5], padded[6], padded[9]
    assert tuple(pnum) == tuple(num_imgs)
    got, got_mask = select_frames_loop(preds, pvin, pmask, pnum, thr)
    assert torch.equal(got[:b], want) and torch.equal(got_mask[:b], want_mask)
    assert float(got_mask[b:].abs().max()) == 0.0 and float(got[b:].abs().max()) == 0.0
    if branch == "none_passes":
        assert torch.equal(got_mask[:b], vmask)
    else:
        assert float(got_mask.sum()) > 0
    dout = torch.randn(rows, 4, 6 + 7, generator=torch.Generator().manual_seed(3))
    pl = preds.clone().requires_grad_(True)
    (select_frames_loop(pl, pvin, pmask, pnum, thr)[0] * dout).sum().backward()
    pt = preds.clone().requires_grad_(True)
    ours, ours_mask = select_frames(pt, pvin, pmask, torch.tensor(pnum), thr, n_valid=torch.tensor([n, n], dtype=torch.int32))
    (ours * dout).sum().backward()
    assert torch.equal(ours.detach(), got) and torch.equal(ours_mask, got_mask) and torch.equal(pt.grad, pl.grad)


@pytest.mark.parametrize("passes", [[1, 1, 1, 1, 1], [1, 0, 1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 1, 1]])
def test_an_empty_utterance_in_the_middle_is_computed_as_the_literal_loop_computes_it(passes):
    """num_imgs = (3, 0, 2): not refused -- train_step.select_frames gives the loop's result (module docstring)"""
    from facialmmt_amd.train_step import select_frames
    from oracle.train_glue import select_frames_loop
    num_imgs = [3, 0, 2]
    preds, vin, vmask = _filter_inputs(num_imgs, passes)
    want, want_mask = select_frames_loop(preds, vin, vmask, num_imgs, 0.5)
    got, got_mask = select_frames(preds, vin, vmask, torch.tensor(num_imgs), 0.5)
    assert torch.equal(got, want) and torch.equal(got_mask, want_mask)
    assert float(want_mask[1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the valid-mean loss in fp64
@pytest.mark.parametrize("B,unlabelled", [(1, 0), (3, 1), (5, 4), (5, 0)])
def test_valid_mean_restatement_against_cross_entropy_with_ignore_index(B, unlabelled):
    """tests/support_pad_rows.head_reference_rows against autograd through oracle.multimodal.additive_attention and F.cross_entropy, whose default
    ignore_index is the padded rows' label -100: loss and every gradient to 1e-10; the rows without a label get exact zeros"""
    L, H, NL = 11, 16, 7
    cpu, _ = UO.head_inputs(B, L, H, NL, seed=40)
    cpu = PR.pad_head_inputs(cpu, unlabelled)
    keep = (torch.rand(B, H, generator=torch.Generator().manual_seed(1)) > 0.3).double() / 0.7
    ref = PR.head_reference_rows(**cpu, keep=keep, dloss=0.37)
    auto = UO.head_autograd(**cpu, keep=keep, dloss=0.37)
    assert ref["n_rows"] == B - unlabelled
    logits = ref["logits"]
    assert abs(float(ref["loss"]) - float(torch.nn.functional.cross_entropy(logits, cpu["labels"], ignore_index=-100))) <= 1e-12
    for k in ("loss", "logits", "alpha", "dh", "dph", "dqq", "dv", "dvb", "dW", "db"):
        err = float((ref[k].reshape(-1) - auto[k].reshape(-1)).abs().max())
        assert err <= 1e-10 * max(1.0, float(auto[k].abs().max())), (k, err)
    if unlabelled:
        assert float(ref["dh"][B - unlabelled:].abs().max()) == 0.0 and float(ref["dph"][B - unlabelled:].abs().max()) == 0.0


def test_valid_mean_restatement_without_a_labelled_row_is_all_zero():
    cpu, _ = UO.head_inputs(3, 11, 16, 7, seed=40)
    cpu = PR.pad_head_inputs(cpu, 3)
    ref = PR.head_reference_rows(**cpu, keep=torch.ones(3, 16))
    assert ref["n_rows"] == 0 and float(ref["loss"]) == 0.0
    assert all(float(ref[k].abs().max()) == 0.0 for k in ("dh", "dph", "dqq", "dv", "dvb", "dW", "db"))
    assert torch.isfinite(ref["logits"]).all()
