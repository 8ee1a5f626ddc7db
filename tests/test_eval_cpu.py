"""CPU tests of the evaluation step's host side: the F1 / confusion-matrix formulas of eval_step.MeldMetrics and eval_step.eval_meld against
scikit-learn (what the reference's utils/eval_metrics.py calls), the argument validation of the two evaluation entry points (before any launch:
no GPU needed), and the refusal of CPU tensors / gradients by their Python front ends."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from facialmmt_amd import _lib

NL = 7


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        from facialmmt_amd.build import build
        build(verbose=False)
    return _lib.load()


def _cases():
    """(name, truth, prediction): random vectors over all classes, with classes absent from the labels, from the predictions, from both, one
    class only, one sample"""
    rng = np.random.RandomState(20240607)
    out = []
    for i in range(200):
        n = int(rng.randint(1, 120))
        present = rng.choice(NL, size=int(rng.randint(1, NL + 1)), replace=False)
        pred_from = rng.choice(NL, size=int(rng.randint(1, NL + 1)), replace=False) if i % 3 else present
        out.append((f"random{i}", rng.choice(present, size=n), rng.choice(pred_from, size=n)))
    out.append(("single_class_all_right", np.full(17, 3), np.full(17, 3)))
    out.append(("single_class_all_wrong", np.full(9, 2), np.full(9, 5)))
    out.append(("one_sample", np.array([6]), np.array([0])))
    out.append(("all_classes_perfect", np.arange(NL).repeat(3), np.arange(NL).repeat(3)))
    return out


def test_f1_formulas_match_scikit_learn():
    sk = pytest.importorskip("sklearn.metrics", reason="scikit-learn is not installed: nothing to hold the F1 formulas against")
    from facialmmt_amd.eval_step import MeldMetrics, confusion_matrix, eval_meld, f1_from_confusion
    for name, truth, pred in _cases():
        want_w = sk.f1_score(truth, pred, average="weighted", zero_division=0)
        want_c = sk.f1_score(truth, pred, average=None, labels=list(range(NL)), zero_division=0)
        conf = confusion_matrix(pred, truth, NL)
        assert conf.sum() == len(truth) and np.array_equal(conf, sk.confusion_matrix(truth, pred, labels=list(range(NL)))), name
        got_w, got_c = f1_from_confusion(conf)
        assert abs(got_w - want_w) <= 1e-12, (name, got_w, want_w)
        assert got_c.shape == (NL,) and np.abs(got_c - want_c).max() <= 1e-12, (name, got_c, want_c)
        # the accumulator words as MeldMetrics.result() copies them from the device: [loss sum as the bits of a double, count, confusion]
        host = np.concatenate([np.array([2.5 * len(truth)], dtype=np.float64).view(np.int64), [len(truth)], conf.ravel()]).astype(np.int64)
        r = MeldMetrics.summarise(host, NL)
        assert abs(r.weighted_f1 - want_w) <= 1e-12 and np.abs(r.f1_per_class - want_c).max() <= 1e-12, name
        assert r.count == len(truth) and abs(r.avg_loss - 2.5) <= 1e-12 and np.array_equal(r.confusion, conf), name
        # eval_meld: logits whose argmax is `pred`
        logits = torch.from_numpy(np.random.RandomState(len(truth)).rand(len(truth), NL).astype(np.float32))
        logits[torch.arange(len(truth)), torch.from_numpy(pred)] = 2.0
        assert abs(eval_meld(logits, torch.from_numpy(truth)) - want_w) <= 1e-12, name


def test_eval_meld_ignores_padded_rows_and_takes_the_first_maximum(capsys):
    from facialmmt_amd.eval_step import MeldMetrics, eval_meld
    logits = torch.tensor([[0.0, 1.0, 1.0, 0, 0, 0, 0], [3.0, 0, 0, 0, 0, 0, 3.0], [0, 0, 0, 0, 9.0, 0, 0]])
    truths = torch.tensor([1, 0, -100])                       # tie -> class 1, tie -> class 0, padded row
    assert eval_meld(logits, truths, test=True) == 1.0
    assert "Neutral, Surprise, Fear, Sadness, Joy, Disgust, Anger" in capsys.readouterr().out
    empty = MeldMetrics.summarise(np.zeros(2 + NL * NL, dtype=np.int64), NL)
    assert empty.count == 0 and empty.weighted_f1 == 0.0 and np.isnan(empty.avg_loss)


def test_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib_loaded()
    E = _lib.FMMT_EINVAL
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned non-NULL address: validation must not touch it

    def head(dtype=0, N=4, K=512, H=64, NL=7, feats=p, ld=512, tau=1.0, preds=p):
        return lib.fmmt_emotion_head_fwd(dtype, N, K, H, NL, feats, ld, p, p, p, p, None, tau, preds, None, None)

    assert head(NL=9) == E and head(NL=0) == E
    assert head(H=65) == E and head(H=32) == E
    assert head(K=100) == E and head(K=0) == E and head(ld=256) == E
    assert head(N=0) == E and head(dtype=7) == E and head(tau=0.0) == E
    assert head(feats=None) == E and head(preds=None) == E
    assert head(ld=514) == _lib.FMMT_EALIGN and head(feats=p + 4) == _lib.FMMT_EALIGN

    def acc(dtype=0, B=4, NL=7, logits=p, ld=7, labels=p, loss=p, out=None, off=0, cap=0):
        return lib.fmmt_eval_accumulate(dtype, B, NL, logits, ld, labels, loss, p, p, None, out, off, cap, None)

    assert acc(B=1025) == E and acc(B=0) == E
    assert acc(NL=9) == E and acc(NL=0) == E and acc(ld=6) == E and acc(dtype=3) == E
    assert acc(logits=None) == E and acc(labels=None) == E and acc(loss=None) == E
    assert acc(out=p, off=0, cap=3) == E and acc(out=p, off=-1, cap=100) == E and acc(out=p, off=97, cap=100) == E


def test_front_ends_refuse_cpu_tensors_and_gradients():
    from facialmmt_amd import ops
    lin, cls = torch.nn.Linear(512, 64), torch.nn.Linear(64, NL)
    with torch.no_grad(), pytest.raises(_lib.FmmtError, match="GPU only"):
        ops.emotion_head(torch.zeros(4, 512), lin, cls, 1.0)
    with torch.no_grad(), pytest.raises(_lib.FmmtError, match="GPU only"):
        ops.eval_accumulate(torch.zeros(4, NL), torch.zeros(4, dtype=torch.int64), torch.zeros(2 + NL * NL, dtype=torch.int64))
    import facialmmt_amd.torch_ops  # noqa: F401
    assert hasattr(torch.ops.fmmt, "emotion_head") and hasattr(torch.ops.fmmt, "eval_accumulate")
    with pytest.raises((NotImplementedError, RuntimeError)):    # no CPU kernel is registered
        torch.ops.fmmt.eval_accumulate(torch.zeros(4, NL), torch.zeros(4, dtype=torch.int64), torch.zeros(2 + NL * NL, dtype=torch.int64), None, 0)
    meta = torch.ops.fmmt.emotion_head(torch.zeros(5, 512, device="meta"), lin.weight.to("meta"), lin.bias.to("meta"), cls.weight.to("meta"),
                                       cls.bias.to("meta"), None, 1.0)
    assert tuple(meta[0].shape) == (5, NL) and tuple(meta[1].shape) == (5,) and meta[0].dtype == torch.float32


def test_evaluation_abi_is_declared_everywhere():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from facialmmt_amd import build
    assert "eval.hip" in build.SOURCES
    text = open(os.path.join(here, "INTEGRATION.md")).read()
    for name in ("fmmt_emotion_head_fwd", "fmmt_eval_accumulate"):
        assert name in _lib.SIGNATURES and name in text
    assert len(_lib.SIGNATURES) == 59
