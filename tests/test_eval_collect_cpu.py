"""CPU tests of ragged evaluation: the ABI surface of include/fmmt_eval_collect.h, the bucket choice of GraphedEvalStep(frame_capacity=...) as a pure
function, and the host half of MeldMetrics.collected()."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_collect_header_signatures_and_library_agree():
    """include/fmmt_eval_collect.h (included by fmmt.h) == _lib.EVAL_COLLECT_SIGNATURES == the symbols of the built library: names, every argument's
    type and the return type, as test_ragged_header_signatures_and_library_agree does; argument validation happens before any launch, so it runs
    without a GPU"""
    from facialmmt_amd import _lib, build
    assert "eval.hip" in build.SOURCES
    assert '#include "fmmt_eval_collect.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmmt_eval_collect.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.EVAL_COLLECT_SIGNATURES) == ["fmmt_eval_accumulate_at"]
    for other in (_lib.SIGNATURES, _lib.POOL_HEAD_SIGNATURES, _lib.RAGGED_SIGNATURES):
        assert not set(_lib.EVAL_COLLECT_SIGNATURES) & set(other)

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    returns = {m.group(2): m.group(1) for m in re.finditer(r"\b(int|size_t)\s+(fmmt_\w+)\s*\(", src)}
    for name, args in protos.items():
        want = [ctype_of(a) for a in args.split(",") if a.strip()]
        res, got = _lib.EVAL_COLLECT_SIGNATURES[name]
        assert got == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g is not w], len(got), len(want))
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[returns[name]], name
    # fmmt_eval_accumulate's list up to the confusion matrix, then cursor / logits_out / labels_out / pred_out / out_capacity / stream
    assert _lib.EVAL_COLLECT_SIGNATURES["fmmt_eval_accumulate_at"][1][:9] == _lib.SIGNATURES["fmmt_eval_accumulate"][1][:9]
    assert "fmmt_eval_accumulate_at" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "fmmt_eval_accumulate_at")
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    p += -p % 16

    def call(dtype=0, B=4, NL=7, logits=p, ld=7, labels=p, loss=p, count=p + 8, conf=p + 16, cursor=p + 128, lo=p, la=p, pr=None, cap=8):
        return lib.fmmt_eval_accumulate_at(dtype, B, NL, logits, ld, labels, loss, count, conf, cursor, lo, la, pr, cap, None)
    for bad in (dict(B=0), dict(B=1025), dict(NL=0), dict(NL=9), dict(ld=6), dict(cap=-1), dict(dtype=5), dict(cursor=None), dict(lo=None), dict(la=None),
                dict(logits=None), dict(labels=None), dict(loss=None), dict(count=None), dict(conf=None)):
        assert call(**bad) == _lib.FMMT_EINVAL, bad
    for bad in (dict(cursor=p + 132), dict(la=p + 4), dict(labels=p + 4), dict(loss=p + 4), dict(count=p + 12), dict(conf=p + 20)):
        assert call(**bad) == _lib.FMMT_EALIGN, bad


def test_bucket_choice_is_a_pure_function_of_host_counts():
    from facialmmt_amd.eval_step import pick_bucket
    buckets = (8, 12, 20)
    assert pick_bucket([5, 3], 6, buckets) == 8                        # exact fit
    assert pick_bucket([5, 4], 6, buckets) == 12                       # one above a bucket
    assert pick_bucket([6, 6], 6, buckets) == 12
    assert pick_bucket([6, 6, 1], 6, buckets) == 20
    assert pick_bucket([0, 0], 6, buckets) == 8
    assert pick_bucket([9, -2], 6, buckets) == 8                       # counts clamp to [0, Lv], as the packing kernel clamps them
    for counts in ([5, 3], [5, 4], [6, 6, 6, 2]):                      # a list and a CPU tensor agree
        assert pick_bucket(torch.tensor(counts), 6, buckets) == pick_bucket(counts, 6, buckets)
    assert pick_bucket([1], 6, (12,)) == 12
    for bad in ([6, 6, 6, 3], torch.tensor([6, 6, 6, 3])):             # 21 frames
        with pytest.raises(ValueError, match="21 face frames.*frame_capacity=20"):
            pick_bucket(bad, 6, buckets)

    class OnDevice(torch.Tensor):                                       # stands for a device tensor: it is not read, whatever it holds
        is_cuda = property(lambda self: True)

        def tolist(self):
            raise AssertionError("a device tensor's counts were read on the host")
    assert pick_bucket(torch.Tensor._make_subclass(OnDevice, torch.tensor([6.0, 6.0, 6.0, 6.0])), 6, buckets) == 20


def test_clamped_sample_counts_fit_the_bucket():
    from facialmmt_amd.eval_step import _clamp_counts
    assert _clamp_counts([5, 2], 6, 12) == [5, 2]
    assert _clamp_counts([6, 6], 6, 8) == [6, 2]
    assert _clamp_counts(torch.tensor([9, 6]), 6, 7) == [6, 1]
    assert _clamp_counts([6, 6], 6, 4) == [4, 0]


def test_collected_reports_an_overflow_from_the_host_copy():
    from facialmmt_amd.eval_step import MeldMetrics
    nl = 7
    host = np.zeros(2 + nl * nl + 1, dtype=np.int64)
    host[-1] = 40
    assert MeldMetrics.collected_count(host, 40) == 40
    assert MeldMetrics.collected_count(host, 64) == 40
    host[-1] = 66
    with pytest.raises(ValueError, match=r"66 rows.*collect_rows=40"):
        MeldMetrics.collected_count(host, 40)
    host[-1] = 0
    assert MeldMetrics.collected_count(host, 0) == 0
    # the accumulators in front of the cursor are summarised as before
    host[0] = np.array([3.0]).view(np.int64)[0]
    host[1] = 2
    host[2] = 2
    r = MeldMetrics.summarise(host[:-1], nl)
    assert r.avg_loss == 1.5 and r.count == 2 and int(r.confusion[0, 0]) == 2
