"""CPU tests of the per-tensor gradient report: the ABI surface of include/fmmt_stats.h (header == _lib.STATS_SIGNATURES == the built library, argument
validation in front of any launch), the pure host half train_step.GradReport.summarise on hand-made records, and FlatGradientTail's refusal of an
optimizer the fused update does not take."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_built():
    from facialmmt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_stats_header_signatures_and_library_agree():
    """include/fmmt_stats.h (included by fmmt.h) == _lib.STATS_SIGNATURES == the symbol of the built library: name, every argument's type and the return
    type; the table is disjoint from every other *SIGNATURES table, and _lib.SIGNATURES keeps its 59 names"""
    from facialmmt_amd import _lib, build
    assert "table_stats.hip" in build.SOURCES
    assert "fmmt_stats.h" in open(os.path.join(ROOT, "facialmmt_amd", "build.py")).read()
    assert '#include "fmmt_stats.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    raw = open(os.path.join(ROOT, "include", "fmmt_stats.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.STATS_SIGNATURES) == ["fmmt_table_stats"]
    others = [n for n in dir(_lib) if n.endswith("SIGNATURES") and n != "STATS_SIGNATURES"]
    assert len(others) >= 11
    for n in others:
        assert not set(_lib.STATS_SIGNATURES) & set(getattr(_lib, n)), n
    assert len(_lib.SIGNATURES) == 59

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    res, got = _lib.STATS_SIGNATURES["fmmt_table_stats"]
    assert got == [ctype_of(a) for a in protos["fmmt_table_stats"].split(",") if a.strip()]
    assert res is C.c_int and re.search(r"\bint\s+fmmt_table_stats\s*\(", src)
    # the table argument is fmmt_adamw_batch's, behind the field selector
    assert got[1:4] == _lib.SIGNATURES["fmmt_adamw_batch"][1][:3]
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(FMMT_STATS_\w+)\s+(\d+)", raw)}
    assert defines == {"FMMT_STATS_G": _lib.STATS_G, "FMMT_STATS_P": _lib.STATS_P, "FMMT_STATS_M": _lib.STATS_M, "FMMT_STATS_V": _lib.STATS_V}
    assert np.dtype(_lib.STATS_FIELDS).itemsize == _lib.STATS_BYTES == 16
    assert "train.py:135-143" in raw
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fmmt_table_stats" in text and "fmmt_stats.h" in text
    assert hasattr(_lib_built(), "fmmt_table_stats")


def test_arguments_are_validated_before_any_launch():
    """FMMT_EINVAL / FMMT_EALIGN come back without a device: nothing is launched for a NULL table, partial or stats, an empty table, a field that does
    not exist, a snapshot without the norm word, or misaligned buffers"""
    from facialmmt_amd import _lib
    lib = _lib_built()
    buf = (C.c_char * 1024)()
    p = C.addressof(buf)
    p += -p % 16

    def call(which=0, n_desc=1, n_blocks=1, desc=p, partial=p + 128, stats=p + 256, norm=None, bad_stats=None, bad_words=None):
        return lib.fmmt_table_stats(which, n_desc, n_blocks, desc, partial, stats, norm, bad_stats, bad_words, None)
    for bad in (dict(desc=None), dict(partial=None), dict(stats=None), dict(n_desc=0), dict(n_desc=-2), dict(n_blocks=0), dict(n_blocks=-1),
                dict(which=-1), dict(which=4), dict(bad_stats=p + 384), dict(bad_words=p + 512), dict(bad_stats=p + 384, bad_words=p + 512)):
        assert call(**bad) == _lib.FMMT_EINVAL, bad
    snap = dict(norm=p + 640, bad_stats=p + 384, bad_words=p + 512)
    for off in (1, 2, 4, 8, 12):
        assert call(partial=p + 128 + off) == _lib.FMMT_EALIGN, off
        assert call(stats=p + 256 + off) == _lib.FMMT_EALIGN, off
        assert call(**dict(snap, bad_stats=p + 384 + off)) == _lib.FMMT_EALIGN, off
    for off in (1, 2, 4, 6):
        assert call(**dict(snap, bad_words=p + 512 + off)) == _lib.FMMT_EALIGN, off
    assert call(n_desc=0, stats=p + 257) == _lib.FMMT_EINVAL                # the counts are looked at first
    assert call(which=7, partial=p + 129) == _lib.FMMT_EINVAL


def _rows(records):
    from facialmmt_amd import _lib
    a = np.zeros(len(records), dtype=np.dtype(_lib.STATS_FIELDS))
    for i, (s, m, k) in enumerate(records):
        a[i] = (s, m, k, 0)
    return a.view(np.int32).reshape(len(records), 4)


def test_summarise_names_norms_and_the_worst():
    from facialmmt_amd.train_step import GradReport
    names = ["a.weight", "a.bias", "b.weight", "param3"]
    stats = _rows([(9.0, 2.5, 0), (0.25, 0.5, 0), (16.0, 4.0, 0), (0.0, 0.0, 0)])
    zero = np.zeros_like(stats)
    r = GradReport.summarise(stats, zero, np.zeros(2, dtype=np.int64), names)
    assert r.names == names
    assert r.norm.tolist() == [3.0, 0.5, 4.0, 0.0] and r.sumsq.tolist() == [9.0, 0.25, 16.0, 0.0]
    assert r.max_abs.tolist() == [2.5, 0.5, 4.0, 0.0] and r.nonfinite.tolist() == [0, 0, 0, 0]
    assert r.sumsq.dtype == np.float32 and r.nonfinite.dtype == np.int32
    assert r.total_norm == np.sqrt(25.25)
    assert r.worst(2) == ["b.weight", "a.weight"] and r.worst(0) == [] and r.worst(9) == ["b.weight", "a.weight", "a.bias", "param3"]
    assert r.bad_updates == 0 and r.last_bad is None
    # the fp64 sum: 2^24 + 1 is no fp32 number
    big = GradReport.summarise(_rows([(2.0 ** 24, 1.0, 0), (1.0, 1.0, 0)]), None, None, ["x", "y"])
    assert big.total_norm == np.sqrt(2.0 ** 24 + 1.0) and not hasattr(big, "bad_updates") and not hasattr(big, "last_bad")
    assert big.worst(1) == ["x"]


def test_summarise_resolves_the_snapshot():
    from facialmmt_amd.train_step import GradReport
    names = ["a", "b", "c"]
    now = _rows([(1.0, 1.0, 0), (4.0, 2.0, 0), (0.0, 0.0, 0)])
    bad = _rows([(1.0, 1.0, 0), (float("nan"), 7.0, 2), (float("inf"), 3e19, 0)])
    r = GradReport.summarise(now, bad, np.array([3, 1], dtype=np.int64), names)
    assert r.bad_updates == 3 and r.nonfinite.sum() == 0 and r.norm.tolist() == [1.0, 2.0, 0.0]
    lb = r.last_bad
    assert lb.first == "b" and lb.names == names and lb.nonfinite.tolist() == [0, 2, 0]
    assert lb.norm[0] == 1.0 and np.isnan(lb.norm[1]) and np.isinf(lb.norm[2]) and np.isnan(lb.total_norm)
    assert lb.max_abs.tolist() == [1.0, 7.0, np.float32(3e19)]
    assert lb.worst(2) == ["b", "c"]                                        # a NaN norm is the worst there is
    # -1: the norm overflowed over tensors that are each finite
    r = GradReport.summarise(now, now, np.array([1, -1], dtype=np.int64), names)
    assert r.bad_updates == 1 and r.last_bad.first is None and r.last_bad.norm.tolist() == [1.0, 2.0, 0.0]
    for words in (np.array([1, 3], dtype=np.int64), np.array([1, -2], dtype=np.int64), np.zeros(3, dtype=np.int64)):
        with pytest.raises(ValueError):
            GradReport.summarise(now, bad, words, names)
    with pytest.raises(ValueError):
        GradReport.summarise(now[:2], bad, np.zeros(2, dtype=np.int64), names)


def test_report_names_follow_the_table_by_identity():
    """bind() is a host matter up to its allocations: on CPU tensors the names come out in the table's order, `param{i}` for a parameter nobody named"""
    import torch
    from facialmmt_amd.train_step import GradReport
    a, b, c = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 4097, 5))
    rep = GradReport([("second", b), ("first", a), ("again", a)])
    with pytest.raises(RuntimeError):
        rep.read()
    with pytest.raises(RuntimeError):
        rep.state("m")
    rep.reset()                                                             # unbound: nothing to zero
    rep.bind(torch.zeros(3 * 56, dtype=torch.uint8), 3, 4, [a, b, c])
    assert rep.names == ["first", "second", "param2"] and rep.n == 3 and rep.blocks == 4
    assert rep.stats.shape == (3, 4) and rep.bad_stats.shape == (3, 4) and rep.bad_words.shape == (2,) and rep.partial.shape == (4, 4)
    assert rep.stats.data_ptr() == rep.buf.data_ptr() and rep.bad_words.data_ptr() == rep.buf.data_ptr() + 2 * 3 * 16
    rep.bad_words[0] = 5
    before = (rep.stats.data_ptr(), rep.bad_stats.data_ptr(), rep.bad_words.data_ptr())
    rep.reset()
    assert int(rep.bad_words[0]) == 0 and before == (rep.stats.data_ptr(), rep.bad_stats.data_ptr(), rep.bad_words.data_ptr())
    r = rep.read()                                                          # zeros: a report nothing wrote into yet
    assert r.names == rep.names and r.bad_updates == 0 and r.last_bad is None and r.total_norm == 0.0
    with pytest.raises(ValueError):
        rep.state("g")
    with pytest.raises(RuntimeError):
        rep.bind(torch.zeros(3 * 56, dtype=torch.uint8), 3, 4, [a, b, c])


def test_flat_gradient_tail_refuses_a_report_without_the_fused_update():
    import torch
    from facialmmt_amd.train_step import FlatGradientTail, GradReport
    model = torch.nn.Linear(3, 2)
    for opt in (torch.optim.AdamW(model.parameters(), lr=1e-3), torch.optim.SGD(model.parameters(), lr=0.05)):   # a host-float learning rate; not AdamW
        with pytest.raises(ValueError, match="grad_report"):
            FlatGradientTail(model.parameters(), opt, 1.0, False, report=GradReport(model.named_parameters()))
        assert all(p.grad is None for p in model.parameters())
