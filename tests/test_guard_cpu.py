"""CPU tests of the guarded optimizer update: the ABI surface of include/fmmt_guard.h (header == _lib.GUARD_SIGNATURES == the built library, argument
validation in front of any launch) and the host half of train_step.TrainMonitor."""
import ctypes as C
import math
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


def test_guard_header_signatures_and_library_agree():
    """include/fmmt_guard.h (included by fmmt.h) == _lib.GUARD_SIGNATURES == the symbols of the built library: names, every argument's type and the
    return type, as test_eval_collect_header_signatures_and_library_agree does; the table is disjoint from the five that exist"""
    from facialmmt_amd import _lib, build
    assert "guard.hip" in build.SOURCES
    assert '#include "fmmt_guard.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmmt_guard.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.GUARD_SIGNATURES) == ["fmmt_adamw_batch_guarded", "fmmt_guard_commit", "fmmt_monitor_loss"]
    for other in (_lib.SIGNATURES, _lib.POOL_HEAD_SIGNATURES, _lib.RAGGED_SIGNATURES, _lib.EVAL_COLLECT_SIGNATURES, _lib.POOL_HEAD_ROWS_SIGNATURES):
        assert not set(_lib.GUARD_SIGNATURES) & set(other)

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    returns = {m.group(2): m.group(1) for m in re.finditer(r"\b(int|size_t)\s+(fmmt_\w+)\s*\(", src)}
    for name, args in protos.items():
        want = [ctype_of(a) for a in args.split(",") if a.strip()]
        res, got = _lib.GUARD_SIGNATURES[name]
        assert got == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g is not w], len(got), len(want))
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[returns[name]], name
    # the guarded update takes fmmt_adamw_batch's list, argument for argument
    assert len(_lib.SIGNATURES["fmmt_adamw_batch"][1]) == 13
    assert _lib.GUARD_SIGNATURES["fmmt_adamw_batch_guarded"][1][:13] == _lib.SIGNATURES["fmmt_adamw_batch"][1][:13]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in _lib.GUARD_SIGNATURES)
    lib = _lib_built()
    assert all(hasattr(lib, name) for name in _lib.GUARD_SIGNATURES)


def test_the_word_layout_is_the_headers():
    from facialmmt_amd import _lib
    src = open(os.path.join(ROOT, "include", "fmmt_guard.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+FMMT_GUARD_(\w+)\s+(\d+)", src)}
    assert header == {"LOSS_SUM": _lib.GUARD_LOSS_SUM, "MICRO_STEPS": _lib.GUARD_MICRO_STEPS, "NONFINITE_LOSSES": _lib.GUARD_NONFINITE_LOSSES,
                      "APPLIED": _lib.GUARD_APPLIED, "SKIPPED": _lib.GUARD_SKIPPED, "LAST_NORM": _lib.GUARD_LAST_NORM, "WORDS": _lib.GUARD_WORDS}
    assert sorted(v for k, v in header.items() if k != "WORDS") == list(range(header["WORDS"]))


def test_arguments_are_validated_before_any_launch():
    """FMMT_EINVAL / FMMT_EALIGN come back without a device: nothing is launched for a NULL norm, NULL or misaligned words, or an empty table"""
    from facialmmt_amd import _lib
    lib = _lib_built()
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    p += -p % 16

    def update(n_desc=1, n_blocks=1, desc=p, lr=p + 64, step=p + 68, norm=p + 72):
        return lib.fmmt_adamw_batch_guarded(n_desc, n_blocks, desc, lr, step, norm, 0.9, 0.999, 1e-6, 0.0, 1.0, 1, None)
    for bad in (dict(norm=None), dict(desc=None), dict(lr=None), dict(step=None), dict(n_desc=0), dict(n_blocks=0), dict(n_desc=-1), dict(n_blocks=-3)):
        assert update(**bad) == _lib.FMMT_EINVAL, bad

    def commit(norm=p + 72, step=p + 68, words=p + 128):
        return lib.fmmt_guard_commit(norm, step, words, None)
    for bad in (dict(norm=None), dict(step=None), dict(words=None)):
        assert commit(**bad) == _lib.FMMT_EINVAL, bad
    for off in (1, 2, 4, 12):
        assert commit(words=p + 128 + off) == _lib.FMMT_EALIGN, off

    def monitor(loss=p + 76, words=p + 128):
        return lib.fmmt_monitor_loss(loss, 2.0, words, None)
    for bad in (dict(loss=None), dict(words=None)):
        assert monitor(**bad) == _lib.FMMT_EINVAL, bad
    for off in (1, 4, 6):
        assert monitor(words=p + 128 + off) == _lib.FMMT_EALIGN, off


def _words(loss_sum=0.0, micro=0, nonfinite=0, applied=0, skipped=0, norm=0.0):
    w = np.zeros(6, dtype=np.int64)
    w[0] = np.array([loss_sum], dtype=np.float64).view(np.int64)[0]
    w[1:5] = (micro, nonfinite, applied, skipped)
    w[5] = int(np.array([norm], dtype=np.float32).view(np.uint32)[0])          # zero-extended, as the kernel stores it
    return w


def test_summarise_on_hand_made_words():
    from facialmmt_amd.train_step import TrainMonitor
    r = TrainMonitor.summarise(_words(4.5, 3, 1, 2, 1, 0.75))
    assert (r.avg_loss, r.loss_sum, r.micro_steps, r.nonfinite_losses, r.applied, r.skipped, r.last_norm) == (1.5, 4.5, 3, 1, 2, 1, 0.75)
    r = TrainMonitor.summarise(_words())                                        # nothing counted yet: NaN, not a division error
    assert math.isnan(r.avg_loss) and r.micro_steps == 0 and r.applied == r.skipped == r.nonfinite_losses == 0 and r.last_norm == 0.0
    r = TrainMonitor.summarise(_words(0.0, 0, 5, 0, 5, float("nan")))           # every loss was non-finite
    assert math.isnan(r.avg_loss) and r.nonfinite_losses == 5 and r.skipped == 5 and math.isnan(r.last_norm)
    assert TrainMonitor.summarise(_words(norm=float("inf"))).last_norm == float("inf")
    assert TrainMonitor.summarise(_words(norm=float("-inf"))).last_norm == float("-inf")       # sign bit set: the word stays non-negative
    assert int(_words(norm=float("-inf"))[5]) == 0xFF800000
    assert TrainMonitor.summarise(_words(1e300, 1).tolist()).avg_loss == 1e300                  # a plain list of ints is words too
    for bad in (np.zeros(5, dtype=np.int64), np.zeros((2, 3), dtype=np.int64)):
        with pytest.raises(ValueError):
            TrainMonitor.summarise(bad)
