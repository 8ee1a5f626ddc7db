"""CPU tests of sharded evaluation: parallel.eval_shard / eval_collect_rows as pure functions, the ABI surface of include/fmmt_eval_shard.h (header ==
_lib.EVAL_SHARD_SIGNATURES == the built library, argument validation in front of any launch), the host half of MeldMetrics.gather_merge on two gloo
ranks, and the numpy restatement of the merge (tests/support_eval_shard.py) that the GPU tests use as their oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import support_eval_shard as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1109, 2610])
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_shards_partition_the_split_in_whole_batches(n, B, W):
    from facialmmt_amd import parallel
    shards = [parallel.eval_shard(n, B, r, W) for r in range(W)]
    cap = parallel.eval_collect_rows(n, B, W)
    assert [i for s in shards for i in s] == list(range(n))                        # a partition, in order
    assert all(s.step == 1 and s.start % B == 0 for s in shards)
    assert all(len(s) <= cap for s in shards) and cap % B == 0
    ragged = [r for r, s in enumerate(shards) if len(s) % B]
    nonempty = [r for r, s in enumerate(shards) if len(s)]
    assert len(ragged) <= 1 and (not ragged or ragged[0] == nonempty[-1])
    # every batch a rank forms is a batch of the single-rank loader
    single = [list(range(i, min(i + B, n))) for i in range(0, n, B)]
    mine = [list(s[i:i + B]) for s in shards for i in range(0, len(s), B)]
    assert mine == single
    assert cap == -(-(-(-n // B)) // W) * B                                         # ceil(ceil(n / B) / W) * B


def test_shard_arguments_and_defaults():
    from facialmmt_amd import parallel
    assert parallel.eval_shard(9, 2, 0, 2) == range(0, 6) and parallel.eval_shard(9, 2, 1, 2) == range(6, 9) and parallel.eval_collect_rows(9, 2, 2) == 6
    assert parallel.eval_shard(2, 2, 1, 2) == range(2, 2) and parallel.eval_collect_rows(2, 2, 2) == 2
    assert parallel.eval_shard(11, 4) == range(0, 11)                               # no process group: rank 0 of 1
    assert parallel.eval_shard(0, 4, 0, 2) == range(0, 0) and parallel.eval_collect_rows(0, 4, 2) == 0
    for bad in ((5, 0, 0, 1), (5, 2, 2, 2), (5, 2, -1, 2), (-1, 2, 0, 1), (5, 2, 0, 0)):
        with pytest.raises(ValueError):
            parallel.eval_shard(*bad)


def _lib_built():
    from facialmmt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_eval_shard_header_signatures_and_library_agree():
    """include/fmmt_eval_shard.h (included by fmmt.h) == _lib.EVAL_SHARD_SIGNATURES == the symbols of the built library: names, every argument's type and
    the return type, as tests/test_digest_cpu.py::test_digest_header_signatures_and_library_agree does; the table is disjoint from the seven that exist"""
    from facialmmt_amd import _lib, build
    assert "eval_shard.hip" in build.SOURCES and "eval.hip" in build.SOURCES
    assert '#include "fmmt_eval_shard.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmmt_eval_shard.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.EVAL_SHARD_SIGNATURES) == ["fmmt_eval_accumulate_rows", "fmmt_eval_merge"]
    for other in (_lib.SIGNATURES, _lib.POOL_HEAD_SIGNATURES, _lib.RAGGED_SIGNATURES, _lib.EVAL_COLLECT_SIGNATURES, _lib.POOL_HEAD_ROWS_SIGNATURES,
                  _lib.GUARD_SIGNATURES, _lib.DIGEST_SIGNATURES):
        assert not set(_lib.EVAL_SHARD_SIGNATURES) & set(other)
    assert len(_lib.SIGNATURES) == 59

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    returns = {m.group(2): m.group(1) for m in re.finditer(r"\b(int|size_t)\s+(fmmt_\w+)\s*\(", src)}
    for name, args in protos.items():
        want = [ctype_of(a) for a in args.split(",") if a.strip()]
        res, got = _lib.EVAL_SHARD_SIGNATURES[name]
        assert got == want, (name, got, want)
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[returns[name]], name
    # fmmt_eval_accumulate_at's list with n_rows put in behind the cursor
    rows = list(_lib.EVAL_SHARD_SIGNATURES["fmmt_eval_accumulate_rows"][1])
    assert rows.pop(10) is C.c_void_p and rows == _lib.EVAL_COLLECT_SIGNATURES["fmmt_eval_accumulate_at"][1]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in _lib.EVAL_SHARD_SIGNATURES) and "fmmt_eval_shard.h" in text
    lib = _lib_built()
    assert all(hasattr(lib, name) for name in _lib.EVAL_SHARD_SIGNATURES)


def test_arguments_are_validated_before_any_launch():
    """FMMT_EINVAL / FMMT_EALIGN come back without a device, by the neighbour's rules plus the new word's"""
    from facialmmt_amd import _lib
    lib = _lib_built()
    buf = (C.c_char * 512)()
    p = C.addressof(buf)
    p += -p % 16

    def rows(dtype=0, B=4, NL=7, logits=p, ld=7, labels=p, loss=p, count=p + 8, conf=p + 16, cursor=p + 128, n_rows=p + 136, lo=p, la=p, pr=None, cap=8):
        return lib.fmmt_eval_accumulate_rows(dtype, B, NL, logits, ld, labels, loss, count, conf, cursor, n_rows, lo, la, pr, cap, None)
    for bad in (dict(B=0), dict(B=1025), dict(NL=0), dict(NL=9), dict(ld=6), dict(cap=-1), dict(dtype=5), dict(cursor=None), dict(n_rows=None), dict(lo=None),
                dict(la=None), dict(logits=None), dict(labels=None), dict(loss=None), dict(count=None), dict(conf=None)):
        assert rows(**bad) == _lib.FMMT_EINVAL, bad
    for bad in (dict(cursor=p + 132), dict(la=p + 4), dict(labels=p + 4), dict(loss=p + 4), dict(count=p + 12), dict(conf=p + 20), dict(n_rows=p + 137),
                dict(n_rows=p + 138)):
        assert rows(**bad) == _lib.FMMT_EALIGN, bad
    assert rows(n_rows=None, cursor=p + 132) == _lib.FMMT_EINVAL                     # NULL is looked at first

    def merge(W=2, NL=7, cap=8, out_cap=16, words=p, results=p, truths=p, words_out=p + 256, results_out=p + 256, truths_out=p + 256):
        return lib.fmmt_eval_merge(W, NL, cap, out_cap, words, results, truths, words_out, results_out, truths_out, None)
    for bad in (dict(W=0), dict(W=65), dict(NL=0), dict(NL=9), dict(cap=-1), dict(out_cap=-1), dict(words=None), dict(results=None), dict(truths=None),
                dict(words_out=None), dict(results_out=None), dict(truths_out=None)):
        assert merge(**bad) == _lib.FMMT_EINVAL, bad
    for bad in (dict(words=p + 4), dict(truths=p + 4), dict(words_out=p + 260), dict(truths_out=p + 260), dict(results=p + 2), dict(results_out=p + 257)):
        assert merge(**bad) == _lib.FMMT_EALIGN, bad


def test_front_ends_refuse_cpu_tensors():
    """the merge and the row update are GPU-only, as every hot-path entry: no CPU or PyTorch fall-back"""
    import torch
    from facialmmt_amd import _lib, ops
    nl = 3
    w = torch.zeros(2, SE.n_words(nl), dtype=torch.int64)
    with pytest.raises(_lib.FmmtError):
        ops.eval_merge(w, torch.zeros(2, 4, nl), torch.zeros(2, 4, dtype=torch.int64), w[0].clone(), torch.zeros(8, nl), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(_lib.FmmtError):
        ops.eval_accumulate_rows(torch.zeros(2, nl), torch.zeros(2, dtype=torch.int64), w[0, :-1], w[0, -1:], torch.zeros(1, dtype=torch.int32), torch.zeros(4, nl),
                                 torch.zeros(4, dtype=torch.int64))


def test_the_numpy_restatement_against_a_single_pass_over_the_rows():
    """random shards: the merged split is what ONE pass over the concatenated real rows gives -- rows and labels in rank order, count and confusion of all
    of them, the loss sum the left-to-right sum of the ranks' sums -- and nothing behind the total is written"""
    rng = np.random.default_rng(7)
    for nl, cursors in ((7, [8, 5, 0, 8, 1]), (3, [4]), (3, [0, 0]), (7, [1, 8, 8])):
        cap = 8
        words, results, truths = SE.fabricate(rng, cursors, cap, nl)
        out_cap = len(cursors) * cap
        wo = np.full(SE.n_words(nl), -5, dtype=np.int64)
        ro = np.full((out_cap, nl), -9.0, dtype=np.float32)
        to = np.full(out_cap, -9, dtype=np.int64)
        SE.merge(words, results, truths, wo, ro, to)
        rows = np.concatenate([results[r, :c] for r, c in enumerate(cursors)])
        labels = np.concatenate([truths[r, :c] for r, c in enumerate(cursors)])
        total = sum(cursors)
        assert np.array_equal(ro[:total], rows) and np.array_equal(to[:total], labels) and int(wo[-1]) == total
        assert np.all(ro[total:] == -9.0) and np.all(to[total:] == -9)
        assert not np.any(ro[:total] == np.float32(1e30))
        ok = labels >= 0
        conf = np.zeros((nl, nl), dtype=np.int64)
        np.add.at(conf, (labels[ok], rows.argmax(axis=1)[ok]), 1)
        assert int(wo[1]) == int(ok.sum()) and np.array_equal(wo[2:-1].reshape(nl, nl), conf)
        want = 0.0
        for r, c in enumerate(cursors):
            if c > 0:
                want = want + float(words[r, :1].view(np.float64)[0])
        assert wo[:1].view(np.float64)[0] == want
        m = rows.max(axis=1) if total else np.zeros(0)
        direct = ((m + np.log(np.exp(rows - m[:, None]).sum(axis=1))) - rows[np.arange(total), np.where(ok, labels, 0)])[ok].astype(np.float64).sum() if total else 0.0
        assert abs(want - direct) <= 1e-12 * max(1.0, abs(direct))                  # another association of the same fp64 terms


def test_the_numpy_restatement_reports_both_overflows():
    rng = np.random.default_rng(8)
    nl, cap = 3, 8
    words, results, truths = SE.fabricate(rng, [5, cap + 3, 2], cap, nl)             # a rank that overflowed its own buffers
    wo, ro, to = np.zeros(SE.n_words(nl), dtype=np.int64), np.full((24, nl), -9.0, dtype=np.float32), np.full(24, -9, dtype=np.int64)
    SE.merge(words, results, truths, wo, ro, to)
    assert int(wo[-1]) == 24 + 3 and np.array_equal(ro[5:13], results[1]) and np.array_equal(ro[13:15], results[2, :2]) and np.all(ro[15:] == -9.0)
    assert int(wo[1]) == int(words[:, 1].sum())                                      # the dropped rows are counted, as one rank counts them
    words, results, truths = SE.fabricate(rng, [8, 5, 1], cap, nl)                   # outputs smaller than the total
    wo, ro, to = np.zeros(SE.n_words(nl), dtype=np.int64), np.full((10, nl), -9.0, dtype=np.float32), np.full(10, -9, dtype=np.int64)
    SE.merge(words, results, truths, wo, ro, to)
    assert int(wo[-1]) == 10 + 4 and np.array_equal(ro[:8], results[0]) and np.array_equal(ro[8:], results[1, :2]) and np.array_equal(to[8:], truths[1, :2])
    from facialmmt_amd.eval_step import MeldMetrics
    with pytest.raises(ValueError, match="14 rows.*collect_rows=10"):
        MeldMetrics.collected_count(wo, 10)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _mismatch_worker(rank, world, port, ret):
    from datetime import timedelta
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    from facialmmt_amd.eval_step import MeldMetrics
    m = MeldMetrics(3, "cpu", collect_rows=6 if rank == 0 else 8)
    try:
        m.gather_merge()
        ret[rank] = None
    except ValueError as e:
        ret[rank] = str(e)
    dist.destroy_process_group()


def test_a_collect_rows_mismatch_raises_on_both_ranks_before_the_large_gather():
    """two gloo ranks on CPU tensors: the small all-gather carries collect_rows, and the rank that is right raises as well"""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_mismatch_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    for r in range(2):
        assert ret[r] is not None and "collect_rows" in ret[r] and "[6, 8]" in ret[r], ret[r]


def test_gather_merge_and_sharded_evaluate_want_collecting_metrics():
    from facialmmt_amd.eval_step import MeldMetrics, evaluate
    import types
    m = MeldMetrics(3, "cpu")
    with pytest.raises(ValueError, match="collect"):
        m.gather_merge()
    with pytest.raises(ValueError, match="collect"):
        evaluate(types.SimpleNamespace(metrics=m), [], sharded=True)
