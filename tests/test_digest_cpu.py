"""CPU tests of the replica digest: the ABI surface of include/fmmt_digest.h (header == _lib.DIGEST_SIGNATURES == the built library, argument validation
in front of any launch), the numpy restatement the GPU test uses (tests/support_digest.py) against hand-computed values, and the host half of
parallel.replicas_agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import support_digest as SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_built():
    from facialmmt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_digest_header_signatures_and_library_agree():
    """include/fmmt_digest.h (included by fmmt.h) == _lib.DIGEST_SIGNATURES == the symbols of the built library: names, every argument's type and the
    return type; the table is disjoint from the six that exist, and _lib.SIGNATURES keeps its 59 names"""
    from facialmmt_amd import _lib, build
    assert "digest.hip" in build.SOURCES
    assert '#include "fmmt_digest.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmmt_digest.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.DIGEST_SIGNATURES) == ["fmmt_param_digest"]
    for other in (_lib.SIGNATURES, _lib.POOL_HEAD_SIGNATURES, _lib.RAGGED_SIGNATURES, _lib.EVAL_COLLECT_SIGNATURES, _lib.POOL_HEAD_ROWS_SIGNATURES,
                  _lib.GUARD_SIGNATURES):
        assert not set(_lib.DIGEST_SIGNATURES) & set(other)
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
        res, got = _lib.DIGEST_SIGNATURES[name]
        assert got == want, (name, got, want)
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[returns[name]], name
    # the table argument is fmmt_adamw_batch's: (n_desc, n_blocks, desc) in front
    assert _lib.DIGEST_SIGNATURES["fmmt_param_digest"][1][:3] == _lib.SIGNATURES["fmmt_adamw_batch"][1][:3]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fmmt_param_digest" in text and "fmmt_digest.h" in text
    lib = _lib_built()
    assert all(hasattr(lib, name) for name in _lib.DIGEST_SIGNATURES)


def test_arguments_are_validated_before_any_launch():
    """FMMT_EINVAL / FMMT_EALIGN come back without a device: nothing is launched for a NULL table, partial or out, an empty table, or misaligned words"""
    from facialmmt_amd import _lib
    lib = _lib_built()
    buf = (C.c_char * 512)()
    p = C.addressof(buf)
    p += -p % 16

    def call(n_desc=1, n_blocks=1, desc=p, partial=p + 128, out=p + 256):
        return lib.fmmt_param_digest(n_desc, n_blocks, desc, partial, out, None)
    for bad in (dict(desc=None), dict(partial=None), dict(out=None), dict(n_desc=0), dict(n_desc=-2), dict(n_blocks=0), dict(n_blocks=-1)):
        assert call(**bad) == _lib.FMMT_EINVAL, bad
    for off in (1, 2, 4, 6, 12):
        assert call(partial=p + 128 + off) == _lib.FMMT_EALIGN, off
        assert call(out=p + 256 + off) == _lib.FMMT_EALIGN, off
    assert call(n_desc=0, out=p + 257) == _lib.FMMT_EINVAL                  # the count is looked at first


def test_the_numpy_restatement_on_values_worked_by_hand():
    """bits of 1.0f = 0x3F800000, of 2.0f = 0x40000000, of -0.0f = 0x80000000"""
    one, two, negzero = 0x3F800000, 0x40000000, 0x80000000
    a = np.array([1.0, 2.0], dtype=np.float32)
    assert SD.sums([a]) == (one + two, one * (1 + (1 << 32)) + two * (2 + (1 << 32)))
    b = np.array([-0.0], dtype=np.float32)
    s1, s2 = SD.sums([a, b])                                                # second tensor: j = 1, weight (i + 1) + 2 * 2^32
    assert s1 == one + two + negzero
    assert s2 == (one * (1 + (1 << 32)) + two * (2 + (1 << 32)) + negzero * (1 + (2 << 32))) % (1 << 64)
    assert SD.sums([np.zeros(5, dtype=np.float32)]) == (0, 0)
    assert SD.sums([np.array([0.0], dtype=np.float32)]) != SD.sums([b])     # +0.0 against -0.0
    assert SD.sums([a])[0] == SD.sums([a[::-1]])[0] and SD.sums([a])[1] != SD.sums([a[::-1]])[1]       # a swap: S2 alone
    # the wrap: 2^20 elements of all-ones bits, S1 = 2^20 * (2^32 - 1), S2 in exact integers
    n = 1 << 20
    e = (1 << 32) - 1
    big = np.full(n, e, dtype=np.uint32).view(np.float32)
    assert SD.sums([big]) == (n * e, e * (n * (n + 1) // 2 + n * (1 << 32)) % (1 << 64))
    assert SD.as_unsigned(np.array([-1, 5], dtype=np.int64)) == [(1 << 64) - 1, 5]
    words = SD.digest([a], [b], [a, b])
    assert words[:2] == list(SD.sums([a])) and words[2:4] == list(SD.sums([b])) and words[4:] == list(SD.sums([a, b]))


def test_the_hand_built_table_is_the_optimizers_record():
    """tests/support_digest.table lays records out as train_step.FusedClipAdamW does: 56 bytes (five pointers, a 64-bit count, two ints), blocks of 4096 elements"""
    raw, blocks = SD.table([(16, 32, 48, 64, 1), (80, 96, 112, 128, 4097), (144, 160, 176, 192, 4096)])
    assert SD.DESC_DTYPE.itemsize == 56 and raw.size == 3 * 56 and blocks == 1 + 2 + 1
    rec = raw.view(SD.DESC_DTYPE)
    assert rec["bb"].tolist() == [0, 1, 3] and rec["n"].tolist() == [1, 4097, 4096] and rec["low"].tolist() == [0, 0, 0]
    src = open(os.path.join(ROOT, "facialmmt_amd", "train_step.py")).read()
    assert '[("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("low", "<u8"), ("n", "<i8"), ("bb", "<i4"), ("pad", "<i4")]' in src


def test_replicas_agree_at_world_size_one_needs_no_process_group():
    import torch
    from facialmmt_amd import parallel
    d = torch.tensor([1, -2, 3, 4, 5, 6], dtype=torch.int64)
    got = parallel.replicas_agree(d)
    assert len(got) == 1 and torch.equal(got[0], d)
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros(6, dtype=torch.int32)):
        with pytest.raises(ValueError):
            parallel.replicas_agree(bad)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _agree_worker(rank, world, port, ret):
    from datetime import timedelta
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    from facialmmt_amd import parallel
    same = torch.tensor([7, -1, 2, 3, 1 << 62, 5], dtype=torch.int64)
    got = parallel.replicas_agree(same)
    out = {"same": [g.tolist() for g in got]}
    mine = same.clone()
    if rank == 1:
        mine[3] += 1                                        # the first moments' S2 on rank 1 alone
        mine[5] += 1
    try:
        parallel.replicas_agree(mine)
        out["error"] = None
    except RuntimeError as e:
        out["error"] = str(e)
    ret[rank] = out
    dist.destroy_process_group()


def test_replicas_agree_names_the_first_rank_and_word_that_differ():
    """two gloo ranks on the CPU: equal digests come back as the list of both; a digest that differs on rank 1 raises on EVERY rank, naming rank 1 and
    word 3 (the first that differs, not word 5)"""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_agree_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    for r in range(2):
        assert ret[r]["same"] == [[7, -1, 2, 3, 1 << 62, 5]] * 2
        assert ret[r]["error"] is not None and "rank 1" in ret[r]["error"] and "word 3" in ret[r]["error"] and "first moments S2" in ret[r]["error"]
        assert "word 5" not in ret[r]["error"]
