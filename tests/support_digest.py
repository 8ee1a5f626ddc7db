"""The replica digest (include/fmmt_digest.h) restated in numpy uint64 arithmetic, and the descriptor table fmmt_adamw_batch / fmmt_param_digest
take, built by hand: what tests/test_digest_cpu.py checks on its own and tests/test_gpu_digest.py holds the kernel to."""
import numpy as np

DESC_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("low", "<u8"), ("n", "<i8"), ("bb", "<i4"), ("pad", "<i4")])
BLOCK = 4096


def sums(arrays):
    """(S1, S2) over a list of float32 arrays, tensor j = position in the list: S1 = sum of the elements' 32 bits, S2 = sum of bits * ((i + 1) +
    (j + 1) * 2^32), both mod 2^64 (numpy's uint64 arithmetic wraps)"""
    s1 = s2 = np.uint64(0)
    with np.errstate(over="ignore"):
        for j, a in enumerate(arrays):
            e = np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
            w = np.arange(1, e.size + 1, dtype=np.uint64) + (np.uint64(j + 1) << np.uint64(32))
            s1 = s1 + e.sum(dtype=np.uint64)
            s2 = s2 + (e * w).sum(dtype=np.uint64)
    return int(s1), int(s2)


def digest(ps, ms, vs):
    """the six words as Python ints in [0, 2^64): p S1, p S2, m S1, m S2, v S1, v S2"""
    return [w for arrays in (ps, ms, vs) for w in sums(arrays)]


def as_unsigned(words):
    """the int64 words a device digest comes back as -> Python ints in [0, 2^64)"""
    return [int(w) & 0xFFFFFFFFFFFFFFFF for w in np.asarray(words, dtype=np.int64).tolist()]


def table(ptrs):
    """descriptor records for [(p, g, m, v, n), ...] (addresses as ints) -> (uint8 array of the records, number of 4096-element blocks)"""
    arr = np.zeros(len(ptrs), dtype=DESC_DTYPE)
    blocks = 0
    for i, (p, g, m, v, n) in enumerate(ptrs):
        arr[i] = (p, g, m, v, 0, n, blocks, 0)
        blocks += (n + BLOCK - 1) // BLOCK
    return arr.view(np.uint8).copy(), blocks
