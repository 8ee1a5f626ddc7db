"""GPU tests of fmmt_table_stats alone (csrc/table_stats.hip, include/fmmt_stats.h) through ops.table_stats, on ONE hand-built table of nine records.

Record sizes 1, 3, 4, 5, 4095, 4096, 4097, 12293 and 8192: below one 16-byte load, a quad exactly, one past it, one short of a block, a block, one past
it (a one-element tail block), several blocks with a tail, two blocks exactly -- the block boundaries are where the record search and the tails can go
wrong.  The 4095 record starts 4 bytes off a 16-byte boundary in all four fields (no vector load anywhere in it); the 12293 record's GRADIENT is bf16
(`g_is_bf16 = 1`) and starts 2 bytes off an 8-byte boundary; everything else is aligned.  Planted in every field: a NaN as the last element of the 4097
record, -inf in the 5 record, two 3e19 in the 4096 record (sumsq overflows to inf, nonfinite stays 0), 1e-40 and -0.0 in the 3 record.

Reference: torch in fp64 on the same values, computed once per field.  max_abs bit-equal, nonfinite equal, sumsq within a relative (n + 2) * 2^-24 where
it is finite -- the worst-case bound of an fp32 sum of n non-negative terms in any order, so it holds for whatever tree the kernel uses -- and inf / NaN
exactly.  Every comparison prints its figures first (run with -s)."""
import numpy as np
import pytest
import torch

from tests import support_digest as SD

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 12293, 8192)
I_3, I_5, I_4095, I_4096, I_4097, I_BF16 = 1, 3, 4, 5, 6, 7
FIELDS = ("g", "p", "m", "v")                                # FMMT_STATS_G .. _V
SENTINEL = 0x5A5A5A5A
_CACHE = {}


def _values(k, j, n):
    g = torch.Generator().manual_seed(1000 * k + j)
    x = torch.randn(n, generator=g, dtype=torch.float32) * (0.5 + j)
    if j == I_3:
        x[0], x[2] = 1e-40, -0.0
    if j == I_5:
        x[2] = float("-inf")
    if j == I_4096:
        x[17], x[4000] = 3e19, 3e19
    if j == I_4097:
        x[4096] = float("nan")
    return x


def _table(dev):
    """the table, built once and never modified: host values per field (what the kernel reads, as fp32), the device tensors, the descriptor"""
    if "t" in _CACHE:
        return _CACHE["t"]
    host = {f: [] for f in FIELDS}
    on_dev = {f: [] for f in FIELDS}
    for k, f in enumerate(FIELDS):
        for j, n in enumerate(SIZES):
            x = _values(k, j, n)
            if f == "g" and j == I_BF16:                     # 2 bytes off an 8-byte boundary: one bf16 element into a fresh allocation
                low = x.to(torch.bfloat16)
                t = torch.cat((torch.zeros(1, dtype=torch.bfloat16), low)).to(dev)[1:]
                assert t.data_ptr() % 8 == 2
                x = low.float()                               # exact: what the kernel must see
            elif j == I_4095:                                 # 4 bytes off a 16-byte boundary
                t = torch.cat((torch.zeros(1), x)).to(dev)[1:]
                assert t.data_ptr() % 16 == 4
            else:
                t = x.to(dev)
                assert t.data_ptr() % 16 == 0
            host[f].append(x)
            on_dev[f].append(t)
    arr = np.zeros(len(SIZES), dtype=SD.DESC_DTYPE)
    blocks = 0
    for j, n in enumerate(SIZES):
        arr[j] = (on_dev["p"][j].data_ptr(), on_dev["g"][j].data_ptr(), on_dev["m"][j].data_ptr(), on_dev["v"][j].data_ptr(), 0, n, blocks,
                  1 if j == I_BF16 else 0)
        blocks += (n + SD.BLOCK - 1) // SD.BLOCK
    assert blocks == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 4 + 2
    desc = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
    _CACHE["t"] = (host, on_dev, desc, blocks)
    return _CACHE["t"]


def _reference(values):
    """per record (sumsq, max_abs, nonfinite) in fp64 from the fp32 values"""
    out = []
    for x in values:
        d = x.double()
        keep = d[~torch.isnan(d)]
        out.append((float((d * d).sum()), float(keep.abs().max()) if keep.numel() else 0.0, int((~torch.isfinite(d)).sum())))
    return out


def _want(f, dev):
    if ("ref", f) not in _CACHE:
        _CACHE[("ref", f)] = _reference(_table(dev)[0][f])
    return _CACHE[("ref", f)]


def _buffers(dev, n, blocks, pad=4):
    """(partial, stats, bad_stats) with `pad` sentinel rows behind each, and the two words"""
    def rows(k):
        return torch.full((k + pad, 4), SENTINEL, dtype=torch.int32, device=dev)
    return rows(blocks), rows(n), rows(n), torch.zeros(2, dtype=torch.int64, device=dev)


def _decode(stats, n):
    from facialmmt_amd import _lib
    return stats[:n].cpu().numpy().view(np.dtype(_lib.STATS_FIELDS)).reshape(n)


def _check(got, want, sizes, label):
    FLT_MAX = float(np.finfo(np.float32).max)
    for j, (n, (s, m, k)) in enumerate(zip(sizes, want)):
        gs, gm, gk = float(got["sumsq"][j]), got["max_abs"][j], int(got["nonfinite"][j])
        print(f"{label} record {j} n {n}: sumsq {gs!r} want {s!r}  max_abs {float(gm)!r} want {m!r}  nonfinite {gk} want {k}")
        assert int(got["reserved"][j]) == 0
        assert gk == k
        assert np.float32(gm).view(np.uint32) == np.float32(m).view(np.uint32)          # bit-equal (fp64 -> fp32 of an fp32 value is exact)
        if s != s:
            assert gs != gs
        elif s == float("inf") or s > FLT_MAX:                  # infinite, or past what fp32 holds: the fp32 sum is inf
            assert gs == float("inf")
        else:
            assert abs(gs - s) <= (n + 2) * 2.0 ** -24 * s, (j, gs, s)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("which", range(4), ids=FIELDS)
def test_every_field_against_fp64(dev, which):
    from facialmmt_amd import ops
    host, _, desc, blocks = _table(dev)
    n = len(SIZES)
    partial, stats, _, _ = _buffers(dev, n, blocks)
    assert ops.table_stats(which, n, blocks, desc, partial, stats) is stats
    got = _decode(stats, n)
    want = _want(FIELDS[which], dev)
    _check(got, want, SIZES, FIELDS[which])
    # the planted values did what they were planted for
    assert want[I_4097][2] == 1 and want[I_5][1] == float("inf") and want[I_5][2] == 1 and want[I_4096][2] == 0
    assert got["sumsq"][I_4096] == np.inf and np.isnan(got["sumsq"][I_4097]) and got["max_abs"][I_4097] > 0
    assert got["max_abs"][I_3] > 0 and got["nonfinite"][I_3] == 0
    assert bool((partial[blocks:] == SENTINEL).all()) and bool((stats[n:] == SENTINEL).all())
    # again: the same bits, partials included
    first, first_partial = stats.clone(), partial.clone()
    stats[:n].zero_()
    ops.table_stats(which, n, blocks, desc, partial, stats)
    assert torch.equal(stats, first) and torch.equal(partial, first_partial)


def test_a_table_of_one_record(dev):
    """n_desc = 1, each record of the table in turn as a table of its own (blk_begin 0): the search's lower end and the finish's upper end"""
    from facialmmt_amd import ops
    _, on_dev, desc, _ = _table(dev)
    rec = desc.cpu().numpy().view(SD.DESC_DTYPE).copy()
    want = _want("g", dev)
    for j in (0, I_4097, I_BF16, len(SIZES) - 1):
        one = rec[j:j + 1].copy()
        one["bb"] = 0
        blocks = (SIZES[j] + SD.BLOCK - 1) // SD.BLOCK
        partial, stats, _, _ = _buffers(dev, 1, blocks)
        ops.table_stats(0, 1, blocks, torch.from_numpy(one.view(np.uint8).copy()).to(dev), partial, stats)
        _check(_decode(stats, 1), want[j:j + 1], SIZES[j:j + 1], f"alone {j}")
        assert bool((partial[blocks:] == SENTINEL).all()) and bool((stats[1:] == SENTINEL).all())


def _clean_table(dev):
    """three finite records (4097, 5, 8192 elements) whose values a test may change: (tensors, desc, blocks)"""
    sizes = (4097, 5, 8192)
    g = torch.Generator().manual_seed(77)
    ts = [torch.randn(n, generator=g).to(dev) for n in sizes]
    raw, blocks = SD.table([(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.numel()) for t in ts])
    return sizes, ts, torch.from_numpy(raw).to(dev), blocks


def test_the_snapshot_follows_the_norm_word(dev):
    from facialmmt_amd import ops
    sizes, ts, desc, blocks = _clean_table(dev)
    n = len(sizes)
    partial, stats, bad, words = _buffers(dev, n, blocks)
    norm = torch.tensor(3.5, device=dev)
    ops.table_stats(0, n, blocks, desc, partial, stats, norm=norm, bad_stats=bad, bad_words=words)
    assert bool((bad == SENTINEL).all()) and words.tolist() == [0, 0]       # finite norm: nothing of the snapshot is touched
    _check(_decode(stats, n), _reference([t.cpu() for t in ts]), sizes, "clean")
    seen = 0
    for value, plant in ((float("nan"), (2, 8191, float("nan"))), (float("inf"), (1, 0, float("inf"))), (float("-inf"), None)):
        norm.fill_(value)
        old = None
        if plant is not None:
            j, i, v = plant
            old = ts[j][i].clone()
            ts[j][i] = v
        ops.table_stats(0, n, blocks, desc, partial, stats, norm=norm, bad_stats=bad, bad_words=words)
        seen += 1
        got = words.tolist()
        print("norm", value, "planted", plant, "words", got)
        assert torch.equal(bad[:n], stats[:n]) and bool((bad[n:] == SENTINEL).all()) and bool((stats[n:] == SENTINEL).all())
        assert got == [seen, plant[0] if plant is not None else -1]
        _check(_decode(stats, n), _reference([t.cpu() for t in ts]), sizes, f"norm {value}")
        if plant is not None:
            ts[plant[0]][plant[1]] = old
    # two offenders: the LOWEST record is named; and an overflowing sum of finite values counts as one
    ts[2][5], ts[0][4096] = float("nan"), 3e19
    ts[0][0] = 3e19
    norm.fill_(float("nan"))
    ops.table_stats(0, n, blocks, desc, partial, stats, norm=norm, bad_stats=bad, bad_words=words)
    d = _decode(bad, n)
    assert words.tolist() == [seen + 1, 0] and d["sumsq"][0] == np.inf and d["nonfinite"].tolist() == [0, 0, 1]
    # a finite norm again: stats move on, the snapshot and the words stay
    ts[2][5], ts[0][4096], ts[0][0] = 0.0, 0.0, 0.0
    norm.fill_(1.0)
    kept = bad.clone()
    ops.table_stats(0, n, blocks, desc, partial, stats, norm=norm, bad_stats=bad, bad_words=words)
    assert torch.equal(bad, kept) and words.tolist() == [seen + 1, 0] and int(_decode(stats, n)["nonfinite"].sum()) == 0
    assert bool((partial[blocks:] == SENTINEL).all())


def test_ops_table_stats_checks_its_buffers(dev):
    from facialmmt_amd import ops
    sizes, ts, desc, blocks = _clean_table(dev)
    n = len(sizes)
    partial, stats, bad, words = _buffers(dev, n, blocks, pad=0)
    norm = torch.tensor(1.0, device=dev)
    for kw in (dict(bad_stats=bad), dict(bad_words=words)):                 # a snapshot without the norm word
        with pytest.raises(ValueError):
            ops.table_stats(0, n, blocks, desc, partial, stats, **kw)
    for kw in (dict(partial=partial[:blocks - 1]), dict(stats=stats[:n - 1]), dict(stats=stats.view(torch.float32)), dict(stats=stats.reshape(-1))):
        with pytest.raises(ValueError):
            ops.table_stats(0, n, blocks, desc, **dict(dict(partial=partial, stats=stats), **kw))
    with pytest.raises(ValueError):
        ops.table_stats(0, n, blocks, desc, partial, stats, norm=norm, bad_stats=bad, bad_words=torch.zeros(3, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.table_stats(0, n, blocks, desc, partial, stats, norm=norm.double())


def test_captured_call_follows_changed_inputs(dev):
    """the call inside a torch.cuda.graph, replayed twice on changed values and a changed norm word"""
    from facialmmt_amd import ops
    sizes, ts, desc, blocks = _clean_table(dev)
    n = len(sizes)
    partial, stats, bad, words = _buffers(dev, n, blocks)
    norm = torch.tensor(2.0, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.table_stats(0, n, blocks, desc, partial, stats, norm=norm, bad_stats=bad, bad_words=words)          # loads the module outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.table_stats(0, n, blocks, desc, partial, stats, norm=norm, bad_stats=bad, bad_words=words)
    assert words.tolist() == [0, 0]
    ts[0].mul_(3.0)
    ts[1][4] = 1e4
    graph.replay()
    _check(_decode(stats, n), _reference([t.cpu() for t in ts]), sizes, "replay 1")
    assert words.tolist() == [0, 0] and bool((bad == SENTINEL).all())
    ts[2][4095] = float("inf")
    norm.fill_(float("inf"))
    graph.replay()
    _check(_decode(stats, n), _reference([t.cpu() for t in ts]), sizes, "replay 2")
    assert words.tolist() == [1, 2] and torch.equal(bad[:n], stats[:n]) and bool((bad[n:] == SENTINEL).all())
