"""GPU tests of fmmt_eval_merge (csrc/eval_shard.hip, include/fmmt_eval_shard.h) alone: one process, gathers fabricated on the host
(tests/support_eval_shard.fabricate: real rows random, every row behind a rank's cursor poisoned), outputs pre-filled with a sentinel.  Everything
is compared EXACTLY with the numpy restatement (tests/support_eval_shard.merge, pinned by tests/test_eval_shard_cpu.py): the kernel moves rows and adds
integers, and its one floating-point sum has a fixed order."""
import numpy as np
import pytest
import torch

from facialmmt_amd import _lib, ops
from tests import support_eval_shard as SE

pytestmark = pytest.mark.gpu

CAP = 8
CURSORS = {1: [5], 2: [8, 3], 3: [0, 8, 1], 5: [8, 5, 0, 8, 1]}                # a full rank, an empty rank, a single row
SENTINEL = -9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import facialmmt_amd.torch_ops  # noqa: F401
    return torch.device("cuda:0")


def _outputs(nl, out_cap):
    return (np.full(SE.n_words(nl), SENTINEL, dtype=np.int64), np.full((out_cap, nl), float(SENTINEL), dtype=np.float32),
            np.full(out_cap, SENTINEL, dtype=np.int64))


def _run(dev, gathered, outputs, fn=None):
    ins = [torch.from_numpy(a).to(dev) for a in gathered]
    outs = [torch.from_numpy(a.copy()).to(dev) for a in outputs]
    assert (fn or ops.eval_merge)(*ins, *outs) is None
    assert all(torch.equal(t.cpu(), torch.from_numpy(a)) for t, a in zip(ins, gathered))          # the inputs are read only
    return [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("nl", [7, 3])
@pytest.mark.parametrize("W", [1, 2, 3, 5])
def test_merged_split_equals_the_numpy_restatement_exactly(dev, W, nl):
    rng = np.random.default_rng(10 * W + nl)
    cursors = CURSORS[W]
    gathered = SE.fabricate(rng, cursors, CAP, nl)
    want = _outputs(nl, W * CAP)
    SE.merge(*gathered, *want)
    got = _run(dev, gathered, _outputs(nl, W * CAP))
    total = sum(cursors)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()                                   # rows, truths, count, confusion, cursor and the loss sum's BITS
    assert int(got[0][-1]) == total and int(got[0][1]) == int(gathered[0][:, 1].sum())
    # the loss sum: Python's left-to-right fp64 sum of the ranks that hold rows
    py = None
    for r, c in enumerate(cursors):
        if c > 0:
            l = float(gathered[0][r, :1].view(np.float64)[0])
            py = l if py is None else py + l
    assert got[0][:1].view(np.float64)[0] == py and np.array([py]).view(np.int64)[0] == got[0][0]
    assert np.all(got[1][total:] == SENTINEL) and np.all(got[2][total:] == SENTINEL)              # the sentinel behind the total
    assert not np.any(got[1] == np.float32(1e30)) and not np.any(got[2] == -777)                  # nothing from behind a rank's cursor
    rows = np.concatenate([gathered[1][r, :c] for r, c in enumerate(cursors)])
    assert np.array_equal(got[1][:total], rows)                                                    # rank order = dataset order


def test_summed_in_rank_order_and_not_in_another(dev):
    """three loss sums whose fp64 sum depends on the association: (1e16 + 1) + 1 == 1e16, 1e16 + (1 + 1) != 1e16"""
    nl = 3
    words = np.zeros((3, SE.n_words(nl)), dtype=np.int64)
    words[:, 0] = np.array([1e16, 1.0, 1.0]).view(np.int64)
    words[:, 1] = words[:, -1] = 1
    results, truths = np.zeros((3, CAP, nl), dtype=np.float32), np.zeros((3, CAP), dtype=np.int64)
    got = _run(dev, (words, results, truths), _outputs(nl, 3 * CAP))
    assert got[0][:1].view(np.float64)[0] == (1e16 + 1.0) + 1.0 == 1e16 != 1e16 + (1.0 + 1.0)
    words[:, 0] = np.array([1.0, 1.0, 1e16]).view(np.int64)
    got = _run(dev, (words, results, truths), _outputs(nl, 3 * CAP))
    assert got[0][:1].view(np.float64)[0] == (1.0 + 1.0) + 1e16 == 1e16 + 2.0


def test_a_rank_that_overflowed_is_reported_and_its_kept_rows_merged(dev):
    """a rank cursor of cap + 3: its cap rows are merged, the three it dropped make cursor_out = out_cap + 3 and collected() raise, as for one rank"""
    from facialmmt_amd.eval_step import MeldMetrics
    nl = 7
    rng = np.random.default_rng(3)
    gathered = SE.fabricate(rng, [5, CAP + 3, 2], CAP, nl)
    want = _outputs(nl, 3 * CAP)
    SE.merge(*gathered, *want)
    m = MeldMetrics(nl, dev, collect_rows=3 * CAP)
    for t in (m.words, m.results, m.truths):
        t.fill_(SENTINEL)
    ops.eval_merge(*[torch.from_numpy(a).to(dev) for a in gathered], m.words, m.results, m.truths)
    got = [t.cpu().numpy() for t in (m.words, m.results, m.truths)]
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert int(got[0][-1]) == 3 * CAP + 3 > 3 * CAP
    assert np.array_equal(got[1][5:13], gathered[1][1]) and np.array_equal(got[1][13:15], gathered[1][2, :2]) and np.all(got[1][15:] == SENTINEL)
    assert m.result().count == int(gathered[0][:, 1].sum())                 # the dropped rows were counted on their rank and stay counted
    with pytest.raises(ValueError, match=rf"{3 * CAP + 3} rows.*collect_rows={3 * CAP}"):
        m.collected()


def test_outputs_smaller_than_the_total_keep_what_fits(dev):
    from facialmmt_amd.eval_step import MeldMetrics
    nl, out_cap = 3, 10
    rng = np.random.default_rng(4)
    gathered = SE.fabricate(rng, [8, 5, 1], CAP, nl)
    want = _outputs(nl, out_cap + 4)                                        # four guard rows behind out_cap, in one allocation
    SE.merge(gathered[0], gathered[1], gathered[2], want[0], want[1][:out_cap], want[2][:out_cap])
    ins = [torch.from_numpy(a).to(dev) for a in gathered]
    wo, ro, to = [torch.from_numpy(a).to(dev) for a in _outputs(nl, out_cap + 4)]
    ops.eval_merge(*ins, wo, ro[:out_cap], to[:out_cap])
    for g, w in zip((wo, ro, to), want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    assert int(wo[-1].item()) == out_cap + 4 > out_cap
    assert torch.equal(ro[8:10].cpu(), torch.from_numpy(gathered[1][1, :2])) and bool((ro[out_cap:] == SENTINEL).all()) and bool((to[out_cap:] == SENTINEL).all())
    with pytest.raises(ValueError, match=rf"{out_cap + 4} rows.*collect_rows={out_cap}"):
        MeldMetrics.collected_count(wo.cpu().numpy(), out_cap)


def test_more_rows_than_one_pass_of_the_grid_and_64_ranks(dev):
    """W = 64 ranks of cap = 700 rows, NL = 8: 358 400 elements against a grid of at most 1024 x 256 threads -- the grid-stride loop turns over, and the
    prefix has its full 64 entries"""
    nl, cap, W = 8, 700, 64
    rng = np.random.default_rng(5)
    cursors = [int(c) for c in rng.integers(0, cap + 1, size=W)]
    cursors[0], cursors[17], cursors[63] = cap, 0, 1
    gathered = SE.fabricate(rng, cursors, cap, nl)
    want = _outputs(nl, W * cap)
    SE.merge(*gathered, *want)
    got = _run(dev, gathered, _outputs(nl, W * cap))
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert int(got[0][-1]) == sum(cursors)


def test_front_end_checks_and_operator(dev):
    nl = 3
    rng = np.random.default_rng(6)
    gathered = SE.fabricate(rng, [4, 2], CAP, nl)
    ins = [torch.from_numpy(a).to(dev) for a in gathered]
    wo, ro, to = [torch.from_numpy(a).to(dev) for a in _outputs(nl, 2 * CAP)]
    for bad in ((ins[0][:, :-1].contiguous(), ins[1], ins[2], wo, ro, to), (ins[0], ins[1], ins[2][:, :-1].contiguous(), wo, ro, to),
                (ins[0], ins[1].double(), ins[2], wo, ro, to), (ins[0], ins[1], ins[2], wo[:-1], ro, to), (ins[0], ins[1], ins[2], wo, ro, to[:-1]),
                (ins[0], ins[1], ins[2], wo, ro[:, :2].contiguous(), to), (ins[0], ins[1], ins[2], wo.cpu(), ro, to)):
        with pytest.raises(_lib.FmmtError):
            ops.eval_merge(*bad)
    assert bool((wo == SENTINEL).all()) and bool((ro == SENTINEL).all())
    a = _run(dev, gathered, _outputs(nl, 2 * CAP))
    b = _run(dev, gathered, _outputs(nl, 2 * CAP), fn=torch.ops.fmmt.eval_merge)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and int(a[0][-1]) == 6
    torch.library.opcheck(torch.ops.fmmt.eval_merge.default, (*ins, wo, ro, to), test_utils=("test_schema", "test_faketensor"))
