"""GPU tests of fmmt_eval_accumulate_at (csrc/eval.hip, include/fmmt_eval_collect.h): the metric update that keeps the batch's rows at a row index
held in a device word and advances it.  Against numpy, against fmmt_eval_accumulate bit for bit, across the end of the buffers, inside a
captured graph, and as a torch.library operator.

Bars: counts, cursor, labels, argmax and the stored logits exact; the loss sum to 1e-5 relative against fp64, the bound of
tests/test_gpu_eval_step.py::test_eval_accumulate_matches_numpy (an NL-term fp32 log-sum-exp carries a few ulp per row, the sum is a double)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facialmmt_amd import _lib, ops

pytestmark = pytest.mark.gpu

GUARD = 16                     # rows behind the capacity that nothing may touch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import facialmmt_amd.torch_ops  # noqa: F401
    return torch.device("cuda:0")


def _reference(logits, labels, nl):
    lg = logits.float().cpu().numpy()
    lab = labels.cpu().numpy()
    arg = np.argmax(lg, axis=1)
    ok = lab >= 0
    conf = np.zeros((nl, nl), dtype=np.int64)
    np.add.at(conf, (lab[ok], arg[ok]), 1)
    lab64 = torch.from_numpy(np.where(ok, lab, -100))
    loss = F.cross_entropy(logits.double().cpu(), lab64, reduction="sum", ignore_index=-100).item() if ok.any() else 0.0
    return arg, conf, int(ok.sum()), loss


def _buffers(dev, nl, capacity):
    """accumulators + cursor in one allocation, and the three row buffers with GUARD rows of a sentinel behind the capacity"""
    words = torch.zeros(2 + nl * nl + 1, dtype=torch.int64, device=dev)
    lo = torch.full((capacity + GUARD, nl), -7.0, device=dev)
    la = torch.full((capacity + GUARD,), -7, dtype=torch.int64, device=dev)
    pr = torch.full((capacity + GUARD,), -7, dtype=torch.int32, device=dev)
    return words, lo, la, pr


def _batch(g, dev, B, nl, dtype):
    logits = (torch.randn(B, nl, generator=g, device=dev) * 3).to(dtype)
    labels = torch.randint(0, nl, (B,), generator=g, device=dev)
    if B > 1:
        if nl > 4:
            logits[::5, 4] = logits[::5, 2] = logits[::5].max(dim=1).values + 1     # ties: the first maximum (class 2) wins
        logits[3] = 0.5                                                              # all equal: class 0
        labels[::7] = -100                                                           # ignored rows, stored as they are
        labels[1] = -1
    return logits, labels


def _summary(words, nl):
    host = words.cpu().numpy()
    return float(host[:1].view(np.float64)[0]), int(host[1]), host[2:2 + nl * nl].reshape(nl, nl), int(host[-1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nl", [1, 7, 8])
@pytest.mark.parametrize("B", [1, 33, 1024])
def test_three_launches_match_numpy_and_the_plain_entry_point(dev, dtype, nl, B):
    """B = 1024 fills the workgroup: without the barrier between reading and advancing the cursor its late waves would store B rows too far"""
    g = torch.Generator(device=dev).manual_seed(100 * B + nl)
    cap = 3 * B
    words, lo, la, pr = _buffers(dev, nl, cap)
    acc, cursor = words[:-1], words[-1:]
    plain = torch.zeros(2 + nl * nl, dtype=torch.int64, device=dev)
    conf, count, loss = np.zeros((nl, nl), dtype=np.int64), 0, 0.0
    kept = []
    for k in range(3):
        logits, labels = _batch(g, dev, B, nl, dtype)
        assert ops.eval_accumulate_at(logits, labels, acc, cursor, lo[:cap], la[:cap], pr[:cap]) is None
        ops.eval_accumulate(logits, labels, plain, pred=False)
        arg, c, n, l = _reference(logits, labels, nl)
        conf, count, loss = conf + c, count + n, loss + l
        kept.append((logits.float(), labels, torch.from_numpy(arg.astype(np.int32)).to(dev)))
        assert int(cursor.item()) == (k + 1) * B
    got_loss, got_count, got_conf, got_cursor = _summary(words, nl)
    assert np.array_equal(got_conf, conf) and got_count == count and got_cursor == 3 * B
    assert torch.equal(lo[:cap], torch.cat([x[0] for x in kept]))
    assert torch.equal(la[:cap], torch.cat([x[1] for x in kept]))
    assert torch.equal(pr[:cap], torch.cat([x[2] for x in kept]))
    assert bool((lo[cap:] == -7).all()) and bool((la[cap:] == -7).all()) and bool((pr[cap:] == -7).all())
    if count:
        rel = abs(got_loss - loss) / max(abs(loss), 1e-300) if loss else abs(got_loss)
        print(f"eval_accumulate_at B={B} NL={nl} {dtype}: loss sum {got_loss!r} against fp64 {loss!r}: rel {rel:.2e}")
        assert rel <= 1e-5
    else:
        assert got_loss == 0.0
    assert torch.equal(acc, plain)                              # the two entry points: the same bits, the loss sum's double included


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_batch_across_the_end_is_cut_and_still_counted(dev, dtype):
    """out_capacity = 40, two batches of 33: the second stores 7 rows, the cursor reads 66, the accumulators count all 66 rows"""
    nl, B, cap = 7, 33, 40
    g = torch.Generator(device=dev).manual_seed(9)
    words, lo, la, pr = _buffers(dev, nl, cap)
    acc, cursor = words[:-1], words[-1:]
    conf, count, loss, kept = np.zeros((nl, nl), dtype=np.int64), 0, 0.0, []
    for _ in range(2):
        logits, labels = _batch(g, dev, B, nl, dtype)
        ops.eval_accumulate_at(logits, labels, acc, cursor, lo[:cap], la[:cap], pr[:cap])
        arg, c, n, l = _reference(logits, labels, nl)
        conf, count, loss = conf + c, count + n, loss + l
        kept.append((logits.float(), labels, torch.from_numpy(arg.astype(np.int32)).to(dev)))
    got_loss, got_count, got_conf, got_cursor = _summary(words, nl)
    assert got_cursor == 66
    assert torch.equal(lo[:cap], torch.cat([x[0] for x in kept])[:cap])
    assert torch.equal(la[:cap], torch.cat([x[1] for x in kept])[:cap])
    assert torch.equal(pr[:cap], torch.cat([x[2] for x in kept])[:cap])
    assert bool((lo[cap:] == -7).all()) and bool((la[cap:] == -7).all()) and bool((pr[cap:] == -7).all())       # the guard region
    assert np.array_equal(got_conf, conf) and got_count == count and count == 66 - int(sum((x[1] < 0).sum() for x in kept))
    assert abs(got_loss - loss) <= 1e-5 * abs(loss)
    # a third batch finds the cursor behind the end: nothing is stored, everything is counted
    logits, labels = _batch(g, dev, B, nl, dtype)
    before = (lo.clone(), la.clone(), pr.clone())
    ops.eval_accumulate_at(logits, labels, acc, cursor, lo[:cap], la[:cap], pr[:cap])
    assert int(cursor.item()) == 99 and int(acc[1].item()) == count + int((labels >= 0).sum())
    assert torch.equal(lo, before[0]) and torch.equal(la, before[1]) and torch.equal(pr, before[2])


def test_negative_labels_are_stored_as_they_are_and_not_counted(dev):
    nl = 7
    words, lo, la, pr = _buffers(dev, nl, 8)
    logits = torch.randn(5, nl, device=dev)
    labels = torch.tensor([-100, 3, -1, -5, 0], device=dev)
    ops.eval_accumulate_at(logits, labels, words[:-1], words[-1:], lo[:8], la[:8])          # no pred_out
    _, count, conf, cursor = _summary(words, nl)
    assert count == 2 and int(conf.sum()) == 2 and cursor == 5
    assert la[:5].tolist() == [-100, 3, -1, -5, 0] and bool((la[5:] == -7).all())
    assert torch.equal(lo[:5], logits) and bool((pr == -7).all())
    with pytest.raises(_lib.FmmtError):
        ops.eval_accumulate_at(logits, labels, words[:-1], words[-1:].int(), lo[:8], la[:8])
    with pytest.raises(_lib.FmmtError):
        ops.eval_accumulate_at(logits, labels, words[:-1], words[-1:], lo[:8], la[:7])
    with pytest.raises(_lib.FmmtError):
        ops.eval_accumulate_at(torch.zeros(1025, nl, device=dev), torch.zeros(1025, dtype=torch.int64, device=dev), words[:-1], words[-1:], lo[:8], la[:8])
    with pytest.raises(NotImplementedError):
        ops.eval_accumulate_at(logits.clone().requires_grad_(True), labels, words[:-1], words[-1:], lo[:8], la[:8])


def test_the_cursor_moves_inside_a_captured_graph(dev):
    """ONE captured MeldMetrics.update, replayed five times on changing inputs: the rows land at 0, B, 2B, ... -- the launch arguments are frozen,
    the cursor is not -- and a second run gives the same bits"""
    from facialmmt_amd.eval_step import MeldMetrics
    from facialmmt_amd.graph_capture import _KEEP_GRAPHS, capture_window
    nl, B, reps = 7, 33, 5
    m = MeldMetrics(nl, dev, collect_rows=reps * B)
    s_logits, s_labels = torch.zeros(B, nl, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        m.update(s_logits, s_labels)                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize(dev)
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with capture_window():
        with torch.cuda.graph(graph, stream=stream):
            m.update(s_logits, s_labels)
    assert int(m.cursor.item()) == 0                            # capturing ran nothing
    runs = []
    for run in range(2):
        m.reset()
        g = torch.Generator(device=dev).manual_seed(77)
        fed = []
        for _ in range(reps):
            logits, labels = _batch(g, dev, B, nl, torch.float32)
            s_logits.copy_(logits)
            s_labels.copy_(labels)
            graph.replay()
            fed.append((logits, labels))
        results, truths = m.collected()
        assert results.shape == (reps * B, nl) and int(m.cursor.item()) == reps * B
        assert torch.equal(results, torch.cat([x[0] for x in fed])) and torch.equal(truths, torch.cat([x[1] for x in fed]))
        assert m.result().count == sum(int((x[1] >= 0).sum()) for x in fed)
        runs.append((m.words.clone(), results.clone(), truths.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    graph.replay()                                              # a sixth batch: counted, not kept, and collected() says so
    with pytest.raises(ValueError, match=rf"{(reps + 1) * B} rows.*collect_rows={reps * B}"):
        m.collected()
    _KEEP_GRAPHS.append((graph,))


def test_operator_matches_front_end_and_passes_opcheck(dev):
    nl = 7
    logits, labels = torch.randn(33, nl, device=dev), torch.randint(0, nl, (33,), device=dev)
    w1, lo1, la1, pr1 = _buffers(dev, nl, 40)
    w2, lo2, la2, pr2 = _buffers(dev, nl, 40)
    w1[-1] = w2[-1] = 5
    assert torch.ops.fmmt.eval_accumulate_at(logits, labels, w1[:-1], w1[-1:], lo1[:40], la1[:40], pr1[:40]) is None
    ops.eval_accumulate_at(logits, labels, w2[:-1], w2[-1:], lo2[:40], la2[:40], pr2[:40])
    assert torch.equal(w1, w2) and torch.equal(lo1, lo2) and torch.equal(la1, la2) and torch.equal(pr1, pr2)
    assert int(w1[-1].item()) == 38 and torch.equal(lo1[5:38], logits) and torch.equal(la1[5:38], labels)
    tests = ("test_schema", "test_faketensor")
    lo, la, pr = lo1[:40].clone(), la1[:40].clone(), pr1[:40].clone()
    acc, cur = torch.zeros(2 + nl * nl, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    torch.library.opcheck(torch.ops.fmmt.eval_accumulate_at.default, (logits, labels, acc, cur, lo, la, pr), test_utils=tests)
    torch.library.opcheck(torch.ops.fmmt.eval_accumulate_at.default, (logits.bfloat16(), labels, acc, cur, lo, la, None), test_utils=tests)
