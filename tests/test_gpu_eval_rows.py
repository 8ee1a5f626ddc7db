"""GPU tests of fmmt_eval_accumulate_rows (csrc/eval.hip, include/fmmt_eval_shard.h): the collecting metric update of a batch padded to B rows, the number
of rows that exist held in a device word.  The rows behind that number carry VALID labels and distinctive logits (1000 + ...): one that is counted or
stored shows.  Against numpy, against fmmt_eval_accumulate_at bit for bit when every row exists, across the end of the buffers, inside a captured graph
with the word rewritten between replays, and as a torch.library operator.

Bars: counts, cursor, labels, argmax and the stored logits exact.  The loss sum against fp64: a row's loss is lse - logit[label] in fp32, two numbers of
magnitude at most M = max|logit| + ln NL whose difference may be small, so the row's error is ABSOLUTE -- the rounding of logf, of m + log z and of the
subtraction, each at most an ulp of M: 4 * 2^-23 * max(1, M) per counted row covers them -- and the sum of the rows is a double, which adds nothing at
this scale.  (A bound relative to the loss sum would be a bound on luck for a batch of one row whose loss is small.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facialmmt_amd import _lib, ops

pytestmark = pytest.mark.gpu

GUARD = 16                     # rows behind the capacity that nothing may touch
SENTINEL = -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import facialmmt_amd.torch_ops  # noqa: F401
    return torch.device("cuda:0")


def _reference(logits, labels, nl):
    """(argmax, confusion, rows counted, fp64 loss sum) of the rows given"""
    lg = logits.float().cpu().numpy()
    lab = labels.cpu().numpy()
    arg = np.argmax(lg, axis=1) if len(lab) else np.zeros(0, dtype=np.int64)
    ok = lab >= 0
    conf = np.zeros((nl, nl), dtype=np.int64)
    np.add.at(conf, (lab[ok], arg[ok]), 1)
    lab64 = torch.from_numpy(np.where(ok, lab, -100))
    loss = F.cross_entropy(logits.double().cpu(), lab64, reduction="sum", ignore_index=-100).item() if ok.any() else 0.0
    return arg, conf, int(ok.sum()), loss


def _loss_bar(logits, count, nl):
    """the absolute bound on the loss sum of `count` rows (module docstring)"""
    m = float(logits.float().abs().max()) + float(np.log(nl)) if logits.numel() else 1.0
    return count * 4 * 2.0 ** -23 * max(1.0, m)


def _buffers(dev, nl, capacity):
    words = torch.zeros(2 + nl * nl + 1, dtype=torch.int64, device=dev)
    lo = torch.full((capacity + GUARD, nl), float(SENTINEL), device=dev)
    la = torch.full((capacity + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    pr = torch.full((capacity + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return words, lo, la, pr


def _batch(g, dev, B, nl, dtype, b):
    """B rows of which the first b exist: those as tests/test_gpu_eval_collect.py draws them (ties, ignored rows); the others with a VALID label and
    logits around 1000 -- a padded row that a kernel counts moves count and confusion, one that it stores is seen in the buffers"""
    logits = torch.randn(B, nl, generator=g, device=dev) * 3
    labels = torch.randint(0, nl, (B,), generator=g, device=dev)
    if b > 4:
        logits[3] = 0.5                                         # all equal: class 0
        labels[::7] = -100                                      # ignored rows, stored as they are
        labels[1] = -1
    logits[b:] = 1000 + torch.arange(B - b, device=dev, dtype=torch.float32)[:, None] + torch.arange(nl, device=dev, dtype=torch.float32)[None]
    labels[b:] = torch.arange(B - b, device=dev) % nl
    return logits.to(dtype), labels


def _summary(words, nl):
    host = words.cpu().numpy()
    return float(host[:1].view(np.float64)[0]), int(host[1]), host[2:2 + nl * nl].reshape(nl, nl), int(host[-1])


def _word(dev, value):
    return torch.tensor([value], dtype=torch.int32, device=dev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nl", [7, 3])
@pytest.mark.parametrize("B", [1, 4, 1024])
def test_only_the_rows_that_exist_are_stored_and_counted(dev, dtype, nl, B):
    """one launch per row count: B, B - 1, 1, 0 and the out-of-range words B + 5 and -3, which clamp to B and 0; the cursor starts at 3"""
    g = torch.Generator(device=dev).manual_seed(100 * B + nl)
    for word in dict.fromkeys((B, B - 1, 1, 0, B + 5, -3)):
        b = min(max(word, 0), B)
        cap = B + 8
        words, lo, la, pr = _buffers(dev, nl, cap)
        words[-1] = 3
        logits, labels = _batch(g, dev, B, nl, dtype, b)
        n_rows = _word(dev, word)
        assert ops.eval_accumulate_rows(logits, labels, words[:-1], words[-1:], n_rows, lo[:cap], la[:cap], pr[:cap]) is None
        assert int(n_rows.item()) == word                                  # the word is read, never written
        arg, conf, count, loss = _reference(logits[:b], labels[:b], nl)
        got_loss, got_count, got_conf, got_cursor = _summary(words, nl)
        assert got_cursor == 3 + b, (word, got_cursor)
        assert got_count == count and np.array_equal(got_conf, conf), (word, got_count, count)
        assert torch.equal(lo[3:3 + b], logits[:b].float()) and torch.equal(la[3:3 + b], labels[:b])
        assert torch.equal(pr[3:3 + b].cpu(), torch.from_numpy(arg.astype(np.int32)))
        for buf in (lo, la, pr):                                            # nothing in front of the cursor, nothing behind the b rows
            assert bool((buf[:3] == SENTINEL).all()) and bool((buf[3 + b:] == SENTINEL).all()), word
        if count:
            bar = _loss_bar(logits[:b], count, nl)
            print(f"eval_accumulate_rows B={B} NL={nl} {dtype} n_rows={word}: loss sum {got_loss!r} against fp64 {loss!r}: |err| {abs(got_loss - loss):.2e}, bar {bar:.2e}")
            assert abs(got_loss - loss) <= bar
        else:
            assert got_loss == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nl", [7, 3])
@pytest.mark.parametrize("B", [1, 4, 1024])
def test_with_every_row_present_the_bits_are_the_neighbours(dev, dtype, nl, B):
    """n_rows == B, three launches: accumulators (the loss sum's double included), stored rows and cursor bit-equal to fmmt_eval_accumulate_at"""
    g = torch.Generator(device=dev).manual_seed(7 * B + nl)
    cap = 3 * B
    w1, lo1, la1, pr1 = _buffers(dev, nl, cap)
    w2, lo2, la2, pr2 = _buffers(dev, nl, cap)
    n_rows = _word(dev, B)
    for _ in range(3):
        logits, labels = _batch(g, dev, B, nl, dtype, B)
        ops.eval_accumulate_rows(logits, labels, w1[:-1], w1[-1:], n_rows, lo1[:cap], la1[:cap], pr1[:cap])
        ops.eval_accumulate_at(logits, labels, w2[:-1], w2[-1:], lo2[:cap], la2[:cap], pr2[:cap])
    assert int(w1[-1].item()) == 3 * B
    assert torch.equal(w1, w2) and torch.equal(lo1, lo2) and torch.equal(la1, la2) and torch.equal(pr1, pr2)


def test_a_short_batch_across_the_end_is_cut_and_still_counted(dev):
    """capacity 10, the cursor at 8, a batch of B = 8 with 5 rows: two are stored, five counted, the cursor reads 13; the three padded rows are nowhere"""
    nl, B, cap = 7, 8, 10
    g = torch.Generator(device=dev).manual_seed(9)
    words, lo, la, pr = _buffers(dev, nl, cap)
    words[-1] = 8
    logits, labels = _batch(g, dev, B, nl, torch.float32, 5)
    ops.eval_accumulate_rows(logits, labels, words[:-1], words[-1:], _word(dev, 5), lo[:cap], la[:cap], pr[:cap])
    arg, conf, count, loss = _reference(logits[:5], labels[:5], nl)
    got_loss, got_count, got_conf, got_cursor = _summary(words, nl)
    assert got_cursor == 13 and got_count == count and np.array_equal(got_conf, conf) and abs(got_loss - loss) <= _loss_bar(logits[:5], count, nl)
    assert torch.equal(lo[8:10], logits[:2]) and torch.equal(la[8:10], labels[:2])
    for buf in (lo, la, pr):
        assert bool((buf[:8] == SENTINEL).all()) and bool((buf[10:] == SENTINEL).all())
    before = (lo.clone(), la.clone(), pr.clone())                           # the cursor behind the end: counted, kept nowhere
    ops.eval_accumulate_rows(logits, labels, words[:-1], words[-1:], _word(dev, 5), lo[:cap], la[:cap], pr[:cap])
    assert int(words[-1].item()) == 18 and int(words[1].item()) == 2 * count
    assert all(torch.equal(a, b) for a, b in zip((lo, la, pr), before))


def test_the_word_is_reread_by_every_replay_of_a_captured_graph(dev):
    """ONE captured MeldMetrics.update(n_rows=word), B = 4, replayed with the word rewritten to 4, 1, 3: the cursor reads 8 and the eight rows are dense"""
    from facialmmt_amd.eval_step import MeldMetrics
    from facialmmt_amd.graph_capture import _KEEP_GRAPHS, capture_window
    nl, B = 7, 4
    m = MeldMetrics(nl, dev, collect_rows=12)
    m.results.fill_(float(SENTINEL))
    m.truths.fill_(SENTINEL)
    s_logits, s_labels, word = torch.zeros(B, nl, device=dev), torch.zeros(B, dtype=torch.int64, device=dev), _word(dev, B)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        m.update(s_logits, s_labels, n_rows=word)                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize(dev)
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with capture_window():
        with torch.cuda.graph(graph, stream=stream):
            m.update(s_logits, s_labels, n_rows=word)
    assert int(m.cursor.item()) == 0                                        # capturing ran nothing
    m.results.fill_(float(SENTINEL))
    m.truths.fill_(SENTINEL)
    g = torch.Generator(device=dev).manual_seed(77)
    fed = []
    for b in (4, 1, 3):
        logits, labels = _batch(g, dev, B, nl, torch.float32, b)
        s_logits.copy_(logits)
        s_labels.copy_(labels)
        word.fill_(b)
        graph.replay()
        fed.append((logits[:b], labels[:b]))
    results, truths = m.collected()
    assert int(m.cursor.item()) == 8 and results.shape == (8, nl)
    assert torch.equal(results, torch.cat([x[0] for x in fed])) and torch.equal(truths, torch.cat([x[1] for x in fed]))
    assert bool((m.results[8:] == SENTINEL).all()) and bool((m.truths[8:] == SENTINEL).all())
    _, conf, count, loss = _reference(results, truths, nl)
    r = m.result()
    assert r.count == count and np.array_equal(r.confusion, conf) and abs(r.loss_sum - loss) <= _loss_bar(results, count, nl)
    _KEEP_GRAPHS.append((graph,))


def test_front_end_checks_the_word(dev):
    nl = 7
    words, lo, la, pr = _buffers(dev, nl, 8)
    logits, labels = torch.randn(4, nl, device=dev), torch.randint(0, nl, (4,), device=dev)
    for bad in (torch.tensor([4], device=dev), torch.tensor([4, 4], dtype=torch.int32, device=dev), torch.tensor([4], dtype=torch.int32), 4):
        with pytest.raises(_lib.FmmtError, match="n_rows"):
            ops.eval_accumulate_rows(logits, labels, words[:-1], words[-1:], bad, lo[:8], la[:8])
    with pytest.raises(_lib.FmmtError):
        ops.eval_accumulate_rows(logits, labels, words[:-1], words[-1:], _word(dev, 4), lo[:8], la[:7])
    assert int(words[-1].item()) == 0 and bool((lo == SENTINEL).all())


def test_operator_matches_front_end_and_passes_opcheck(dev):
    nl, B = 7, 33
    g = torch.Generator(device=dev).manual_seed(3)
    logits, labels = _batch(g, dev, B, nl, torch.float32, 20)
    w1, lo1, la1, pr1 = _buffers(dev, nl, 40)
    w2, lo2, la2, pr2 = _buffers(dev, nl, 40)
    w1[-1] = w2[-1] = 5
    word = _word(dev, 20)
    assert torch.ops.fmmt.eval_accumulate_rows(logits, labels, w1[:-1], w1[-1:], word, lo1[:40], la1[:40], pr1[:40]) is None
    ops.eval_accumulate_rows(logits, labels, w2[:-1], w2[-1:], word, lo2[:40], la2[:40], pr2[:40])
    assert torch.equal(w1, w2) and torch.equal(lo1, lo2) and torch.equal(la1, la2) and torch.equal(pr1, pr2)
    assert int(w1[-1].item()) == 25 and torch.equal(lo1[5:25], logits[:20]) and bool((lo1[25:] == SENTINEL).all())
    tests = ("test_schema", "test_faketensor")
    lo, la, pr = lo1[:40].clone(), la1[:40].clone(), pr1[:40].clone()
    acc, cur = torch.zeros(2 + nl * nl, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    torch.library.opcheck(torch.ops.fmmt.eval_accumulate_rows.default, (logits, labels, acc, cur, word, lo, la, pr), test_utils=tests)
    torch.library.opcheck(torch.ops.fmmt.eval_accumulate_rows.default, (logits.bfloat16(), labels, acc, cur, word, lo, la, None), test_utils=tests)
