"""fmmt_eval_merge (include/fmmt_eval_shard.h) restated in numpy, and fabricated gathers to feed it: what tests/test_eval_shard_cpu.py checks against a
direct single-pass computation and tests/test_gpu_eval_merge.py holds the kernel to."""
import numpy as np


def n_words(nl):
    return 2 + nl * nl + 1


def merge(words, results, truths, words_out, results_out, truths_out):
    """words (W, 2 + NL^2 + 1) int64, results (W, cap, NL) float32, truths (W, cap) int64 -> the three outputs, written IN PLACE where the kernel
    writes them and left alone elsewhere: rank r's first n_r = clamp(cursor_r, 0, cap) rows at [start_r, start_r + n_r) as far as out_cap goes, the
    loss sums added left to right in rank order, integer sums of count and confusion, ranks with a cursor <= 0 left out; the cursor as the header
    states it"""
    W, cap, nl = results.shape
    out_cap = results_out.shape[0]
    cursors = [int(c) for c in words[:, -1]]
    start = 0
    loss, first = 0.0, True
    ints = np.zeros(n_words(nl) - 2, dtype=np.int64)
    for r in range(W):
        n = min(max(cursors[r], 0), cap)
        fits = max(min(n, out_cap - start), 0)
        results_out[start:start + fits] = results[r, :fits]
        truths_out[start:start + fits] = truths[r, :fits]
        start += n
        if cursors[r] > 0:
            l = float(words[r, :1].view(np.float64)[0])
            loss = l if first else loss + l
            first = False
            ints += words[r, 1:-1]
    seen = sum(max(c, 0) for c in cursors)
    kept = min(start, out_cap)
    words_out[:1] = np.array([loss], dtype=np.float64).view(np.int64)
    words_out[1:-1] = ints
    words_out[-1] = kept if seen == kept else out_cap + (seen - kept)


def fabricate(rng, cursors, cap, nl, poison=1e30):
    """a gather as W ranks with the given cursors leave it: rows in front of min(cursor, cap) random with labels in [-1, nl) (a negative one: a row the
    loader marked ignored), rows behind it POISON (a kernel that reads or moves one shows); accumulators computed from the rows that went through the
    updates -- for a cursor above cap the rows that were dropped are counted too, as the metric update does"""
    W = len(cursors)
    words = np.zeros((W, n_words(nl)), dtype=np.int64)
    results = np.full((W, cap, nl), poison, dtype=np.float32)
    truths = np.full((W, cap), -777, dtype=np.int64)
    for r, c in enumerate(cursors):
        seen = max(c, 0)
        rows = rng.standard_normal((seen, nl)).astype(np.float32)
        labels = rng.integers(-1, nl, size=seen).astype(np.int64)
        n = min(seen, cap)
        results[r, :n], truths[r, :n] = rows[:n], labels[:n]
        ok = labels >= 0
        m = rows.max(axis=1)
        lse = m + np.log(np.exp(rows - m[:, None]).sum(axis=1))
        losses = (lse - rows[np.arange(seen), np.where(ok, labels, 0)]).astype(np.float64)
        words[r, :1] = np.array([losses[ok].sum()], dtype=np.float64).view(np.int64)
        words[r, 1] = int(ok.sum())
        conf = np.zeros((nl, nl), dtype=np.int64)
        np.add.at(conf, (labels[ok], rows.argmax(axis=1)[ok]), 1)
        words[r, 2:-1] = conf.ravel()
        words[r, -1] = c
    return words, results, truths
