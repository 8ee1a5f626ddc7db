"""GPU tests of the kernels of csrc/guard.hip (include/fmmt_guard.h): the optimizer update that touches nothing when the gradient norm is not finite,
its commit and the loss monitor.

One descriptor table over five records walks every path of the shared body (csrc/adamw_core.h):
  n = 5                 the scalar tail alone;
  n = 4096 + 3          two blocks: the vector path, then a tail;
  n = 8192              with a bf16 twin;
  n = 4096              with a bf16 gradient (g_is_bf16);
  n = 1027              p, g, m, v as views starting ONE element into larger buffers: the 16-byte check fails and the scalar fallback runs.
Every comparison is torch.equal: the guarded kernel on a finite norm is held to the bits of ops.adamw_batch with the step word one higher, on a
non-finite norm to the bits from before.  The loss monitor is held to the same sum formed in Python -- one fp32 product widened to a double, then a
double sum, in order -- exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (5, 4096 + 3, 8192, 4096, 1027)
TWIN, BF16_GRAD, OFFSET = 2, 3, 4                              # the records with a bf16 twin / a bf16 gradient / misaligned views
HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01, max_norm=1.0)
BLOCKS = sum((n + 4095) // 4096 for n in SIZES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _view(t, rec):
    """the record's tensor: for the OFFSET record a view that starts one element into a buffer one element longer"""
    if rec != OFFSET:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t)
    return buf[1:]


class State:
    """parameters, moments, twins, gradients, the step / norm / learning-rate words and the descriptor table over them"""

    def __init__(self, dev, seed=0):
        g = torch.Generator(device=dev).manual_seed(1000 + seed)
        self.p = [_view(torch.randn(n, device=dev, generator=g), i) for i, n in enumerate(SIZES)]
        self.m = [_view(0.01 * torch.randn(n, device=dev, generator=g), i) for i, n in enumerate(SIZES)]
        self.v = [_view(1e-4 * torch.rand(n, device=dev, generator=g), i) for i, n in enumerate(SIZES)]
        self.low = [p.to(torch.bfloat16) if i == TWIN else None for i, p in enumerate(self.p)]
        self.g = [_view(torch.zeros(n, dtype=torch.bfloat16 if i == BF16_GRAD else torch.float32, device=dev), i) for i, n in enumerate(SIZES)]
        assert self.p[OFFSET].data_ptr() % 16 == 4 and self.p[0].data_ptr() % 16 == 0
        self.step = torch.zeros((), device=dev)
        self.norm = torch.zeros((), device=dev)
        self.lr = torch.tensor(1e-2, device=dev)
        self.words = torch.zeros(6, dtype=torch.int64, device=dev)
        arr = np.zeros(len(SIZES), dtype=np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("low", "<u8"), ("n", "<i8"), ("bb", "<i4"), ("gb", "<i4")]))
        blocks = 0
        for i, n in enumerate(SIZES):
            arr[i] = (self.p[i].data_ptr(), self.g[i].data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(),
                      self.low[i].data_ptr() if self.low[i] is not None else 0, n, blocks, int(i == BF16_GRAD))
            blocks += (n + 4095) // 4096
        assert blocks == BLOCKS and arr.itemsize == 56
        self.desc = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)

    def tensors(self):
        return self.p + self.m + self.v + [self.low[TWIN], self.step]

    def snapshot(self):
        return [t.clone() for t in self.tensors()]

    def copy_from(self, other):
        for a, b in zip(self.tensors() + self.g, other.tensors() + other.g):
            a.copy_(b)

    def set_grads(self, seed, scale=1.0):
        g = torch.Generator(device=self.step.device).manual_seed(2000 + seed)
        for t in self.g:
            t.copy_(scale * torch.randn(t.numel(), device=t.device, generator=g))

    def guarded(self, hf):
        from facialmmt_amd import ops
        ops.adamw_batch_guarded(len(SIZES), BLOCKS, self.desc, self.lr, self.step, self.norm, hf=hf, **HYPER)
        ops.guard_commit(self.norm, self.step, self.words)

    def plain(self, hf):
        from facialmmt_amd import ops
        self.step.add_(1.0)
        ops.adamw_batch(len(SIZES), BLOCKS, self.desc, self.lr, self.step, self.norm, hf=hf, **HYPER)

    def read(self):
        from facialmmt_amd.train_step import TrainMonitor
        return TrainMonitor.summarise(self.words.cpu().numpy())

    def norm_bits(self):
        return int(self.norm.view(torch.int32).item()) & 0xFFFFFFFF


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("hf", [False, True])
def test_finite_norm_gives_the_bits_of_the_plain_update(dev, hf):
    """two successive updates, the clip binding in the first (norm 2.5 against max_norm 1) and not in the second (0.5)"""
    a, b = State(dev), State(dev)
    b.copy_from(a)
    start = a.snapshot()
    for k, norm in enumerate((2.5, 0.5)):
        for s in (a, b):
            s.set_grads(k)
            s.norm.fill_(norm)
        a.guarded(hf)
        b.plain(hf)
        torch.cuda.synchronize()
        assert _same(a.snapshot(), b.snapshot()), (hf, k)
        assert float(a.step) == float(b.step) == k + 1
        r = a.read()
        assert (r.applied, r.skipped, r.last_norm) == (k + 1, 0, norm)
    moved = [not torch.equal(x, y) for x, y in zip(a.snapshot(), start)]
    assert all(moved), moved                                    # every record's p, m, v, the twin and the step word
    for s in (a, b):                                            # the twin is the parameter re-rounded; the bytes in front of the offset views are untouched
        assert torch.equal(s.low[TWIN], s.p[TWIN].to(torch.bfloat16))


@pytest.mark.parametrize("hf", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_norm_written_into_the_word_leaves_every_bit(dev, hf, bad):
    s = State(dev)
    s.set_grads(0)
    s.norm.fill_(1.5)
    s.guarded(hf)                                               # one applied update first: a step word and moments that are not the initial ones
    before = s.snapshot()
    for k in range(2):
        s.set_grads(1 + k)
        s.norm.fill_(bad)
        s.guarded(hf)
        torch.cuda.synchronize()
        assert _same(s.snapshot(), before), (hf, bad, k)
        r = s.read()
        assert (r.applied, r.skipped) == (1, k + 1) and float(s.step) == 1.0
        assert int(s.words[5]) == s.norm_bits() and not np.isfinite(r.last_norm)
    s.set_grads(3)
    s.norm.fill_(0.7)                                           # and the next finite norm applies, as update number two
    ref = State(dev)
    ref.copy_from(s)
    ref.norm.fill_(0.7)
    s.guarded(hf)
    ref.plain(hf)
    torch.cuda.synchronize()
    assert _same(s.snapshot(), ref.snapshot()) and float(s.step) == 2.0 and s.read().applied == 2


def _handover_norm(s):
    """fmmt_grad_handover over the state's gradients into fp32 slots of their own: the norm of what the update will read lands in s.norm"""
    from facialmmt_amd import _lib
    dev = s.step.device
    dst = [torch.empty(n, device=dev) for n in SIZES]
    arr = np.zeros(len(SIZES), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("n", "<i8"), ("bb", "<i4"), ("flags", "<i4")]))
    blocks = 0
    for i, n in enumerate(SIZES):
        arr[i] = (s.g[i].data_ptr(), dst[i].data_ptr(), n, blocks, int(i == BF16_GRAD))
        blocks += (n + 4095) // 4096
    table = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
    partial = torch.empty(blocks, device=dev)
    _lib.check(_lib.load().fmmt_grad_handover(len(SIZES), blocks, table.data_ptr(), partial.data_ptr(), s.norm.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "fmmt_grad_handover")
    torch.cuda.synchronize()
    return dst


def test_the_norm_of_the_hand_over_skips_on_nan_inf_and_overflow(dev):
    """the norm as the steps produce it: one NaN in the last element of the last record, one inf in the first element of the first, and two FINITE
    values of 3e19 whose squares overflow fp32 -- all three skip"""
    s = State(dev)
    before = s.snapshot()

    def poison(case):
        s.set_grads(10 + case, scale=1e-2)
        if case == 0:
            s.g[-1][-1] = float("nan")
        elif case == 1:
            s.g[0][0] = float("inf")
        else:
            s.g[1][7] = 3e19
            s.g[1][4098] = 3e19
            assert all(bool(torch.isfinite(t.float()).all()) for t in s.g)
    for case in range(3):
        poison(case)
        _handover_norm(s)
        assert not bool(torch.isfinite(s.norm)), (case, float(s.norm))
        s.guarded(True)
        torch.cuda.synchronize()
        assert _same(s.snapshot(), before), case
        r = s.read()
        assert (r.applied, r.skipped) == (0, case + 1) and not np.isfinite(r.last_norm)
    s.set_grads(20, scale=1e-2)                                 # clean gradients: the same path applies
    _handover_norm(s)
    assert bool(torch.isfinite(s.norm)) and float(s.norm) > 0
    s.guarded(True)
    torch.cuda.synchronize()
    assert not any(torch.equal(x, y) for x, y in zip(s.snapshot(), before)) and s.read().applied == 1


def test_monitor_loss_is_the_python_sum_exactly(dev):
    from facialmmt_amd import ops
    from facialmmt_amd.train_step import TrainMonitor
    # 3e38 is finite and its product with the scale is not: the product is what is tested
    seq = [0.5, float("nan"), 1.25, float("inf"), 0.1, 3e38, float("-inf"), 1e-3, 7.0 / 3.0, -0.3]
    scale = 3.0
    losses = torch.tensor(seq, dtype=torch.float32, device=dev)
    mon = TrainMonitor(dev)
    for i in range(len(seq)):
        ops.monitor_loss(losses[i:i + 1], scale, mon.words)
    want, micro, bad = 0.0, 0, 0
    for x in np.asarray(seq, dtype=np.float32):
        with np.errstate(over="ignore", invalid="ignore"):
            prod = np.float32(x) * np.float32(scale)            # one fp32 product
        if np.isfinite(prod):
            want += float(prod)                                 # widened to a double, added in order
            micro += 1
        else:
            bad += 1
    r = mon.read()
    print("loss_sum", r.loss_sum, "python", want, "micro", r.micro_steps, "non-finite", r.nonfinite_losses)
    assert (micro, bad) == (6, 4)
    assert np.float64(r.loss_sum).view(np.int64) == np.float64(want).view(np.int64)
    assert (r.micro_steps, r.nonfinite_losses, r.applied, r.skipped) == (micro, bad, 0, 0)
    assert r.avg_loss == want / micro
    mon.reset()
    assert int(mon.words.abs().sum()) == 0
    for bad_words in (mon.words[:5], torch.zeros(6, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError):
            ops.monitor_loss(losses[:1], scale, bad_words)
    with pytest.raises(ValueError):
        ops.monitor_loss(losses[:2], scale, mon.words)


def test_update_commit_and_monitor_inside_a_captured_graph(dev):
    """ONE capture of guarded update + commit + monitor, replayed with the norm word rewritten between replays -- finite, NaN, finite: the parameters
    move, hold, move; two identical runs give identical bits"""
    from facialmmt_amd import ops
    from facialmmt_amd.graph_capture import _KEEP_GRAPHS, capture_window
    s = State(dev)
    s.set_grads(30)
    loss = torch.tensor(0.25, device=dev)
    start = State(dev)
    start.copy_from(s)
    stream = torch.cuda.Stream(dev)

    def body():
        s.guarded(True)
        ops.monitor_loss(loss, 2.0, s.words)
    s.norm.fill_(1.0)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        body()                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with capture_window():
        with torch.cuda.graph(graph, stream=stream):
            body()
    runs = []
    for _ in range(2):
        s.copy_from(start)
        s.words.zero_()
        shots = [s.snapshot()]
        for norm, lv in ((1.0, 0.25), (float("nan"), float("nan")), (4.0, 0.5)):
            s.norm.fill_(norm)
            loss.fill_(lv)
            graph.replay()
            torch.cuda.synchronize()
            shots.append(s.snapshot())
        assert not any(torch.equal(x, y) for x, y in zip(shots[0], shots[1]))       # moved
        assert _same(shots[1], shots[2])                                            # held
        assert not any(torch.equal(x, y) for x, y in zip(shots[2], shots[3]))       # moved
        r = s.read()
        assert (r.applied, r.skipped, r.micro_steps, r.nonfinite_losses, r.loss_sum, r.last_norm) == (2, 1, 2, 1, 1.5, 4.0)
        assert float(s.step) == 2.0
        runs.append(shots[3] + [s.words.clone()])
    assert _same(*runs)
    _KEEP_GRAPHS.append((graph,))
