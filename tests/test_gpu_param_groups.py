"""GPU tests of the fused update over parameter groups (csrc/adamw_groups.hip, include/fmmt_groups.h; train_step.FusedClipAdamW over several groups).

The tensors are those of test_fused_clip_adamw_matches_torch -- (1024, 300) with a bf16 twin, (7,) the scalar tail, (4097,) across a block, (33, 5),
and a 12-byte-offset view of 5000 elements (the alignment fallback) -- spread over three groups in interleaved order [0, 1, 0, 2, 1]: different
learning rates, one group without weight decay, one with other betas and eps.  The kernels are held to BITS (torch.equal): the grouped launch to
one fmmt_adamw_batch launch per group over that group's sub-table, the guarded entry to the plain one; FusedClipAdamW is held to the eager
optimizers within the tolerance of test_fused_clip_adamw_matches_torch (the arithmetic per element is the same)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 300), (7,), (4097,), (33, 5), (5000,)]
GROUP_OF = [0, 1, 0, 2, 1]
TWIN, OFFSET = 0, 4
HYPER = [dict(betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05), dict(betas=(0.9, 0.98), eps=1e-6, weight_decay=0.0),
         dict(betas=(0.8, 0.95), eps=1e-8, weight_decay=0.01)]
LR0 = [1e-2, 3e-3, 5e-3]
MAX_NORM = 1.0
RTOL, ATOL = 2e-6, 2e-7                                          # test_fused_clip_adamw_matches_torch's
DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("low", "<u8"), ("n", "<i8"), ("bb", "<i4"), ("gb", "<i4")])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lr_at(j, k):
    return LR0[j] * (k + 1) / 4                                   # a moving learning rate, another one per group


class State:
    """parameters, moments, the twin, gradients, the step / norm words, one learning-rate word per group, and descriptor tables over any subset"""

    def __init__(self, dev, seed=0):
        g = torch.Generator(device="cpu").manual_seed(100 + seed)
        base = torch.zeros(5003, device=dev)
        self.p = [torch.randn(sh, generator=g).to(dev) for sh in SHAPES[:-1]] + [base[3:5003]]
        self.p[OFFSET].copy_(torch.randn(SHAPES[OFFSET], generator=g))
        assert self.p[OFFSET].data_ptr() % 16 == 12
        self.m = [(0.01 * torch.randn(sh, generator=g)).to(dev) for sh in SHAPES]
        self.v = [(1e-4 * torch.rand(sh, generator=g)).to(dev) for sh in SHAPES]
        self.low = [p.to(torch.bfloat16) if i == TWIN else None for i, p in enumerate(self.p)]
        self.g = [torch.zeros(sh, device=dev) for sh in SHAPES]
        self.step = torch.zeros((), device=dev)
        self.norm = torch.zeros((), device=dev)
        self.lrs = [torch.tensor(lr, device=dev) for lr in LR0]
        self.words = torch.zeros(6, dtype=torch.int64, device=dev)
        self.keep = []

    def table(self, records):
        arr = np.zeros(len(records), dtype=DESC)
        blocks = 0
        for k, i in enumerate(records):
            n = self.p[i].numel()
            arr[k] = (self.p[i].data_ptr(), self.g[i].data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(),
                      self.low[i].data_ptr() if self.low[i] is not None else 0, n, blocks, 0)
            blocks += (n + 4095) // 4096
        desc = torch.from_numpy(arr.view(np.uint8).copy()).to(self.step.device)
        self.keep.append(desc)
        return len(records), blocks, desc

    def group_tables(self, group_of, hyper, lrs):
        from facialmmt_amd import _lib
        tab = np.zeros(len(hyper), dtype=np.dtype(_lib.ADAMW_GROUP_FIELDS))
        for j, (h, lr) in enumerate(zip(hyper, lrs)):
            tab[j] = (lr.data_ptr(), h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], 0)
        dev = self.step.device
        out = torch.tensor(group_of, dtype=torch.int32, device=dev), torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        self.keep.append(out)
        return out

    def tensors(self):
        return self.p + self.m + self.v + [self.low[TWIN]]

    def snapshot(self):
        return [t.clone() for t in self.tensors()]

    def copy_from(self, other):
        for a, b in zip(self.tensors() + self.g + [self.step, self.norm] + self.lrs, other.tensors() + other.g + [other.step, other.norm] + other.lrs):
            a.copy_(b)

    def set_grads(self, k, scale):
        g = torch.Generator(device="cpu").manual_seed(2000 + k)
        for t in self.g:
            t.copy_(scale * torch.randn(t.shape, generator=g))
        self.norm.copy_(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(t) for t in self.g])))
        for j, lr in enumerate(self.lrs):
            lr.fill_(_lr_at(j, k))


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _per_group(s, hf):
    """the reference of the bit tests: one fmmt_adamw_batch launch per group over that group's sub-table, the same norm and step words"""
    from facialmmt_amd import ops
    for j, h in enumerate(HYPER):
        n, blocks, desc = s.table([i for i, k in enumerate(GROUP_OF) if k == j])
        ops.adamw_batch(n, blocks, desc, s.lrs[j], s.step, s.norm, h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], MAX_NORM, hf)


@pytest.mark.parametrize("hf", [False, True])
def test_grouped_launch_has_the_bits_of_one_launch_per_group(dev, hf):
    """four updates with moving learning rates, the clip binding in the first and third (gradient scale 10) and not in the others (1e-3)"""
    from facialmmt_amd import ops
    a, b = State(dev), State(dev)
    b.copy_from(a)
    n, blocks, desc = a.table(range(len(SHAPES)))
    group_of, groups = a.group_tables(GROUP_OF, HYPER, a.lrs)
    start = a.snapshot()
    for k in range(4):
        for s in (a, b):
            s.set_grads(k, 10.0 if k % 2 == 0 else 1e-3)
            s.step.add_(1.0)
        assert (float(a.norm) > MAX_NORM) == (k % 2 == 0)
        ops.adamw_groups(n, blocks, desc, len(HYPER), group_of, groups, a.step, a.norm, MAX_NORM, hf)
        _per_group(b, hf)
        torch.cuda.synchronize()
        assert _same(a.snapshot(), b.snapshot()), (hf, k)
    assert not any(torch.equal(x, y) for x, y in zip(a.snapshot(), start))
    assert torch.equal(a.low[TWIN], a.p[TWIN].to(torch.bfloat16))
    # a NULL norm word (no clip) is the plain entry's, too
    ops.adamw_groups(n, blocks, desc, len(HYPER), group_of, groups, a.step, None, MAX_NORM, hf)
    for j, h in enumerate(HYPER):
        nj, bj, dj = b.table([i for i, g in enumerate(GROUP_OF) if g == j])
        ops.adamw_batch(nj, bj, dj, b.lrs[j], b.step, None, h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], MAX_NORM, hf)
    torch.cuda.synchronize()
    assert _same(a.snapshot(), b.snapshot())


@pytest.mark.parametrize("hf", [False, True])
def test_one_group_has_the_bits_of_the_one_group_kernel(dev, hf):
    from facialmmt_amd import ops
    a, b = State(dev), State(dev)
    b.copy_from(a)
    h = HYPER[2]
    group_of, groups = a.group_tables([0] * len(SHAPES), [h], a.lrs[:1])
    for k in range(2):
        for s in (a, b):
            s.set_grads(k, 10.0 if k == 0 else 1e-3)
            s.step.add_(1.0)
        n, blocks, desc = a.table(range(len(SHAPES)))
        ops.adamw_groups(n, blocks, desc, 1, group_of, groups, a.step, a.norm, MAX_NORM, hf)
        n, blocks, desc = b.table(range(len(SHAPES)))
        ops.adamw_batch(n, blocks, desc, b.lrs[0], b.step, b.norm, h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], MAX_NORM, hf)
        torch.cuda.synchronize()
        assert _same(a.snapshot(), b.snapshot()), (hf, k)


def _guarded(s, tables, hf):
    from facialmmt_amd import ops
    n, blocks, desc, group_of, groups = tables
    ops.adamw_groups_guarded(n, blocks, desc, len(HYPER), group_of, groups, s.step, s.norm, MAX_NORM, hf)
    ops.guard_commit(s.norm, s.step, s.words)


def _one_group_guarded(s, table, hf):
    """the one-group pair on the same norm word: what the step word and the monitor words are held to"""
    from facialmmt_amd import ops
    n, blocks, desc = table
    h = HYPER[0]
    ops.adamw_batch_guarded(n, blocks, desc, s.lrs[0], s.step, s.norm, h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], MAX_NORM, hf)
    ops.guard_commit(s.norm, s.step, s.words)


@pytest.mark.parametrize("hf", [False, True])
def test_guarded_entry_applies_on_a_finite_norm_and_holds_on_nan_and_inf(dev, hf):
    from facialmmt_amd import ops
    a, b, c = State(dev), State(dev), State(dev)                  # guarded groups / plain groups / the one-group guarded pair
    b.copy_from(a)
    c.copy_from(a)
    ta = a.table(range(len(SHAPES))) + a.group_tables(GROUP_OF, HYPER, a.lrs)
    nb, bb, db = b.table(range(len(SHAPES)))
    gb = b.group_tables(GROUP_OF, HYPER, b.lrs)
    tc = c.table(range(len(SHAPES)))
    with pytest.raises(ValueError):
        ops.adamw_groups_guarded(*ta[:3], len(HYPER), *ta[3:], a.step, None, MAX_NORM, hf)
    applied = 0
    for k, bad in enumerate((None, float("nan"), None, float("inf"), float("-inf"))):
        for s in (a, b, c):
            s.set_grads(k, 10.0 if k % 2 == 0 else 1e-3)
            if bad is not None:
                s.norm.fill_(bad)
        before = a.snapshot()
        _guarded(a, ta, hf)
        _one_group_guarded(c, tc, hf)
        if bad is None:
            applied += 1
            b.step.add_(1.0)                                      # the plain entry called with step + 1
            ops.adamw_groups(nb, bb, db, len(HYPER), *gb, b.step, b.norm, MAX_NORM, hf)
        torch.cuda.synchronize()
        if bad is None:
            assert _same(a.snapshot(), b.snapshot()) and not _same(a.snapshot(), before), (hf, k)
        else:
            assert _same(a.snapshot(), before), (hf, k, bad)     # no byte of p, m, v or the twin
        assert float(a.step) == float(c.step) == applied
        assert torch.equal(a.words, c.words) and int(a.words[3]) == applied and int(a.words[4]) == k + 1 - applied
        assert int(a.words[5]) == int(a.norm.view(torch.int32).item()) & 0xFFFFFFFF


def test_guarded_update_and_commit_inside_a_captured_graph(dev):
    """ONE capture of the grouped guarded update + commit, replayed twice -- a finite norm, then a NaN: moved, then held, as the eager calls do"""
    from facialmmt_amd.graph_capture import _KEEP_GRAPHS, capture_window
    s, ref = State(dev), State(dev)
    s.set_grads(0, 10.0)
    ref.copy_from(s)
    ts = s.table(range(len(SHAPES))) + s.group_tables(GROUP_OF, HYPER, s.lrs)
    tr = ref.table(range(len(SHAPES))) + ref.group_tables(GROUP_OF, HYPER, ref.lrs)
    start = State(dev)
    start.copy_from(s)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _guarded(s, ts, True)                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with capture_window():
        with torch.cuda.graph(graph, stream=stream):
            _guarded(s, ts, True)
    s.copy_from(start)
    s.words.zero_()
    shots = []
    for norm in (None, float("nan")):
        for x in (s, ref):
            if norm is not None:
                x.norm.fill_(norm)
        graph.replay()
        _guarded(ref, tr, True)
        torch.cuda.synchronize()
        shots.append(s.snapshot())
        assert _same(shots[-1], ref.snapshot())
    assert not _same(shots[0], start.snapshot()) and _same(shots[0], shots[1])
    assert float(s.step) == 1.0 and torch.equal(s.words, ref.words) and (int(s.words[3]), int(s.words[4])) == (1, 1)
    _KEEP_GRAPHS.append((graph,))


# ------------------------------------------------------------------------------------------------ FusedClipAdamW over several groups
def _models(dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    base = torch.randn(20000, generator=g).to(dev)
    ref = [torch.nn.Parameter(torch.randn(sh, generator=g).to(dev)) for sh in SHAPES]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref[:-1]] + [torch.nn.Parameter(base[3:5003].detach())]   # a 12-byte-offset view
    with torch.no_grad():
        mine[-1].copy_(ref[-1])
    return g, ref, mine


def _optimizers(kind, ref, mine, dev, lr0=LR0, shared_lr=False):
    from facialmmt_amd.train_step import HFAdamW
    members = [[i for i, k in enumerate(GROUP_OF) if k == j] for j in range(3)]
    lrs = [torch.tensor(lr, device=dev) for lr in lr0]
    if shared_lr:
        lrs[2] = lrs[0]
    if kind == "hf":
        opt_ref = HFAdamW([dict(params=[ref[i] for i in members[j]], lr=lr0[j], **HYPER[j]) for j in range(3)])
        opt_mine = HFAdamW([dict(params=[mine[i] for i in members[j]], lr=lrs[j], **HYPER[j]) for j in range(3)])
    else:
        opt_ref = torch.optim.AdamW([dict(params=[ref[i] for i in members[j]], lr=lr0[j], **HYPER[j]) for j in range(3)])
        opt_mine = torch.optim.AdamW([dict(params=[mine[i] for i in members[j]], lr=lrs[j], **HYPER[j]) for j in range(3)], fused=True, capturable=True)
    return opt_ref, opt_mine, lrs


def _run(g, ref, mine, opt_ref, fused, grads, lrs, lr_at, steps=4):
    for k in range(steps):
        scale = 10.0 if k % 2 == 0 else 1e-3                     # clipped / not clipped
        for pr, pm in zip(ref, mine):
            gr = torch.randn(pr.shape, generator=g).to(pr.device) * scale
            pr.grad = gr.clone()
            grads[pm].copy_(gr)
        for j, grp in enumerate(opt_ref.param_groups):
            grp["lr"] = lr_at(j, k)
            lrs[j].fill_(lr_at(j, k))
        torch.nn.utils.clip_grad_norm_(ref, MAX_NORM)
        opt_ref.step()
        fused.update()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["torch", "hf"])
def test_fused_clip_adamw_over_three_groups_matches_the_eager_optimizer(dev, kind):
    from facialmmt_amd.train_step import FusedClipAdamW
    g, ref, mine = _models(dev, 3 if kind == "torch" else 5)
    opt_ref, opt_mine, lrs = _optimizers(kind, ref, mine, dev)
    low = mine[TWIN].detach().to(torch.bfloat16)
    grads = {p: torch.zeros_like(p) for p in mine}
    assert FusedClipAdamW.eligible(opt_mine, mine)
    fused = FusedClipAdamW(opt_mine, mine, grads, {id(mine[TWIN]): low}, max_norm=MAX_NORM)
    assert fused.hf == (kind == "hf") and fused.group_table is not None and fused.group_of.tolist() == GROUP_OF
    _run(g, ref, mine, opt_ref, fused, grads, lrs, _lr_at)
    for i, (pr, pm) in enumerate(zip(ref, mine)):
        print(kind, i, "max |eager - fused|", float((pr.detach() - pm.detach()).abs().max()))
        assert torch.allclose(pr, pm, rtol=RTOL, atol=ATOL), (i, (pr - pm).abs().max())
    assert torch.equal(low, mine[TWIN].detach().to(torch.bfloat16))
    assert float(fused.step) == 4 and not opt_mine.state


@pytest.mark.parametrize("kind", ["torch", "hf"])
def test_a_group_with_lr_zero_keeps_its_parameters_and_advances_its_moments(dev, kind):
    from facialmmt_amd.train_step import FusedClipAdamW
    g, ref, mine = _models(dev, 7)
    opt_ref, opt_mine, lrs = _optimizers(kind, ref, mine, dev, lr0=[1e-2, 0.0, 5e-3])
    grads = {p: torch.zeros_like(p) for p in mine}
    fused = FusedClipAdamW(opt_mine, mine, grads, {}, max_norm=MAX_NORM)
    start = [p.detach().clone() for p in mine]
    _run(g, ref, mine, opt_ref, fused, grads, lrs, lambda j, k: 0.0 if j == 1 else _lr_at(j, k), steps=2)
    for i, (pr, pm, p0, m, v) in enumerate(zip(ref, mine, start, fused.m, fused.v)):
        if GROUP_OF[i] == 1:
            assert torch.equal(pm, p0) and torch.equal(pr, p0), i
            assert float(m.abs().max()) > 0 and float(v.abs().max()) > 0
        else:
            assert not torch.equal(pm, p0)
        assert torch.allclose(pr, pm, rtol=RTOL, atol=ATOL)
        assert torch.allclose(opt_ref.state[pr]["exp_avg"], m, rtol=RTOL, atol=ATOL), i
        assert torch.allclose(opt_ref.state[pr]["exp_avg_sq"], v, rtol=RTOL, atol=ATOL), i


def test_eligibility_over_groups(dev):
    from facialmmt_amd.train_step import FusedClipAdamW
    for kind in ("torch", "hf"):
        _, ref, mine = _models(dev, 9)
        opt_ref, opt_mine, lrs = _optimizers(kind, ref, mine, dev, shared_lr=True)      # two groups share one learning-rate tensor
        assert FusedClipAdamW.eligible(opt_mine, mine)
        assert FusedClipAdamW.eligible(opt_mine, mine[:2])                              # a subset of the optimizer's parameters
        assert not FusedClipAdamW.eligible(opt_ref, ref)                                # every group's lr a Python float
        assert not FusedClipAdamW.eligible(opt_mine, mine + [torch.nn.Parameter(torch.zeros(3, device=dev))])     # a parameter no group holds
        opt_mine.param_groups[1]["lr"] = 3e-3                                           # ONE group's lr a Python float
        assert not FusedClipAdamW.eligible(opt_mine, mine)
        opt_mine.param_groups[1]["lr"] = lrs[1]
        opt_mine.param_groups[2]["lr"] = lrs[2].cpu()                                   # ... or a host tensor
        assert not FusedClipAdamW.eligible(opt_mine, mine)
        opt_mine.param_groups[2]["lr"] = lrs[2].double()                                # ... or a device word the kernel cannot read as fp32
        assert not FusedClipAdamW.eligible(opt_mine, mine)


def test_digest_and_export_load_round_trip_over_groups(dev):
    from facialmmt_amd.train_step import FusedClipAdamW
    objs = []
    for _ in range(2):
        g, ref, mine = _models(dev, 11)
        opt_ref, opt_mine, lrs = _optimizers("hf", ref, mine, dev)
        grads = {p: torch.zeros_like(p) for p in mine}
        fused = FusedClipAdamW(opt_mine, mine, grads, {}, max_norm=MAX_NORM)
        _run(g, ref, mine, opt_ref, fused, grads, lrs, _lr_at, steps=2)
        objs.append((fused, mine, grads, opt_mine))
    (fa, pa, ga, oa), (fb, pb, gb, ob) = objs
    da, db = fa.digest(), fb.digest()
    assert da.shape == (6,) and torch.equal(da, db)
    m, v, n = fa.export()
    assert n == 2 and all(t.device.type == "cpu" for t in m + v)
    fb.reset()
    assert not torch.equal(fb.digest(), da)
    saved = types.SimpleNamespace(param_groups=[dict(h) for h in HYPER],
                                  state={p: {"exp_avg": mi, "exp_avg_sq": vi, "step": n} for p, mi, vi in zip(pb, m, v)})
    fb.load_from(saved)
    assert float(fb.step) == 2.0 and torch.equal(fb.digest(), da)
    other = [dict(h) for h in HYPER]
    other[1]["eps"] = 1e-3
    with pytest.raises(ValueError, match="group 1.*`eps`"):
        fb.load_from(types.SimpleNamespace(param_groups=other, state=saved.state))
    for (fused, mine, grads, _) in objs:                                               # and both continue alike
        gen = torch.Generator(device="cpu").manual_seed(99)
        for p in mine:
            grads[p].copy_(torch.randn(p.shape, generator=gen))
        fused.update()
    assert torch.equal(fa.digest(), fb.digest()) and all(torch.equal(x, y) for x, y in zip(pa, pb))
