"""GPU tests of the three ops that let a fixed-capacity frame buffer stand in for a ragged MELD batch (csrc/ragged.hip, csrc/frame_filter.hip;
include/fmmt_ragged.h): device-side packing, the row-masked BatchNorm1d of Swin's embedding head, the frame filter's n_valid.

References: torch.nn.functional.batch_norm in fp64 on the CPU over the real rows; torch.cat of the real frames; oracle.train_glue.select_frames_loop
on the real rows of preds.  Tolerances of the masked BatchNorm are those tests/support_op_cases.py::t_misc holds the unmasked kernel to (relative to
the reference's largest magnitude): fp32 1e-5 forward / 4e-5 backward, bf16 1.5e-2 / 6e-2, running mean 1e-5, running variance 1e-5 (fp32) / 2e-2 (bf16)."""
import pytest
import torch

from facialmmt_amd import synth

pytestmark = pytest.mark.gpu

N_CAP = 40


def _close(name, got, ref, tol):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    print(f"{name:40s} max|err|={err:.3e} ref_scale={scale:.3e} tol={tol:g}")
    assert torch.isfinite(got).all(), name
    assert err <= tol * max(scale, 1e-6), (name, err, scale, tol)


def _bn_inputs(C, dt, dev):
    x = synth.tensor("x", (N_CAP, C), seed=1).to(dt)
    dy = synth.tensor("dy", (N_CAP, C), seed=6).to(dt)
    g = synth.tensor("g", (C,), seed=2) * 0.2 + 1
    b = synth.tensor("b", (C,), seed=3) * 0.1
    rm, rv = synth.tensor("rm", (C,), seed=4) * 0.1, synth.tensor("rv", (C,), seed=5).abs() + 0.5
    return x, dy, g, b, rm, rv


def _bn_reference(x, dy, g, b, rm, rv, n):
    """fp64, CPU, over the n real rows; one row: the reference's duplicate-the-sample rule (Swin_Transformer.forward, ref :535-538)"""
    xr = x[:n].double().requires_grad_(True)
    gr, br = g.double().requires_grad_(True), b.double().requires_grad_(True)
    rm2, rv2 = rm.double().clone(), rv.double().clone()
    xin = torch.cat((xr, xr), dim=0) if n == 1 else xr
    yr = torch.nn.functional.batch_norm(xin, rm2, rv2, gr, br, True, 0.1, 1e-5)[:n]
    yr.backward(dy[:n].double())
    return yr.detach(), rm2, rv2, xr.grad, gr.grad, br.grad


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [512, 70])
@pytest.mark.parametrize("n", [1, 2, 17, 40])
def test_masked_batchnorm_matches_fp64_over_the_real_rows(n, C, dt):
    """n = 2 leaves 14 of the 16 row groups empty, 17 is one past a group boundary, C = 70 exercises the column guard.  The padded rows of x and dy hold
    1e3: a leak into the statistics, the column sums or dx could not hide.  Rows >= n of y and dx are exactly zero."""
    from facialmmt_amd import ops
    dev = torch.device("cuda:0")
    tol = 1e-5 if dt == torch.float32 else 1.5e-2
    x, dy, g, b, rm, rv = _bn_inputs(C, dt, dev)
    ref = _bn_reference(x, dy, g, b, rm, rv, n)
    xd, dyd = x.clone(), dy.clone()
    xd[n:] = 1e3
    dyd[n:] = 1e3
    xd = xd.to(dev).requires_grad_(True)
    gd, bd = g.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    rmd, rvd = rm.to(dev), rv.to(dev)
    nv = torch.tensor([n, 12345], dtype=torch.int32, device=dev)           # pack_frames' counts: the first word counts
    y = ops.batch_norm_1d(xd, gd, bd, rmd, rvd, 0.1, 1e-5, True, n_valid=nv)
    y.backward(dyd.to(dev))
    torch.cuda.synchronize()
    tag = f"n={n} C={C} {dt}"
    _close(f"bn_n fwd {tag}", y[:n], ref[0], tol)
    _close(f"bn_n running_mean {tag}", rmd, ref[1], 1e-5)
    _close(f"bn_n running_var {tag}", rvd, ref[2], 1e-5 if dt == torch.float32 else 2e-2)
    _close(f"bn_n bwd dx {tag}", xd.grad[:n], ref[3], tol * 4)
    _close(f"bn_n bwd dgamma {tag}", gd.grad, ref[4], tol * 4)
    _close(f"bn_n bwd dbeta {tag}", bd.grad, ref[5], tol * 4)
    assert y.shape == (N_CAP, C) and xd.grad.shape == (N_CAP, C)
    assert float(y[n:].float().abs().max()) == 0.0 if n < N_CAP else True
    assert float(xd.grad[n:].float().abs().max()) == 0.0 if n < N_CAP else True
    if n == 1:                                                  # the duplicate rule: variance 0 -> y = beta, running variance decays by (1 - momentum), dx = 0
        assert float(xd.grad[:1].float().abs().max()) == 0.0
        _close(f"bn_n running_var n=1 {tag}", rvd, 0.9 * rv.double(), 1e-6)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [512, 70])
def test_masked_batchnorm_over_every_row_gives_the_unmasked_bits(C, dt):
    from facialmmt_amd import ops
    dev = torch.device("cuda:0")
    x, dy, g, b, rm, rv = _bn_inputs(C, dt, dev)
    out = []
    for nv in (None, torch.tensor([N_CAP], dtype=torch.int32, device=dev)):
        xd = x.to(dev).requires_grad_(True)
        gd, bd = g.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        rmd, rvd = rm.to(dev), rv.to(dev)
        y = ops.batch_norm_1d(xd, gd, bd, rmd, rvd, 0.1, 1e-5, True, n_valid=nv) if nv is not None else ops.batch_norm_1d(xd, gd, bd, rmd, rvd, 0.1, 1e-5, True)
        y.backward(dy.to(dev))
        out.append((y.detach(), rmd, rvd, xd.grad, gd.grad, bd.grad))
    torch.cuda.synchronize()
    for name, a, m in zip(("y", "running_mean", "running_var", "dx", "dgamma", "dbeta"), *out):
        assert torch.equal(a, m), name


def test_masked_batchnorm_without_real_rows_writes_zeros_and_keeps_the_statistics():
    from facialmmt_amd import ops
    dev = torch.device("cuda:0")
    x, dy, g, b, rm, rv = _bn_inputs(70, torch.float32, dev)
    xd = (x + 1e3).to(dev).requires_grad_(True)
    gd, bd = g.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    rmd, rvd = rm.to(dev), rv.to(dev)
    y = ops.batch_norm_1d(xd, gd, bd, rmd, rvd, 0.1, 1e-5, True, n_valid=torch.zeros(1, dtype=torch.int32, device=dev))
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)
    for t in (y, xd.grad, gd.grad, bd.grad):
        assert float(t.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ packing
_ROWS = {"u8": (torch.uint8, (112, 112, 3), 37632), "bf16": (torch.bfloat16, (3, 224, 224), 301056), "fp32": (torch.float32, (3, 224, 224), 602112)}
_FRAMES = {}


def _loader_frames(kind, dev):
    """(3, 5, ...) frames, every slot filled (padding included: packing, not luck, has to remove it); made once per element type"""
    if kind not in _FRAMES:
        dt, shape, row_bytes = _ROWS[kind]
        g = torch.Generator(device="cpu").manual_seed(7)
        if dt == torch.uint8:
            f = torch.randint(1, 256, (3, 5) + shape, generator=g, dtype=torch.uint8)
        else:
            f = (torch.randn((3, 5) + shape, generator=g) + 3.0).to(dt)
        assert f[0, 0].numel() * f.element_size() == row_bytes
        _FRAMES[kind] = f.to(dev)
    return _FRAMES[kind]


@pytest.mark.parametrize("kind", ["u8", "bf16", "fp32"])
@pytest.mark.parametrize("capacity", [15, 8])
@pytest.mark.parametrize("num_imgs", [[5, 5, 5], [2, 0, 4], [1, 1, 1]], ids=["full", "gap", "ones"])
def test_pack_frames_is_the_reference_concatenation(num_imgs, capacity, kind):
    """packed[:n] is bit-identical to torch.cat([frames[u, :n_u]]), the tail all zero, counts == [min(total, capacity), total]; 15 frames into a
    capacity of 8: the first 8, counts == [8, 15], and no error from the runtime"""
    from facialmmt_amd import ops
    dev = torch.device("cuda:0")
    frames = _loader_frames(kind, dev)
    packed, counts = ops.pack_frames(frames, torch.tensor(num_imgs, device=dev), capacity)
    torch.cuda.synchronize()                                   # a fault of the launch would surface here
    total = sum(num_imgs)
    n = min(total, capacity)
    assert counts.dtype == torch.int32 and counts.tolist() == [n, total]
    assert packed.shape == (capacity,) + tuple(frames.shape[2:]) and packed.dtype == frames.dtype
    want = torch.cat([frames[u, :k] for u, k in enumerate(num_imgs)], dim=0)[:n]
    as_bytes = lambda t: t.contiguous().view(torch.uint8)
    assert torch.equal(as_bytes(packed[:n]), as_bytes(want))
    assert int(as_bytes(packed[n:]).max()) == 0 if n < capacity else True
    if num_imgs == [5, 5, 5] and capacity == 8:
        assert counts.tolist() == [8, 15]


def test_pack_frames_clamps_counts_and_refuses_unaligned_rows():
    from facialmmt_amd import _lib, ops
    dev = torch.device("cuda:0")
    frames = _loader_frames("u8", dev)
    packed, counts = ops.pack_frames(frames, [9, -3, 2], 15)    # a list, as the reference's collate yields; counts clamp to [0, Lv]
    assert counts.tolist() == [7, 7]
    assert torch.equal(packed[:7], torch.cat((frames[0, :5], frames[2, :2]))) and int(packed[7:].max()) == 0
    with pytest.raises(_lib.FmmtError, match="FMMT_EALIGN"):
        ops.pack_frames(torch.zeros(2, 3, 40, dtype=torch.uint8, device=dev), [1, 1], 4)


# ------------------------------------------------------------------------------------------------ frame filter
def _filter_case(case):
    """B = 2, Lv = 6, num_imgs = [5, 2], F_cap = 12: preds (12, 7) whose rows 7.. are padding.  'mixed': some real faces pass the threshold;
    'padded_only': every real face near-uniform (importance ~ 1/7 < 0.5), every padded row one-hot (importance 1)."""
    g = torch.Generator().manual_seed(11)
    B, Lv, D, NL, cap, num_imgs, thr = 2, 6, 16, 7, 12, [5, 2], 0.5
    n = sum(num_imgs)
    near_uniform = torch.softmax(0.05 * torch.randn(cap, NL, generator=g), dim=1)
    one_hot = torch.eye(NL)[torch.randint(0, NL, (cap,), generator=g)] * 0.97 + 0.03 / NL
    if case == "mixed":
        passes = torch.tensor([1, 0, 1, 1, 0, 0, 1] + [1, 0, 1, 0, 1], dtype=torch.bool)
    else:
        passes = torch.tensor([0] * n + [1] * (cap - n), dtype=torch.bool)
    preds = torch.where(passes.view(-1, 1), one_hot, near_uniform)
    vin = torch.randn(B, Lv, D, generator=g)
    vmask = torch.zeros(B, Lv)
    for u, k in enumerate(num_imgs):
        vmask[u, :k] = 1
    dout = torch.randn(B, Lv, D + NL, generator=g)
    return preds, vin, vmask, num_imgs, thr, n, dout


@pytest.mark.parametrize("kernel", [True, False], ids=["kernel", "torch"])
@pytest.mark.parametrize("case", ["mixed", "padded_only"])
def test_select_frames_ignores_padded_rows(case, kernel, monkeypatch):
    from facialmmt_amd import train_step
    from oracle.train_glue import select_frames_loop
    dev = torch.device("cuda:0")
    preds, vin, vmask, num_imgs, thr, n, dout = _filter_case(case)
    pr = preds[:n].clone().requires_grad_(True)
    want, want_mask = select_frames_loop(pr, vin, vmask, num_imgs, thr)
    (want * dout).sum().backward()
    monkeypatch.setattr(train_step, "SELECT_FRAMES_KERNEL", kernel)
    pd = preds.to(dev).requires_grad_(True)
    nv = torch.tensor([n, n], dtype=torch.int32, device=dev)
    got, got_mask = train_step.select_frames(pd, vin.to(dev), vmask.to(dev), torch.tensor(num_imgs, device=dev), thr, n_valid=nv)
    (got * dout.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(got.detach().cpu(), want.detach()) and torch.equal(got_mask.cpu(), want_mask)
    assert torch.equal(pd.grad[:n].cpu(), pr.grad)
    assert float(pd.grad[n:].abs().max()) == 0.0
    if case == "padded_only":                                   # the keep-everything branch, bit for bit
        assert torch.equal(got_mask.cpu(), vmask) and torch.equal(got[..., :vin.shape[2]].detach().cpu(), vin)
        # without n_valid the padded rows flip the batch into the selection branch: the case does discriminate
        other, other_mask = train_step.select_frames(preds.to(dev), vin.to(dev), vmask.to(dev), torch.tensor(num_imgs, device=dev), thr)
        assert not torch.equal(other_mask.cpu(), vmask)
