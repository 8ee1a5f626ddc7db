"""ops.ce_loss (csrc/ce_loss.hip: class-weighted, label-smoothed mean cross-entropy of (B, NL) logits, one launch per direction) against the fp64 CPU
result of train_step.Criterion.reference (held to torch.nn.CrossEntropyLoss in tests/test_criterion_cpu.py).

Shapes: B in {1, 3, 64, 150, 1024, 1025, 2500} (one leaf, a partial wave, a full 1024-leaf tree, the second and third row per leaf), NL in {2, 7, 8},
fp32 and bf16 logits (bf16 values are rounded BEFORE the reference sees them), rows `ld` apart with ld = NL and ld = 8; weights none / random in [0.2, 3] /
one class at 0; eps 0 and 0.1; 0, 1 and B - 1 ignored rows.
Bars.  fp32: the error of torch's own fp32 F.cross_entropy autograd on the same device inputs against the same fp64 result is measured, 4 x that error is
allowed (the factor covers the other summation order over B), never less than 2e-6 of the tensor's scale (about 30 fp32 roundings, in the row and the
10-level tree, at 6e-8 each).  bf16 d(logits): one bf16 rounding, 2^-8 of the scale, on top of the fp32 bar.  den: 1e-6 relative."""
import pytest
import torch

from tests import support_criterion as SC

pytestmark = pytest.mark.gpu

BS = [1, 3, 64, 150, 1024, 1025, 2500]
NLS = [2, 7, 8]
FLOOR, FACTOR, BF16_ROUNDING = 2e-6, 4.0, 2.0 ** -8
DLOSS = 0.37


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def reference(x64, y, w, eps):
    """fp64 on the CPU: (loss, d(logits) for an upstream gradient DLOSS, den)"""
    from facialmmt_amd.train_step import Criterion
    x = x64.clone().requires_grad_(True)
    loss = Criterion(w, eps, device="cpu").reference(x, y)
    (g,) = torch.autograd.grad(loss * DLOSS, x)
    NL = x.shape[1]
    valid = (y >= 0) & (y < NL)
    wy = (torch.ones(NL, dtype=torch.float64) if w is None else w.double())[y.clamp(0, NL - 1)]
    return float(loss.detach()), g, float((valid.double() * wy).sum())


def strided(x, ld, dev, dtype):
    """the (B, NL) device logits as a view of a (B, ld) buffer"""
    B, NL = x.shape
    buf = torch.full((B, ld), 777.0, dtype=dtype, device=dev)
    buf[:, :NL] = x.to(dev).to(dtype)
    return buf[:, :NL]


def run_op(xd, yd, wd, eps):
    from facialmmt_amd import ops
    leaf = xd.detach().requires_grad_(True)
    loss = ops.ce_loss(leaf, yd, wd, eps)
    (g,) = torch.autograd.grad(loss * DLOSS, leaf)
    _, den = ops.ce_fwd_raw(xd, yd, wd, eps)
    return loss.detach(), g, den


def torch_fp32(x32d, yd, wd, eps):
    NL = x32d.shape[1]
    leaf = x32d.detach().clone().requires_grad_(True)
    lab = torch.where((yd >= 0) & (yd < NL), yd, torch.full_like(yd, -100))
    loss = torch.nn.functional.cross_entropy(leaf, lab, weight=wd, label_smoothing=eps)
    (g,) = torch.autograd.grad(loss * DLOSS, leaf)
    return float(loss.detach()), g


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("NL", NLS)
@pytest.mark.parametrize("B", BS)
def test_forward_and_backward_against_fp64(dev, B, NL, dtype):
    worst = dict(loss=(0.0, 0.0), grad=(0.0, 0.0))             # (ours, torch fp32) relative to the scale
    for ld in sorted({NL, 8}):
        for kind in SC.WEIGHT_KINDS:
            for eps in (0.0, 0.1):
                for ignored in ("none", "one", "all_but_one"):
                    label = f"B={B} NL={NL} {dtype} ld={ld} {kind} eps={eps} ignored={ignored}"
                    w = SC.weights_for(kind, NL)
                    x32, y = SC.logits_and_labels(B, NL, seed=11, ignored=ignored)
                    x64 = x32.to(dtype).double()                                   # what the kernel reads
                    want, gwant, den = reference(x64, y, w, eps)
                    xd, yd = strided(x32, ld, dev, dtype), y.to(dev)
                    wd = None if w is None else w.to(dev)
                    loss, g, dden = run_op(xd, yd, wd, eps)
                    assert loss.dtype == torch.float32 and g.dtype == dtype and g.shape == (B, NL) and torch.isfinite(g).all(), label
                    assert abs(float(dden) - den) <= 1e-6 * max(den, 1e-30), (label, float(dden), den)
                    if den == 0.0:
                        assert float(loss) == 0.0 and float(g.abs().max()) == 0.0, label
                        continue
                    t_loss, t_g = torch_fp32(x64.float().to(dev), yd, wd, eps)
                    ls, gs = abs(want), float(gwant.abs().max())
                    t_le, t_ge = abs(t_loss - want), float((t_g.double().cpu() - gwant).abs().max())
                    le, ge = abs(float(loss) - want), float((g.double().cpu() - gwant).abs().max())
                    lbar = max(FACTOR * t_le, FLOOR * ls)
                    gbar = max(FACTOR * t_ge, FLOOR * gs) + (BF16_ROUNDING * gs if dtype == torch.bfloat16 else 0.0)
                    worst["loss"] = max(worst["loss"], (le / ls, t_le / ls))
                    worst["grad"] = max(worst["grad"], (ge / gs, t_ge / gs))
                    assert le <= lbar, (label, "loss", le, lbar, t_le)
                    assert ge <= gbar, (label, "d(logits)", ge, gbar, t_ge)
                    valid = (y >= 0) & (y < NL)
                    if (~valid).any():
                        assert float(g[(~valid).to(dev)].abs().max()) == 0.0, label
    print(f"B={B} NL={NL} {dtype}: worst loss error {worst['loss'][0]:.3e} of scale (torch fp32 {worst['loss'][1]:.3e}); "
          f"worst d(logits) error {worst['grad'][0]:.3e} of scale (torch fp32 {worst['grad'][1]:.3e})")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [150, 2500])
def test_two_runs_are_bit_equal(dev, B, dtype):
    w = SC.weights_for("random", 7).to(dev)
    x32, y = SC.logits_and_labels(B, 7, seed=12, ignored="one")
    xd, yd = x32.to(dev).to(dtype), y.to(dev)
    a = [t.clone() for t in run_op(xd, yd, w, 0.1)]
    b = run_op(xd, yd, w, 0.1)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_den_zero_gives_zeros_and_nothing_non_finite(dev, eps):
    x32, _ = SC.logits_and_labels(5, 7, seed=13)
    xd = x32.to(dev)
    w0 = torch.tensor([1.0, 0.0, 2.0, 1.0, 1.0, 1.0, 1.0], device=dev)
    for wd, y in ((None, torch.full((5,), -100)), (w0, torch.tensor([1, 1, -100, 1, 9]))):
        loss, g, den = run_op(xd, y.to(dev), wd, eps)
        assert float(loss) == 0.0 and float(den) == 0.0 and float(g.abs().max()) == 0.0 and torch.isfinite(g).all()


def test_a_weight_tensor_changed_in_place_changes_the_next_call(dev):
    from facialmmt_amd.train_step import Criterion
    x32, y = SC.logits_and_labels(9, 7, seed=14)
    crit = Criterion(SC.weights_for("random", 7), 0.1, device=dev)
    xd, yd = x32.to(dev), y.to(dev)
    first, ptr = float(crit(xd, yd)), crit.weight.data_ptr()
    new = SC.weights_for("random", 7, seed=5)
    crit.weight.copy_(new)
    second = crit(xd, yd)
    from facialmmt_amd import ops
    assert crit.weight.data_ptr() == ptr and first != float(second)
    assert torch.equal(second, ops.ce_loss(xd, yd, new.to(dev), 0.1))          # the bits of a call that was given the new weights outright


def test_bad_arguments(dev):
    from facialmmt_amd import _lib, ops
    x, y = torch.zeros(4, 7, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    assert abs(float(ops.ce_loss(x, y)) - 1.9459101) < 1e-6
    for call in (lambda: ops.ce_loss(x.cpu(), y), lambda: ops.ce_loss(torch.zeros(4, 9, device=dev), y), lambda: ops.ce_loss(x, y[:3]),
                 lambda: ops.ce_loss(x, y, torch.ones(6, device=dev)), lambda: ops.ce_loss(x, y, torch.ones(7)), lambda: ops.ce_loss(x, y, None, 1.0),
                 lambda: ops.ce_loss(x.half(), y), lambda: ops.ce_loss(x, y, torch.ones(7, device=dev, dtype=torch.float64))):
        with pytest.raises(_lib.FmmtError):
            call()


def test_the_registered_operator_is_the_function(dev):
    import facialmmt_amd.torch_ops  # noqa: F401
    w = SC.weights_for("random", 7).to(dev)
    x32, y = SC.logits_and_labels(150, 7, seed=15, ignored="one")
    xd, yd = x32.to(dev), y.to(dev)
    loss, g, den = run_op(xd, yd, w, 0.1)
    leaf = xd.clone().requires_grad_(True)
    l2, d2 = torch.ops.fmmt.ce_loss(leaf, yd, w, 0.1)
    (g2,) = torch.autograd.grad(l2 * DLOSS, leaf)
    assert torch.equal(l2.detach(), loss) and torch.equal(d2, den) and torch.equal(g2, g)
    torch.library.opcheck(torch.ops.fmmt.ce_loss.default, (xd.clone().requires_grad_(True), yd, w, 0.1), test_utils=("test_schema", "test_faketensor"))


def test_replays_inside_a_captured_graph_follow_labels_and_weights(dev):
    """ONE small captured graph, forward and backward, replayed with the logits, the labels and the weight tensor rewritten in place between the
    replays: each replay gives the bits of the same call issued eagerly"""
    from facialmmt_amd import ops
    from facialmmt_amd.graph_capture import _KEEP_GRAPHS, capture_window
    from facialmmt_amd.train_step import Criterion
    B, NL = 150, 7
    crit = Criterion(SC.weights_for("random", NL), 0.1, device=dev)
    s_x = torch.zeros(B, NL, device=dev, requires_grad=True)
    s_y = torch.zeros(B, dtype=torch.int64, device=dev)

    def body():
        loss = crit(s_x, s_y)
        (g,) = torch.autograd.grad(loss * DLOSS, s_x)
        return loss.detach(), g
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        body()                                                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with capture_window():
        with torch.cuda.graph(graph, stream=stream):
            c_loss, c_g = body()
    for i, (kind, ignored) in enumerate((("random", "none"), ("zero_class", "one"), ("random", "all_but_one"))):
        x32, y = SC.logits_and_labels(B, NL, seed=20 + i, ignored=ignored)
        w = SC.weights_for(kind, NL, seed=i)
        with torch.no_grad():
            s_x.copy_(x32.to(dev))
        s_y.copy_(y.to(dev))
        crit.weight.copy_(w)
        graph.replay()
        torch.cuda.synchronize(dev)
        loss, g, _ = run_op(s_x.detach(), s_y, crit.weight, 0.1)
        assert torch.equal(c_loss, loss) and torch.equal(c_g, g), (kind, ignored)
        assert torch.equal(loss, ops.ce_loss(x32.to(dev), y.to(dev), w.to(dev), 0.1))       # ... which saw this replay's logits, labels and weights
    _KEEP_GRAPHS.append((graph,))
