"""CPU tests of the criterion (class-weighted, label-smoothed cross-entropy as a construction argument of the training steps):
train_step.Criterion.reference against torch.nn.CrossEntropyLoss(weight, label_smoothing) in fp64 (both sides fp64: 1e-12 of scale), its den == 0 rule and its
invariance under a rescaling of the weights; argument validation (Criterion, global_rows with class weights as a pure host function); the fp64 restatement of
the pooling head under the criterion (tests/support_criterion.head_reference_crit) against autograd through CrossEntropyLoss; and the ABI surface of
include/fmmt_loss.h (header == _lib.LOSS_SIGNATURES == the built library, argument validation in front of any launch)."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import support_criterion as SC
from tests import support_unimodal_oracle as UO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12


def _lib_built():
    from facialmmt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def _torch_loss(x, y, w, eps):
    NL = x.shape[1]
    lab = torch.where((y >= 0) & (y < NL), y, torch.full_like(y, -100))
    return torch.nn.CrossEntropyLoss(weight=None if w is None else w.double(), label_smoothing=eps)(x, lab)


@pytest.mark.parametrize("ignored", ["none", "one", "all_but_one"])
@pytest.mark.parametrize("kind", SC.WEIGHT_KINDS)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("NL", [2, 7, 8])
@pytest.mark.parametrize("B", [1, 4, 9])
def test_reference_is_torchs_cross_entropy_loss_in_fp64(B, NL, eps, kind, ignored):
    from facialmmt_amd.train_step import Criterion
    w = SC.weights_for(kind, NL)
    x32, y = SC.logits_and_labels(B, NL, seed=3, ignored=ignored)
    crit = Criterion(w, eps, device="cpu")
    x = x32.double().requires_grad_(True)
    loss = crit.reference(x, y)
    (g,) = torch.autograd.grad(loss, x)
    loss = loss.detach()
    assert loss.dtype == torch.float64 and g.shape == x.shape
    valid = (y >= 0) & (y < NL)
    den = float((valid.double() * (torch.ones(NL) if w is None else w).double()[y.clamp(0, NL - 1)]).sum())
    if den == 0.0:                                            # the stated departure: torch gives NaN here
        assert float(loss) == 0.0 and float(g.abs().max()) == 0.0
        return
    xt = x32.double().requires_grad_(True)
    want = _torch_loss(xt, y, w, eps)
    (gt,) = torch.autograd.grad(want, xt)
    want = want.detach()
    scale_l, scale_g = max(1.0, abs(float(want))), max(float(gt.abs().max()), 1e-300)
    print(f"B={B} NL={NL} eps={eps} {kind} {ignored}: loss err {abs(float(loss) - float(want)):.2e}, grad err {float((g - gt).abs().max()):.2e}")
    assert abs(float(loss) - float(want)) <= BAR * scale_l
    assert float((g - gt).abs().max()) <= BAR * max(1.0, scale_g)
    if (~valid).any():
        assert float(g[~valid].abs().max()) == 0.0


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_den_zero_gives_loss_zero_and_gradient_zero(eps):
    """no labelled row at all; and every labelled row of a class whose weight is 0 (with smoothing the numerator is not zero there, the loss still is)"""
    from facialmmt_amd.train_step import Criterion
    x32, y = SC.logits_and_labels(4, 7, seed=5)
    for w, lab in ((None, torch.full_like(y, -100)), (SC.weights_for("random", 7), torch.tensor([-100, 9, -1, 7])),
                   (torch.tensor([1.0, 0.0, 2.0, 1.0, 1.0, 1.0, 1.0]), torch.tensor([1, 1, -100, 1]))):
        x = x32.double().requires_grad_(True)
        loss = Criterion(w, eps, device="cpu").reference(x, lab)
        (g,) = torch.autograd.grad(loss, x)
        assert float(loss) == 0.0 and float(g.abs().max()) == 0.0 and torch.isfinite(g).all()


@pytest.mark.parametrize("kind", ["random", "zero_class"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_scaling_the_weights_changes_nothing(kind, eps):
    """a weighted MEAN: w -> c w leaves loss and gradient where they are (a forgotten den does not)"""
    from facialmmt_amd.train_step import Criterion
    w = SC.weights_for(kind, 7).double()
    x32, y = SC.logits_and_labels(9, 7, seed=8, ignored="one")
    out = []
    for c in (1.0, 4.0, 0.125):                                # powers of two: the fp32 weights scale exactly
        x = x32.double().requires_grad_(True)
        loss = Criterion(w * c, eps, device="cpu").reference(x, y)
        out.append((float(loss), torch.autograd.grad(loss, x)[0]))
    for l, g in out[1:]:
        assert abs(l - out[0][0]) <= BAR * max(1.0, abs(out[0][0])) and float((g - out[0][1]).abs().max()) <= BAR


def test_criterion_validates_its_arguments():
    from facialmmt_amd.train_step import Criterion, _check_criterion
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Criterion(None, bad, device="cpu")
    for bad in ([1.0, -0.5, 1.0], [1.0, float("nan")], [float("inf"), 1.0], [[1.0, 2.0]], [], [1.0] * 9):
        with pytest.raises(ValueError):
            Criterion(bad, 0.0, device="cpu")
    c = Criterion([1.0, 2.0, 0.0], 0.25, device="cpu")
    assert c.weight.dtype == torch.float32 and c.weight.tolist() == [1.0, 2.0, 0.0] and c.label_smoothing == 0.25 and c.num_labels == 3
    with pytest.raises(ValueError):                            # a wrong length for the logits it is given
        c.reference(torch.zeros(2, 7, dtype=torch.float64), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        _check_criterion(c, 7)
    with pytest.raises(ValueError):
        _check_criterion(torch.nn.CrossEntropyLoss())
    assert _check_criterion(None, 7) is None and _check_criterion(c, 3) is c
    assert Criterion(None, 0.0, device="cpu").weight is None and Criterion(None, 0.0, device="cpu").num_labels is None
    # the weight is ONE tensor: an in-place copy is what the next call computes with
    x, y = torch.tensor([[0.5, -1.0, 2.0]], dtype=torch.float64), torch.tensor([1])
    before, ptr = float(c.reference(x, y)), c.weight.data_ptr()
    c.weight.copy_(torch.tensor([1.0, 2.0, 5.0]))
    assert c.weight.data_ptr() == ptr and float(c.reference(x, y)) != before
    # on the CPU calling it is the reference
    assert float(c(x, y)) == float(c.reference(x, y))


def test_global_rows_with_class_weights_is_refused_on_the_host():
    from facialmmt_amd.train_step import Criterion, check_criterion_rows
    weighted, smoothed = Criterion([1.0, 2.0], 0.0, device="cpu"), Criterion(None, 0.1, device="cpu")
    with pytest.raises(ValueError, match="global_rows"):
        check_criterion_rows("GraphedTargetStep", weighted, 7)
    with pytest.raises(ValueError, match="global_rows"):
        check_criterion_rows("GraphedAuxStep", Criterion([1.0, 1.0], 0.1, device="cpu"), 1)
    for crit, rows in ((weighted, None), (smoothed, 7), (smoothed, None), (None, 7), (None, None)):
        assert check_criterion_rows("GraphedUnimodalStep", crit, rows) is None


@pytest.mark.parametrize("unlabelled", [0, 1, 2, 3])
@pytest.mark.parametrize("kind,eps", [("none", 0.0), ("random", 0.1), ("zero_class", 0.1), ("random", 0.0)])
def test_head_reference_crit_against_autograd(kind, eps, unlabelled):
    """the fp64 restatement the GPU head test compares with, held to autograd through CrossEntropyLoss on a random keep mask (1e-10 of scale, the bar
    tests/test_unimodal_oracle_cpu.py holds head_reference to)"""
    from tests import support_pad_rows as PR
    B, L, H, NL = 3, 7, 8, 7
    cpu, _ = UO.head_inputs(B, L, H, NL, 40)
    cpu = PR.pad_head_inputs(cpu, unlabelled)
    g = torch.Generator().manual_seed(5)
    keep = (torch.rand(B, H, generator=g) > 0.3).double() / 0.7
    w = SC.weights_for(kind, NL)
    got = SC.head_reference_crit(**cpu, keep=keep, weight=w, eps=eps, dloss=0.37)
    if unlabelled == B:
        assert float(got["loss"]) == 0.0 and all(float(got[k].abs().max()) == 0.0 for k in ("dh", "dph", "dqq", "dv", "dvb", "dW", "db"))
        return
    want = SC.head_autograd_crit(**cpu, keep=keep, weight=w, eps=eps, dloss=0.37)
    for k, r in want.items():
        scale = max(float(r.abs().max()), 1e-3)
        assert float((got[k] - r).abs().max()) <= 1e-10 * scale, (k, float((got[k] - r).abs().max()), scale)
    if kind == "none" and eps == 0.0:                          # and it is head_reference_rows where the criterion is the plain loss
        rows = PR.head_reference_rows(**cpu, keep=keep, dloss=0.37)
        for k in ("loss", "dh", "dph", "dqq", "dv", "dW", "db"):
            assert float((got[k] - rows[k]).abs().max()) <= 1e-12 * max(float(rows[k].abs().max()), 1e-3), k


def test_loss_header_signatures_and_library_agree():
    """include/fmmt_loss.h (included by fmmt.h, listed in build.py) == _lib.LOSS_SIGNATURES == the symbols of the built library: name, every argument's type and
    the return type; the table is disjoint from every other *SIGNATURES table, and _lib.SIGNATURES keeps its 59 names"""
    from facialmmt_amd import _lib, build
    assert "ce_loss.hip" in build.SOURCES
    assert "fmmt_loss.h" in open(os.path.join(ROOT, "facialmmt_amd", "build.py")).read()
    assert '#include "fmmt_loss.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    raw = open(os.path.join(ROOT, "include", "fmmt_loss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.LOSS_SIGNATURES) == ["fmmt_ce_bwd", "fmmt_ce_fwd", "fmmt_pool_head_bwd_crit", "fmmt_pool_head_fwd_crit"]
    others = [n for n in dir(_lib) if n.endswith("SIGNATURES") and n != "LOSS_SIGNATURES"]
    assert len(others) >= 13
    for n in others:
        assert not set(_lib.LOSS_SIGNATURES) & set(getattr(_lib, n)), n
    assert len(_lib.SIGNATURES) == 59

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    lib = _lib_built()
    for name, (res, got) in _lib.LOSS_SIGNATURES.items():
        assert got == [ctype_of(a) for a in protos[name].split(",") if a.strip()], name
        assert res is C.c_int and re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name), name
    # the _crit pair is the _rows pair with class_w and smoothing added and a float word in the count's place
    for d in ("fwd", "bwd"):
        rows, crit = _lib.POOL_HEAD_ROWS_SIGNATURES[f"fmmt_pool_head_{d}_rows"][1], _lib.LOSS_SIGNATURES[f"fmmt_pool_head_{d}_crit"][1]
        assert len(crit) == len(rows) + 2
    assert "train.py:295" in raw and "den == 0" in raw


def test_arguments_are_validated_before_any_launch():
    """FMMT_EINVAL comes back without a device: NULL pointers, NL / B / ld / smoothing out of range, another dtype; class_w may be NULL"""
    from facialmmt_amd import _lib
    lib = _lib_built()
    buf = (C.c_char * 1024)()
    p = C.addressof(buf)
    p += -p % 16

    def fwd(dtype=0, B=4, NL=7, logits=p, ld=7, labels=p + 256, class_w=None, eps=0.0, loss=p + 512, den=p + 516):
        return lib.fmmt_ce_fwd(dtype, B, NL, logits, ld, labels, class_w, eps, loss, den, None)

    def bwd(dtype=0, B=4, NL=7, logits=p, ld=7, labels=p + 256, class_w=None, eps=0.0, dloss=p + 512, den=p + 516, dlogits=p + 640, ld_d=7):
        return lib.fmmt_ce_bwd(dtype, B, NL, logits, ld, labels, class_w, eps, dloss, den, dlogits, ld_d, None)
    common = (dict(dtype=2), dict(dtype=-1), dict(B=0), dict(B=-3), dict(B=65537), dict(NL=0), dict(NL=9), dict(ld=6), dict(ld=0), dict(eps=-0.01),
              dict(eps=1.0), dict(eps=float("nan")), dict(logits=None), dict(labels=None), dict(den=None))
    for bad in common + (dict(loss=None),):
        assert fwd(**bad) == _lib.FMMT_EINVAL, bad
    for bad in common + (dict(dloss=None), dict(dlogits=None), dict(ld_d=6)):
        assert bwd(**bad) == _lib.FMMT_EINVAL, bad
    # the head: the _rows pair's shape checks first, then den and the smoothing
    f = lambda **kw: lib.fmmt_pool_head_fwd_crit(kw.get("dtype", 0), 4, kw.get("L", 160), 768, kw.get("NL", 7), *([None] * 9), 0.0, 0, *([None] * 6), None,
                                                 kw.get("eps", 0.0), kw.get("den", None), None, 0, None)
    b = lambda **kw: lib.fmmt_pool_head_bwd_crit(kw.get("dtype", 1), 4, kw.get("L", 160), 768, kw.get("NL", 7), *([None] * 11), None, kw.get("eps", 0.0),
                                                 kw.get("den", None), *([None] * 8), 0, None)
    for call in (f, b):
        for kw in (dict(), dict(L=1), dict(NL=9), dict(dtype=5), dict(den=p), dict(den=p, eps=1.0), dict(den=p, eps=-1.0)):
            assert call(**kw) == _lib.FMMT_EINVAL, kw            # (den given: the NULL operands behind it)
