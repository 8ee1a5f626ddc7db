"""The strided-operand helper and its checker (tests/support_strided.py), driven on the CPU by torch stand-ins for a GEMM kernel that address memory the
way a kernel does -- a flat buffer, a base offset, m * ld + n: the right one must pass, and each of three deliberately wrong ones must be flagged."""
import pytest
import torch

from tests import support_strided as SS
from tests.support_gemm_cases import layout_of

M, N, K = 37, 24, 16
LAYOUTS = ["contig", "pitch", "packed"]


def _operands(dtype, lay):
    g = torch.Generator().manual_seed(5)
    xv = torch.randn(M, K, generator=g).to(dtype)
    wv = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    mk = lambda rows, width, **kw: SS.make(rows, width, dtype, "cpu", **dict(zip(("ld", "col"), layout_of(lay, width))), **kw)
    return mk(M, K, values=xv), mk(N, K, values=wv), mk(M, N, output=True), xv, wv


def _gemm(x, w, y, *, ldy=None, kread=K, stray=None):
    """y[m * ldy + n] = sum_{k < kread} x[m * ldx + k] w[n * ldw + k] on the flat buffers, as a kernel addresses them"""
    xf, wf, yf = x.flat(), w.flat(), y.flat()
    ldy = y.ld if ldy is None else ldy
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[None, :], torch.arange(kread)
    xa = xf[x.offset + torch.arange(M)[:, None] * x.ld + k[None, :]].double()
    wa = wf[w.offset + torch.arange(N)[:, None] * w.ld + k[None, :]].double()
    yf[y.offset + m * ldy + n] = (xa @ wa.t()).to(yf.dtype)
    if stray is not None:
        yf[y.offset + stray] = 0.5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("lay", LAYOUTS)
def test_right_stand_in_passes(dtype, lay):
    x, w, y, xv, wv = _operands(dtype, lay)
    _gemm(x, w, y)
    assert y.problems() == []
    assert torch.equal(y.view, (xv.double() @ wv.double().t()).to(dtype))
    # the helper built what it promises: NaN / Inf around inputs, a 16-byte aligned base, one Inf in the padding of every row
    assert x.ptr % 16 == 0 and y.ptr % 16 == 0 and x.buf.shape[0] == M + 2 * SS.GUARD
    outside = torch.ones_like(x.buf, dtype=torch.bool)
    outside[SS.GUARD:SS.GUARD + M, x.col:x.col + K] = False
    assert not torch.isfinite(x.buf[outside]).any() and torch.isfinite(x.view).all()
    if lay != "contig":
        assert (torch.isinf(x.buf).sum(1) == 1).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("lay", ["pitch", "packed"])
def test_stand_in_that_ignores_ldy_is_flagged(dtype, lay):
    x, w, y, _, _ = _operands(dtype, lay)
    _gemm(x, w, y, ldy=N)                                       # rows at m * N: lands in the padding and leaves region elements unwritten
    p = y.problems()
    assert any("stray write" in s for s in p) and any("not finite" in s for s in p), p


# (a contiguous row has no padding beside it -- column N is row m + 1 --: no such case)
@pytest.mark.parametrize("lay,where", [(lay, where) for lay in LAYOUTS for where in ("row M", "column N", "row -1") if (lay, where) != ("contig", "column N")])
def test_stand_in_that_writes_one_padding_element_is_flagged(lay, where):
    x, w, y, _, _ = _operands(torch.bfloat16, lay)
    stray = {"row M": M * y.ld, "column N": 3 * y.ld + N, "row -1": -y.ld + N - 1}[where]
    _gemm(x, w, y, stray=stray)
    p = y.problems()
    assert len(p) == 1 and p[0].startswith("stray write: 1 element"), p


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("lay", ["pitch", "packed"])
def test_stand_in_that_contracts_one_padded_column_is_flagged(dtype, lay):
    x, w, y, _, _ = _operands(dtype, lay)
    _gemm(x, w, y, kread=K + 1)                                 # an over-read K tail that enters the sum
    p = y.problems()
    assert len(p) == 1 and "not finite" in p[0], p


def test_a_value_equal_to_the_padding_pattern_is_still_compared_bitwise():
    """-0.0 == 0.0 and NaN != NaN as floats; the integer view sees a changed sign bit and does not trip over a NaN pattern"""
    y = SS.make(4, 8, torch.float32, "cpu", ld=16, output=True)
    y.view.fill_(1.0)
    assert y.problems() == []
    y.buf[SS.GUARD, 9] = 1.23                                     # the same VALUE as the fill pattern 0x3F9D70A4: no change of bits, no finding
    assert y.problems() == []
    y.buf.view(torch.int32)[SS.GUARD, 9] += 1                     # one ulp
    assert len(y.problems()) == 1
