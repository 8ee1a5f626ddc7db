"""GPU tests of the replica digest (csrc/digest.hip, include/fmmt_digest.h): ops.param_digest on hand-built descriptor tables against the numpy uint64
restatement tests/support_digest.py, element for element of the six words, and FusedClipAdamW.digest() on the table the optimizer built itself.

Sizes: n in {1, 3, 4095, 4096, 4097, 3 * 4096 + 5} -- below one 16-byte load, one short of a block, a block exactly (the vector path), one past it, and
several blocks with a tail -- alone and three to a table (the tensor number enters S2).  The values are random BIT patterns (NaNs and denormals
included): the digest is over bits, not numbers."""
import numpy as np
import pytest
import torch

from tests import support_digest as SD

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4095, 4096, 4097, 3 * 4096 + 5)
TABLES = [(n,) for n in SIZES] + [(1, 4097, 3), (4095, 4096, 3 * 4096 + 5), (4096, 1, 4096)]


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def _state(sizes, seed=0, offset=0):
    """host (p, m, v) lists of random bit patterns and their device copies; `offset`: every device tensor starts that many elements into its
    allocation (offset 1: no 16-byte alignment, so full blocks go element by element too)"""
    dev = torch.device("cuda:0")
    host = [[_bits(n, seed + 100 * k + j) for j, n in enumerate(sizes)] for k in range(3)]
    on_dev = [[torch.cat((torch.zeros(offset, dtype=torch.int32), torch.from_numpy(a.view(np.int32)))).to(dev)[offset:].view(torch.float32)
               for a in arrays] for arrays in host]                          # moved as integers: no payload of a NaN is touched on the way
    return host, on_dev


def _digest(on_dev, stream=None):
    from facialmmt_amd import ops
    ps, ms, vs = on_dev
    raw, blocks = SD.table([(p.data_ptr(), 0, m.data_ptr(), v.data_ptr(), p.numel()) for p, m, v in zip(ps, ms, vs)])
    desc = torch.from_numpy(raw).to(ps[0].device)
    if stream is None:
        out = ops.param_digest(len(ps), blocks, desc)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out = ops.param_digest(len(ps), blocks, desc)
        torch.cuda.current_stream().wait_stream(stream)
    assert out.dtype == torch.int64 and out.shape == (6,) and out.is_cuda
    return SD.as_unsigned(out.cpu().numpy())


@pytest.mark.parametrize("sizes", TABLES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("offset", [0, 1])
def test_digest_equals_the_numpy_restatement(sizes, offset):
    host, on_dev = _state(sizes, seed=sum(sizes), offset=offset)
    got, want = _digest(on_dev), SD.digest(*host)
    print("sizes", sizes, "offset", offset, "got", [hex(w) for w in got], "want", [hex(w) for w in want])
    assert got == want


def test_what_changes_which_word():
    """one flipped bit of one element: both words of that quantity and no other; two unequal elements swapped: S2 alone; +0.0 against -0.0: both"""
    sizes = (4097, 3)
    host, on_dev = _state(sizes, seed=5)
    base = _digest(on_dev)
    for k in range(3):                                       # p, m, v in turn: element 4096 of tensor 0 (the block's scalar tail)
        t = on_dev[k][0].view(torch.int32)
        old = t[4096:4097].clone()
        t[4096:4097] = old ^ (1 << 7)
        got = _digest(on_dev)
        changed = [i for i in range(6) if got[i] != base[i]]
        print("flip in quantity", k, "changed words", changed)
        assert changed == [2 * k, 2 * k + 1]
        t[4096:4097] = old
        assert _digest(on_dev) == base
    t = on_dev[1][0].view(torch.int32)                       # swap elements 10 and 2000 of m, tensor 0
    assert t[10] != t[2000]
    a, b = t[10:11].clone(), t[2000:2001].clone()
    t[10:11], t[2000:2001] = b, a
    got = _digest(on_dev)
    assert [i for i in range(6) if got[i] != base[i]] == [3]
    t[10:11], t[2000:2001] = a, b
    t = on_dev[0][1]                                         # tensor 1 of p: +0.0 against -0.0 in element 2
    t[2:3] = 0.0
    plus = _digest(on_dev)
    t[2:3] = -0.0
    minus = _digest(on_dev)
    assert [i for i in range(6) if plus[i] != minus[i]] == [0, 1]
    assert (minus[0] - plus[0]) % (1 << 64) == 0x80000000 and (minus[1] - plus[1]) % (1 << 64) == 0x80000000 * (3 + (2 << 32)) % (1 << 64)


def test_two_streams_give_the_same_words():
    host, on_dev = _state((3 * 4096 + 5, 4095, 1), seed=9)
    torch.cuda.synchronize()
    first = _digest(on_dev, torch.cuda.Stream())
    second = _digest(on_dev, torch.cuda.Stream())
    assert first == second == SD.digest(*host) == _digest(on_dev)


def test_param_digest_checks_its_buffers():
    from facialmmt_amd import ops
    _, on_dev = _state((3,), seed=1)
    raw, blocks = SD.table([(on_dev[0][0].data_ptr(), 0, on_dev[1][0].data_ptr(), on_dev[2][0].data_ptr(), 3)])
    desc = torch.from_numpy(raw).to("cuda:0")
    out = torch.zeros(6, dtype=torch.int64, device="cuda:0")
    assert ops.param_digest(1, blocks, desc, out=out) is out
    for bad in (torch.zeros(5, dtype=torch.int64, device="cuda:0"), torch.zeros(6, dtype=torch.int32, device="cuda:0")):
        with pytest.raises(ValueError):
            ops.param_digest(1, blocks, desc, out=bad)
    with pytest.raises(ValueError):
        ops.param_digest(1, blocks, desc, partial=torch.zeros(5, dtype=torch.int64, device="cuda:0"))


def test_fused_optimizer_digest_after_one_update():
    """FusedClipAdamW over a 3-tensor toy model: one update on fixed gradients, then digest() against the restatement on host copies of p, m and v"""
    from facialmmt_amd.train_step import FusedClipAdamW
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, device=dev)) for s in ((5,), (4097,), (2, 4096))]
    grads = {p: torch.randn(p.shape, generator=g, device=dev) for p in params}
    opt = torch.optim.AdamW(params, lr=torch.tensor(1e-2, device=dev), weight_decay=0.01)
    assert FusedClipAdamW.eligible(opt, params)
    fused = FusedClipAdamW(opt, params, grads, {}, max_norm=1.0)
    zero = SD.as_unsigned(fused.digest().cpu().numpy())
    assert zero[2:] == [0, 0, 0, 0] and zero[:2] == list(SD.sums([p.detach().cpu().numpy() for p in params]))     # moments start at +0.0
    before = [p.detach().clone() for p in params]
    fused.update()
    torch.cuda.synchronize()
    assert all(not torch.equal(a, p) for a, p in zip(before, params))
    got = SD.as_unsigned(fused.digest().cpu().numpy())
    want = SD.digest(*[[t.detach().cpu().numpy() for t in ts] for ts in (params, fused.m, fused.v)])
    print("got", [hex(w) for w in got], "want", [hex(w) for w in want])
    assert got == want and got[:2] != zero[:2] and 0 not in got
    assert SD.as_unsigned(fused.digest().cpu().numpy()) == got                 # the kept scratch is reused: the same words again
