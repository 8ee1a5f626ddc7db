"""tests/support_exact_cases.py on the host, no device: the integer recipe keeps every row exact by arithmetic on its ranges, every route has an
exactly determined output, the fp64 reference equals int64 arithmetic, the operands put most outputs off the bf16 grid and enough of them on
ties, honest fp32 restatements in three summation orders pass the bit test and the a-priori bound, and each deliberately wrong stand-in fails.

What is left to other tests, by count (asserted below): of the 63 Nt rows 4 have no exactly determined output (the two GELU_DG and the two
GELU_BWD rows) and 3 only their pre-activation (EPI_GELU: y is a GELU value); of the 15 Tn rows 1 (x_gelu).  59 + 14 rows and 59 + 28 outputs
are held bit-exact.

Smallest margins by which a stand-in fails (the share of a row's elements whose bits change, the smallest over the small bf16 rows it applies to;
printed by the test):
    truncating store 0.27 (a row whose dropped samples carry no rounding; 0.43 or more elsewhere)      round-half-away store 0.0068
    bf16 before the residual add 0.15      bf16 partial between K splits 0.24      bias after the rounding 0.15
    dropped last 8-element K chunk (|x| <= 15 there, 1/16 of the range) 0.50
On real operands the truncating store puts the mean signed error at -0.49 ulp or below against a limit of 0.02 to 0.05, and the dropped chunk exceeds
the a-priori bound by a factor of 4.0 or more on every small row with K <= 2048 (K = 4096, 4104, 6144: 0.98, 0.92, 0.73 -- inside a worst-case
bound, which is what the integer pass is for)."""
import pytest
import torch

from tests import support_exact_cases as EC
from tests import support_gemm_cases as GC

BF16 = torch.bfloat16
SMALL = [c for c in GC.NT_CASES if c.M <= 70 and EC.nt_exact_outputs(c)]
SMALL_BF16 = [c for c in SMALL if c.dt == "bf16"]


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", GC.NT_CASES, ids=lambda c: c.id)
def test_nt_worst_case_sum_stays_exact(case):
    """recomputed here from the ranges, not from a sample and not from the support module's own arithmetic"""
    r = EC.nt_recipe(case)
    assert r.x <= 255 and r.w <= 7 and r.bias <= 100 and r.res <= 256 and r.aux <= 7 and set(r.scales) <= {0.0, 0.5, 1.0, 2.0}
    worst = r.x * r.w * case.K + r.bias
    if case.epi == GC.EPI_MUL_AUX:
        assert r.aux > 0
        worst *= r.aux
    grid = 1.0
    if case.rps:
        assert 0.0 in r.scales and 0.5 in r.scales
        worst *= max(r.scales)
        grid = 0.5                                                 # half-integers: exact in fp32 below 2^23
    worst += r.res
    assert worst / grid < 1 << 24, (case.id, worst)
    assert worst == r.worst
    # the ladder takes the largest rung that fits
    first = next((x, w) for x, w in EC.X_W_LADDER if EC.nt_worst(case, x, w) < r.limit)
    assert (r.x, r.w) == first


@pytest.mark.parametrize("case", GC.TN_CASES, ids=lambda c: c.id)
def test_tn_worst_case_sum_stays_exact(case):
    r = EC.tn_recipe(case)
    assert r.x <= 7 and r.w <= 15
    assert set(r.scales) == (set() if not case.rps else {0.0, 2.0} if case.two_valued else {-1.0, 0.0, 0.5, 1.0, 2.0})
    smax = max([abs(s) for s in r.scales] or [1.0])
    grid = 0.5 if 0.5 in r.scales else 1.0
    assert case.M * r.x * r.w * smax / grid < 1 << 24, case.id
    assert case.M * r.x * smax / grid < 1 << 24                    # db
    if case.M * 105 < 1 << 24 and grid == 1.0 and smax == 1.0:
        assert (r.x, r.w) == (7, 15)
    if case.M == 262145:
        assert r.x * r.w < 105                                     # the one row that needs a smaller range
    # every scaled operand is on the bf16 grid: the register-staged kernel's rounding of s * dy is the identity here
    for s in r.scales:
        for d in range(-r.x, r.x + 1):
            assert float(torch.tensor(s * d).to(BF16)) == s * d


def test_colsum_worst_case_sum_stays_exact():
    for dt, M, N in GC.COLSUM_CASES:
        assert M * EC.colsum_recipe(dt, M, N).x < 1 << 24
    for C in {c for _, c in EC.MLP_CASES}:
        assert EC.mlp_worst(C) < 1 << 24
    assert EC.patch_worst() < 1 << 24


def test_every_route_has_a_row_with_an_exactly_determined_output():
    routes = GC.route_enum()
    assert len(routes) == 50
    held = {c.route for c in GC.NT_CASES if EC.nt_exact_outputs(c)} | {c.route for c in GC.TN_CASES if EC.tn_exact_outputs(c)}
    assert sorted(set(routes) - held) == []
    # what is left out: GELU-only outputs and the one x_gelu row, nothing else
    nt_none = [c for c in GC.NT_CASES if not EC.nt_exact_outputs(c)]
    assert all(c.epi in (GC.EPI_GELU_DG, GC.EPI_GELU_BWD) for c in nt_none) and len(nt_none) == 4
    pre_only = [c for c in GC.NT_CASES if EC.nt_exact_outputs(c) == ("y_pre",)]
    assert all(c.epi == GC.EPI_GELU for c in pre_only) and len(pre_only) == 3
    assert not [c for c in GC.NT_CASES if c.epi == GC.EPI_GELU and not c.pre]
    tn_none = [c for c in GC.TN_CASES if not EC.tn_exact_outputs(c)]
    assert len(tn_none) == 1 and tn_none[0].x_gelu
    rows = len(GC.NT_CASES) - 4, len(GC.TN_CASES) - 1
    outputs = sum(len(EC.nt_exact_outputs(c)) for c in GC.NT_CASES), sum(len(EC.tn_exact_outputs(c)) for c in GC.TN_CASES)
    assert (len(GC.NT_CASES), len(GC.TN_CASES), rows, outputs) == (63, 15, (59, 14), (59, 28))


# ------------------------------------------------------------------------------------------------ the reference
def _int64_nt(case, v):
    """int64 arithmetic in halves (a row scale of 0.5): 2 * the value in front of the store"""
    i = lambda t: t.double().round().long()
    acc = i(v["x"]) @ i(v["w"]).t()
    if v["bias"] is not None:
        acc = acc + i(v["bias"])
    out = {}
    if case.epi == GC.EPI_GELU:
        out["y_pre"] = 2 * acc
        return out
    if case.epi == GC.EPI_MUL_AUX:
        acc = acc * i(v["aux"])
    acc = acc * (i(2 * v["rs"]).repeat_interleave(case.rps)[:case.M, None] if v["rs"] is not None else 2)
    if v["res"] is not None:
        acc = acc + 2 * i(v["res"])
    out["y"] = acc
    return out


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_reference_is_int64_arithmetic(case):
    v = EC.nt_int_values(case)
    r = EC.nt_recipe(case)
    assert v["x"].abs().max() == r.x and v["w"].abs().max() == r.w       # the ranges are used to their ends
    assert torch.equal(v["x"].double(), v["x"].double().round())
    if v["rs"] is not None:
        assert set(v["rs"].tolist()) <= set(r.scales) and 0.0 in v["rs"].tolist()
    ref, exact = EC.nt_reference(case, v), _int64_nt(case, v)
    assert sorted(ref) == sorted(EC.nt_exact_outputs(case))
    for name in ref:
        assert torch.equal(ref[name] * 2, exact[name].double()), name
        assert ref[name].abs().max().item() <= r.worst
        # the fp32 product torch forms is the same integer (the issue's check), and fp32 holds the epilogue value
        assert torch.equal(ref[name].float().double(), ref[name])
    plain = v["x"].float() @ v["w"].float().t()
    assert torch.equal(plain.double(), v["x"].double() @ v["w"].double().t())


def test_tn_reference_is_int64_arithmetic():
    for case in [c for c in GC.TN_CASES if c.M <= 5000 and EC.tn_exact_outputs(c)]:
        v = EC.tn_int_values(case)
        ref = EC.tn_reference(case, v)
        s2 = (2 * v["rs"]).round().long().repeat_interleave(case.rps)[:case.M, None] if v["rs"] is not None else 2
        sdy = v["dy"].double().round().long() * s2
        assert torch.equal(ref["dw"] * 2, (sdy.t() @ v["x"].double().round().long()).double()), case.id
        assert torch.equal(ref["db"] * 2, sdy.sum(0).double()), case.id
        assert torch.equal(ref["dw"].float().double(), ref["dw"])


def test_single_rounding_from_fp64():
    """rne() rounds once: a value just above a bf16 tie whose fp32 image IS the tie goes up, where torch's fp64 -> fp32 -> bf16 goes to even"""
    tie = 1.0 + 2.0 ** -8                                          # between bf16 1.0 and 1.0078125
    x = torch.tensor([tie, tie + 2.0 ** -40, tie - 2.0 ** -40, -(tie + 2.0 ** -40), 3.0], dtype=torch.float64)
    assert EC.rne(x, BF16).tolist() == [1.0, 1.0078125, 1.0, -1.0078125, 3.0]
    assert x.to(BF16).tolist()[1] == 1.0                           # the double rounding this avoids
    assert EC.ulp(torch.tensor([1.0, 1.5, 2.0, 0.1], dtype=torch.float64), BF16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -11]


def _off_grid_and_ties(ref64):
    f = ref64.float()
    low = f.view(torch.int32) & 0xFFFF
    return float((low != 0).double().mean()), float((low == 0x8000).double().mean())


@pytest.mark.parametrize("case", [c for c in GC.NT_CASES if c.M * c.N <= 1e6 and c.dt == "bf16" and EC.nt_exact_outputs(c)], ids=lambda c: c.id)
def test_most_outputs_are_off_the_bf16_grid_and_enough_are_ties(case):
    ref = EC.nt_reference(case, EC.nt_int_values(case))
    for name, r in ref.items():
        off, ties = _off_grid_and_ties(r)
        print(f"  {case.id} {name}: {off:.3f} not representable in bf16, {ties:.4f} exact ties")
        assert off >= 0.5 and ties >= 0.01, (name, off, ties)


# ------------------------------------------------------------------------------------------------ restatements
def _products(v):
    return v["x"].float()[:, None, :] * v["w"].float()[None, :, :]  # exact in fp32 for bf16 operands


def _sequential(p):
    acc = torch.zeros(p.shape[:2])
    for k in range(p.shape[2]):
        acc = acc + p[:, :, k]
    return acc


def _pairwise(p):
    while p.shape[2] > 1:
        if p.shape[2] % 2:
            p = torch.cat([p, torch.zeros_like(p[:, :, :1])], 2)
        p = p[:, :, 0::2] + p[:, :, 1::2]
    return p[:, :, 0]


def _split4(p, partial=None):
    acc = torch.zeros(p.shape[:2])
    for chunk in p.chunk(4, 2):
        s = _pairwise(chunk)
        acc = acc + (s if partial is None else s.to(partial).float())
    return acc


ORDERS = {"sequential": _sequential, "pairwise": _pairwise, "split4": _split4}


def _to(t, dtype, store):
    if dtype == torch.float32:
        return t
    if store == "rne":
        return t.to(BF16)
    b = t.view(torch.int32)
    if store == "trunc":
        return (b & -65536).view(torch.float32).to(BF16)
    assert store == "half_away"                                    # sign-magnitude: add half an ulp to the magnitude, truncate
    return ((b + 0x8000) & -65536).view(torch.float32).to(BF16)


def _epilogue(case, v, acc, store="rne", wrong=None):
    """fp32, in the order of nt_epilogue (gemm_common.h): bias, [y_pre], aux product, row scale, residual, ONE rounding at the store"""
    dt = torch.float32 if case.dt == "f32" else BF16
    if wrong == "bias_after_rounding" and v["bias"] is not None:
        acc = _to(acc, dt, "rne").float()
    if v["bias"] is not None:
        acc = acc + v["bias"]
    out = {}
    if case.epi == GC.EPI_GELU:
        out["y_pre"] = _to(acc, dt, store)
        return out
    if case.epi == GC.EPI_MUL_AUX:
        acc = acc * v["aux"].float()
    if v["rs"] is not None:
        acc = acc * v["rs"].repeat_interleave(case.rps)[:case.M, None]
    if v["res"] is not None:
        if wrong == "bf16_before_residual":
            acc = _to(acc, dt, "rne").float()
        acc = acc + v["res"].float()
    out["y"] = _to(acc, dt, store)
    return out


def _expected(case, v):
    dt = torch.float32 if case.dt == "f32" else BF16
    return {k: EC.rne(r, dt) for k, r in EC.nt_reference(case, v).items()}


def _failures(got, want):
    n = z = total = 0
    for k in want:
        a, b = EC.bit_mismatch(got[k], want[k])
        n, z, total = n + a, z + b, total + want[k].numel()
    return n - z, total


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_honest_restatements_pass_the_bit_test_and_the_bound(case):
    vi, vr = EC.nt_int_values(case), EC.nt_real_values(case)
    want = _expected(case, vi)
    ref, S = EC.nt_reference(case, vr), EC.nt_reference(case, vr, absolute=True)
    pi, pr = _products(vi), _products(vr)
    for name, order in ORDERS.items():
        bad, total = _failures(_epilogue(case, vi, order(pi)), want)
        assert bad == 0, (name, bad, total)
        got = _epilogue(case, vr, order(pr))
        for k in ref:
            ratio = EC.worst_ratio((got[k].double() - ref[k]).abs(), EC.nt_bound(case, k, ref[k], S[k]))
            print(f"  {case.id} {k} [{name}] worst err / bound {ratio:.3f}")
            assert ratio <= 1.0, (name, k, ratio)
            if case.dt == "bf16":
                share, bias = EC.rounding_stats(got[k], ref[k])
                assert abs(bias) <= EC.bias_limit(0.0, got[k].numel()), (name, k, share, bias)


def _small_chunk_values(case):
    """integer operands whose last 8-element K chunk is at most 1/16 of the row's range (|x| <= 15 of 255)"""
    v = dict(EC.nt_int_values(case))
    g = torch.Generator().manual_seed(EC.seed_of("tail " + case.id))
    x = v["x"].clone()
    tail = torch.randint(-15, 16, (case.M, 8), generator=g)
    tail[tail == 0] = 15
    x[:, -8:] = tail.to(x.dtype)
    v["x"] = x
    return v


def _wrong(name, case, v):
    p = _products(v)
    if name == "truncating store":
        return _epilogue(case, v, _split4(p), store="trunc")
    if name == "round-half-away store":
        return _epilogue(case, v, _split4(p), store="half_away")
    if name == "bf16 before the residual add":
        return _epilogue(case, v, _split4(p), wrong="bf16_before_residual")
    if name == "bf16 partial between K splits":
        return _epilogue(case, v, _split4(p, partial=BF16))
    if name == "dropped last K chunk":
        return _epilogue(case, v, _split4(p[:, :, :-8]))
    assert name == "bias after the rounding"
    return _epilogue(case, v, _split4(p), wrong="bias_after_rounding")


STAND_INS = {
    "truncating store": lambda c: True,
    "round-half-away store": lambda c: True,
    "bf16 before the residual add": lambda c: c.res,
    "bf16 partial between K splits": lambda c: True,
    "dropped last K chunk": lambda c: True,
    "bias after the rounding": lambda c: c.bias,
}


@pytest.mark.parametrize("name", list(STAND_INS), ids=lambda n: n.replace(" ", "_"))
def test_wrong_stand_ins_fail_the_bit_test(name):
    """every applicable small bf16 row: the stand-in changes bits of an exactly determined output.  The smallest share is the margin (docstring)"""
    rows = [c for c in SMALL_BF16 if STAND_INS[name](c)]
    assert len(rows) >= 2, name
    margin = 1.0
    for case in rows:
        v = _small_chunk_values(case) if name == "dropped last K chunk" else EC.nt_int_values(case)
        bad, total = _failures(_wrong(name, case, v), _expected(case, v))
        print(f"  {name}: {case.id}: {bad} of {total} elements differ ({bad / total:.4f})")
        margin = min(margin, bad / total)
        assert bad > 0, (name, case.id)
    print(f"  {name}: smallest share of changed elements {margin:.4f}")
    # the check a kernel is held to is bad == 0; a stand-in that changed only a handful of elements would pass a noisy kernel by luck
    assert margin >= 0.005, (name, margin)


@pytest.mark.parametrize("case", SMALL_BF16, ids=lambda c: c.id)
def test_wrong_stand_ins_fail_the_real_pass(case):
    """what the integer pass cannot see alone is seen twice: on real operands a truncating store misses the signed-error limit, a dropped K chunk
    whose operands are 1/16 of the rest misses the a-priori bound"""
    v = EC.nt_real_values(case)
    ref, S = EC.nt_reference(case, v), EC.nt_reference(case, v, absolute=True)
    got = _wrong("truncating store", case, v)
    for k in ref:
        share, bias = EC.rounding_stats(got[k], ref[k])
        live = float((v["rs"] != 0).float().mean()) if k == "y" and v["rs"] is not None else 1.0      # rows of dropped samples carry no rounding
        print(f"  {case.id} {k}: truncating store: mismatch share {share:.3f}, mean signed error {bias:.3f} ulp (limit {EC.bias_limit(0.0, ref[k].numel()):.4f})")
        assert abs(bias) > EC.bias_limit(0.0, ref[k].numel()) and bias < -0.3 * live
        assert share > EC.share_limit(0.0, ref[k].numel())
    v2 = dict(v)
    x = v["x"].clone()
    x[:, -8:] = (x[:, -8:].float() / 16).to(x.dtype)
    v2["x"] = x
    ref, S = EC.nt_reference(case, v2), EC.nt_reference(case, v2, absolute=True)
    got = _wrong("dropped last K chunk", case, v2)
    for k in ref:
        ratio = EC.worst_ratio((got[k].double() - ref[k]).abs(), EC.nt_bound(case, k, ref[k], S[k]))
        print(f"  {case.id} {k}: dropped chunk: worst err / bound {ratio:.2f}")
        # a worst-case bound grows with K: past K = 2048 eight operands of 1/16 the size fit inside it, and only the integer pass sees them
        assert ratio > 1.0 or case.K > 2048, (k, ratio)


def test_tn_restatement_and_documented_rounding():
    """the weight gradient: fp32 accumulation passes the bit test on integers in two orders; on real operands the register-staged rounding of s * dy
    (EXTRA_ROUNDINGS) stays inside the bound that charges it and misses the one that does not"""
    case = next(c for c in GC.TN_CASES if c.route == "TN_REG32_FEW" and c.M == 100)
    v = EC.tn_int_values(case)
    ref = EC.tn_reference(case, v)
    dy, x = v["dy"].float(), v["x"].float()
    seq = torch.zeros(case.N, case.K)
    for m in range(case.M):
        seq = seq + dy[m, :, None] * x[m, None, :]
    assert torch.equal(seq.double(), ref["dw"]) and torch.equal((dy.t() @ x).double(), ref["dw"]) and torch.equal(dy.sum(0).double(), ref["db"])
    scaled = next(c for c in GC.TN_CASES if c.route == "TN_REG64" and c.rps and not c.x_gelu)
    small = GC.Tn(scaled.route, "bf16", 512, 96, 96, rps=64, two_valued=False)
    assert EC.tn_extra(small) == 2.0 ** -8 and EC.tn_extra(GC.Tn("TN_DMA_256_SCALED", "bf16", 8256, 1024, 1024, rps=64)) == 0.0
    v = EC.tn_real_values(small)
    ref, S = EC.tn_reference(small, v), EC.tn_reference(small, v, absolute=True)
    sdy = (v["dy"].float() * v["rs"].repeat_interleave(64)[:, None]).to(BF16).float()
    got = sdy.t() @ v["x"].float()
    err = (got.double() - ref["dw"]).abs()
    assert (err / EC.tn_bound(small, "dw", ref["dw"], S["dw"])).max().item() <= 1.0
    assert (err / EC.bound(ref["dw"], S["dw"], small.M + 1, 0.0)).max().item() > 1.0
