"""The case table of the kernel-bounds test (tests/support_bounds_cases.py) and the support it runs on (tests/support_bounds.py), without a GPU.

The table: unique ids, every family in the classes of M it must show against the unit each row states, a zero in every rowscale the GPU test builds,
five pairwise distinct 16-byte aligned pitches per attention row, guard rows beyond the largest over-read.  The support: torch stand-ins that address
flat buffers the way a kernel does (base offset + row * pitch + column) -- the right one passes, and each deliberately wrong one is flagged."""
import pytest
import torch

from tests import support_bounds as SB
from tests import support_bounds_cases as BC
from tests import support_strided as SS


# ------------------------------------------------------------------------------------------------ the table
def test_ids_are_unique_and_every_row_is_complete():
    ids = [c.id for c in BC.CASES]
    assert len(ids) == len(set(ids))
    for c in BC.CASES:
        assert c.family in BC.FAMILIES and c.entry.startswith("fmmt_") and c.dt in ("bf16", "f32"), c.id
        assert c.unit >= 1 and c.unit_name and c.M >= 1, c.id


def test_every_family_has_its_classes_of_m():
    for fam, need in BC.FAMILIES.items():
        rows = [c for c in BC.CASES if c.family == fam]
        assert rows, fam
        have = {BC.m_class(c.M, c.unit) for c in rows}
        assert need <= have, (fam, need - have)
    # ... and, entry point by entry point, wherever the family promises all three (an entry point whose unit is one row or one window has no "below")
    for fam, need in BC.FAMILIES.items():
        if len(need) < 3:
            continue
        for entry in sorted({c.entry for c in BC.CASES if c.family == fam}):
            rows = BC.of(entry)
            if entry.endswith("_ragged") or all(c.unit == 1 for c in rows):
                continue
            have = {BC.m_class(c.M, c.unit) for c in rows if c.unit > 1}
            assert need <= have, (entry, need - have)


def test_the_guard_free_instantiations_are_reached():
    """M % 256 == 0 selects FULL in the fused Mlp forward, and a whole number of tiles everywhere else"""
    for entry in ("fmmt_mlp_fwd", "fmmt_mlp_ln_fwd", "fmmt_mlp_bwd_input", "fmmt_mlp_ln_bwd_input", "fmmt_linear_ln_bwd"):
        assert any(c.M % 256 == 0 for c in BC.of(entry)) and any(c.M % 256 for c in BC.of(entry)), entry
    assert {c.M for c in BC.of("fmmt_mlp_bwd_input") if c.shape["C"] == 192} == {40, 168, 296, 256}


def test_rowscale_vectors_contain_a_zero():
    """the rule the GPU test builds every rowscale by (support_bounds.rowscale_values): entry 0 is a dropped sample whenever there is more than one entry,
    the only entry otherwise -- and a case with a rowscale has rows for it"""
    for c in BC.CASES:
        if not c.opts.get("rowscale"):
            continue
        n = BC.rowscale_len(c)
        assert n >= 1, c.id
        v = SB.rowscale_values(n, torch.Generator().manual_seed(0), "cpu")
        assert v.numel() == n and (v == 0).sum().item() >= 1 and (n == 1 or (v != 0).any()), c.id


def test_mha_pitches_are_distinct_and_aligned():
    rows = [c for c in BC.CASES if c.family == "mha"]
    assert any(c.opts.get("separate") for c in rows) and any(c.entry.endswith("_ragged") for c in rows)
    for c in rows:
        s = c.shape
        lds = [s[k] for k in ("ldq", "ldkv", "ldo", "lddq", "lddkv")]
        assert len(set(lds)) == 5 and all(ld % 8 == 0 for ld in lds), c.id
        E = s["E"]
        kvw = E if c.opts.get("separate") else 2 * E
        assert s["ldq"] > E and s["ldo"] > E and s["lddq"] > E and s["ldkv"] > kvw and s["lddkv"] > kvw, c.id
    r = [c for c in rows if c.entry.endswith("_ragged")][0].shape
    assert sum(r["lens"]) < r["rows"] <= r["B"] * r["T"] and max(r["lens"]) == r["T"]


def test_guard_rows_exceed_the_largest_overread():
    assert BC.GUARD_ROWS == SS.GUARD == SB.GUARD
    worst = BC.largest_overread_rows()
    assert worst >= 256 and SS.GUARD > worst, worst
    # the 1-D operands get GUARD elements; a vector indexed by row (mean, rstd, rowscale, lse) is over-read by at most a unit of rows, lse by a unit of
    # windows x heads x 49 values -- the largest: 4 windows of 24 heads
    assert SB.GUARD * 4 % 16 == 0 and SB.GUARD > 256


# ------------------------------------------------------------------------------------------------ the support, on stand-ins
M, C = 37, 24


def _colsum_operands(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    xv = torch.randn(M, C, generator=g).to(dtype)
    x = SS.make(M, C, dtype, "cpu", values=xv)
    out = SB.make1d(C, torch.float32, "cpu", output=True)
    return x, out, xv


def _colsum(x, out, rows=M, stray=None):
    """out[c] = sum_{m < rows} x[m * ld + c] on the flat buffers"""
    xf, of = x.flat(), out.flat()
    idx = x.offset + torch.arange(rows)[:, None] * x.ld + torch.arange(C)[None, :]
    of[out.offset + torch.arange(C)] = xf[idx].double().sum(0).float()
    if stray is not None:
        of[out.offset + stray] = 0.5


def test_right_column_sum_passes_and_the_vector_is_built_as_promised():
    x, out, xv = _colsum_operands()
    snap = SB.snapshot({"x": x})
    _colsum(x, out)
    assert out.problems() == [] and SB.changed({"x": x}, snap) == []
    assert torch.equal(out.vec, xv.double().sum(0).float())
    v = SB.make1d(5, torch.float32, "cpu", values=torch.arange(5.0))
    assert v.ptr % 16 == 0 and v.buf.shape == (1, 5 + 2 * SB.GUARD) and torch.equal(v.vec, torch.arange(5.0))
    outside = torch.ones_like(v.buf, dtype=torch.bool)
    outside[0, SB.GUARD:SB.GUARD + 5] = False
    assert not torch.isfinite(v.buf[outside]).any()
    assert torch.isinf(v.buf[0, SB.GUARD - 1]) and torch.isinf(v.buf[0, SB.GUARD + 5])


def test_column_sum_over_one_row_too_many_is_flagged():
    x, out, _ = _colsum_operands()
    _colsum(x, out, rows=M + 1)                                    # the row behind M: 0 x zero-filled memory would have hidden it
    p = out.problems()
    assert len(p) == 1 and "not finite" in p[0], p


@pytest.mark.parametrize("where", [C, -1])
def test_one_element_behind_or_in_front_of_a_vector_is_flagged(where):
    x, out, _ = _colsum_operands()
    _colsum(x, out, stray=where)
    p = out.problems()
    assert len(p) == 1 and p[0].startswith("stray write: 1 element"), p


def _partials(ws, nblocks, nbytes_used):
    """a kernel's per-workgroup partial sums: fp32 words from the workspace base on"""
    ws.flat()[ws.offset:ws.offset + nbytes_used] = 7
    return nblocks


def test_workspace_is_nan_filled_aligned_and_its_tail_is_watched():
    ws = SB.Workspace(1000, "cpu")
    assert ws.ptr % 256 == 0 and (ws.buf[ws.pad:ws.pad + 1000] == 0xFF).all() and ws.buf.numel() == 1000 + 2 * SB.WS_PAD
    assert torch.isnan(ws.buf[ws.pad:ws.pad + 1000].view(torch.float32)).all()
    _partials(ws, 4, 1000)
    assert ws.problems() == []
    _partials(ws, 4, 1001)                                         # one byte behind
    p = ws.problems()
    assert len(p) == 1 and "1 byte(s) changed behind" in p[0], p
    ws2 = SB.Workspace(64, "cpu")
    ws2.flat()[ws2.offset - 1] = 0
    assert len(ws2.problems()) == 1 and "in front of" in ws2.problems()[0]


def test_a_modified_input_is_flagged_even_where_the_value_compares_equal():
    x, out, _ = _colsum_operands()
    idx = torch.tensor([0, 1, 2], dtype=torch.int32)
    ins = {"x": x, "index": idx, "absent": None}
    snap = SB.snapshot(ins)
    _colsum(x, out)
    assert SB.changed(ins, snap) == []
    x.view[3, 4] = -x.view[3, 4]                                   # the region
    assert SB.changed(ins, snap) == ["input x: 1 element(s) modified by the call"]
    snap = SB.snapshot(ins)
    x.buf[0, 0] = 1.0                                              # a guard row (NaN before: NaN != NaN as floats, the integer view sees the change once)
    idx[1] = 5
    assert sorted(SB.changed(ins, snap)) == ["input index: 1 element(s) modified by the call", "input x: 1 element(s) modified by the call"]
    z = SS.make(2, 8, torch.float32, "cpu", values=torch.zeros(2, 8))
    snap = SB.snapshot({"z": z})
    z.view[0, 0] = -0.0                                            # -0.0 == 0.0 as floats
    assert len(SB.changed({"z": z}, snap)) == 1


# ---- the attention core's five pitches
LQ, E = 9, 16


def _mha_like(use_ldq_for_dq):
    """a stand-in with the ABI's shape: reads q at ldq, writes out at ldo and dq at lddq -- or, wrongly, at ldq"""
    p = BC.mha_pitches(E)
    g = torch.Generator().manual_seed(9)
    qv = torch.randn(LQ, E, generator=g)
    q = SS.make(LQ, E, torch.float32, "cpu", ld=p["ldq"], values=qv)
    out = SS.make(LQ, E, torch.float32, "cpu", ld=p["ldo"], output=True)
    dq = SS.make(LQ, E, torch.float32, "cpu", ld=p["lddq"], output=True)
    m, n = torch.arange(LQ)[:, None], torch.arange(E)[None, :]
    val = q.flat()[q.offset + m * p["ldq"] + n]
    out.flat()[out.offset + m * p["ldo"] + n] = 2.0 * val
    dq.flat()[dq.offset + m * (p["ldq"] if use_ldq_for_dq else p["lddq"]) + n] = 3.0 * val
    return qv, out, dq


def test_attention_stand_in_with_the_right_pitches_passes():
    qv, out, dq = _mha_like(False)
    assert out.problems() == [] and dq.problems() == []
    assert torch.equal(out.view, 2.0 * qv) and torch.equal(dq.view, 3.0 * qv)


def test_attention_stand_in_that_uses_ldq_for_dq_is_flagged():
    _, out, dq = _mha_like(True)
    assert out.problems() == []
    p = dq.problems()
    assert any("stray write" in s for s in p) and any("not finite" in s for s in p), p


# ---- the bookkeeping of one call
@pytest.mark.parametrize("guarded", [False, True])
def test_arena_hands_out_the_same_operands_plain_and_guarded(guarded):
    A = SB.Arena("cpu", guarded)
    xv = torch.arange(12.0).reshape(3, 4)
    xp, ldx = A.mat_in("x", xv, ld=8)
    gp = A.vec_in("g", torch.ones(4))
    ip = A.vec_in("index", torch.arange(4, dtype=torch.int32))
    assert A.mat_in("absent", None) == (None, 0) and A.vec_in("absent", None) is None
    yp, ldy = A.mat_out("y", 3, 4, torch.float32, ld=12, col=4)
    dp = A.vec_out("d", 4)
    assert A.mat_out("none", 3, 4, torch.float32, present=False) == (None, 0) and A.vec_out("none", 4, present=False) is None
    wp, wn = A.workspace(100)
    assert (ldx, ldy) == ((8, 12) if guarded else (4, 4)) and wn == 100 and all(p % 16 == 0 for p in (xp, gp, yp, dp, wp)) and ip
    assert torch.isnan(A.result("y")).all() and A.result("y").shape == (3, 4) and A.result("d").shape == (4,)

    def kernel():
        A.result("y").copy_(xv * 2)
        A.result("d").fill_(1.0)
        return 0
    assert A.launch(kernel) == 0
    assert A.problems() == []
    assert torch.equal(A.result("y"), xv * 2)
    A.result("d")[2] = float("nan")
    assert len(A.problems()) == 1 and A.problems(unwritten_ok=("d",)) == []
    short = SB.Arena("cpu", guarded, short=True)
    assert short.workspace(100)[1] == 99
