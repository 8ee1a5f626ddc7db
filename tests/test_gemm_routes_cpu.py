"""The GEMM route query (include/fmmt_route.h: the dispatch itself with the launch replaced by the kernel's name) on the host, no device:
the header, _lib.ROUTE_SIGNATURES and the library agree; every row of the strided case table lands on the kernel family it names, in every layout;
every kernel family is reached by a row whose leading dimensions differ from the row widths; the 32-bit-offset guards and the leading-dimension
contract (include/fmmt.h, DESIGN.md "Leading dimensions of the GEMMs") answer the same through the query and through the real entry points."""
import os
import re

import pytest

from facialmmt_amd import _lib
from tests import support_gemm_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = GC.route_enum()
NAMES = {v: k for k, v in ROUTES.items()}
BF16, F32 = _lib.BF16, _lib.F32
EINVAL = _lib.FMMT_EINVAL
PTR = 4096              # a present, 16-byte aligned operand for calls that must be refused before any launch (never dereferenced on the host)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from facialmmt_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_route_header_signatures_and_library_agree(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmmt_route.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.ROUTE_SIGNATURES)
    for name, args in protos.items():
        res, argtypes = _lib.ROUTE_SIGNATURES[name]
        params = [a.strip() for a in args.split(",")]
        assert all(re.fullmatch(r"int \w+", a) for a in params), (name, params)       # every argument a plain int: presence flags, no pointers
        assert len(params) == len(argtypes) and all(t is _lib._i for t in argtypes) and res is _lib._i, name
        assert hasattr(lib, name)
    assert '#include "fmmt_route.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    # the enum: 1 .. COUNT - 1 without gaps; the mode constants as Python states them
    assert sorted(ROUTES.values()) == list(range(1, len(ROUTES) + 1))
    assert int(re.search(r"FMMT_ROUTE_COUNT = (\d+)", src).group(1)) == len(ROUTES) + 1
    modes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define FMMT_ROUTE_MODE_(\w+) (\d+)", src)}
    assert modes == {"FWD": _lib.ROUTE_MODE_FWD, "SEG3_N": _lib.ROUTE_MODE_SEG3_N, "SEG3_K": _lib.ROUTE_MODE_SEG3_K, "SPLITK": _lib.ROUTE_MODE_SPLITK}


@pytest.mark.parametrize("case", GC.NT_CASES + GC.TN_CASES, ids=lambda c: c.id)
def test_case_lands_on_the_route_it_names(lib, case):
    assert case.route in ROUTES, case.route
    for layout in ("contig",) + tuple(case.layouts):
        got = GC.query_route(lib, case, layout)
        assert NAMES.get(got, got) == case.route, (case.id, layout)


def test_case_ids_are_unique():
    ids = [c.id for c in GC.NT_CASES + GC.TN_CASES]
    assert len(ids) == len(set(ids))


def test_every_route_is_reached_with_a_leading_dimension_that_is_not_the_width(lib):
    reached = set()
    for case in GC.NT_CASES + GC.TN_CASES:
        for layout in case.layouts:
            ld = GC.lds(case, layout)
            widths = {"x": case.K, "dy": case.N, "y": case.N}
            if any(ld[k][0] != widths[k] for k in ld if k in widths):
                reached.add(GC.query_route(lib, case, layout))
    # the exclusion list may only hold routes that the contract makes unreachable with ld != width; none are
    assert GC.UNREACHABLE_WITH_LD == ()
    missing = sorted(set(ROUTES) - {NAMES[r] for r in reached if r in NAMES} - set(GC.UNREACHABLE_WITH_LD))
    assert missing == [], missing


def _fwd(lib, dt, M, N, K, *, ldx=None, ldw=None, ldy=None, bias=1, pre=0, epi=0, aux=0, ldaux=None, res=0, ldres=None, rs=0, rps=1, mode=0):
    ldy = N if ldy is None else ldy
    return lib.fmmt_linear_fwd_route(dt, M, N, K, K if ldx is None else ldx, K if ldw is None else ldw, ldy, bias, pre, epi, aux, ldy if ldaux is None else ldaux,
                                     res, ldy if ldres is None else ldres, rs, rps, mode)


def test_an_ld_past_the_32_bit_offsets_moves_a_launch_to_64_bit_addressing(lib):
    """ph_plan / p256_plan: M * ld >= 2^31 elements (byte offsets >= 2^32) leaves the kernels that form per-lane unsigned 32-bit byte offsets; the
    128-row kernels address with 64-bit products.  One element below the bound stays."""
    wide64 = {ROUTES["NT128_DMA"], ROUTES["NT128_BK32"], ROUTES["NT128_BK64"]}
    for (M, N, K, kw, route) in [(8192, 2048, 192, {}, "PH"), (8192, 1024, 192, {}, "PH3_PLAIN"), (8192, 1024, 192, {"res": 1}, "PH3_OP"),
                                 (56072, 384, 192, {}, "PH3W_PLAIN"), (16384, 1024, 128, {}, "P256_256"), (16384, 768, 128, {"res": 1}, "P256_192_OP")]:
        assert NAMES[_fwd(lib, BF16, M, N, K, **kw)] == route
        big = ((1 << 31) + M - 1) // M
        big = (big + 7) // 8 * 8                                  # the smallest ld % 8 == 0 with M * ld >= 2^31
        assert M * big >= 1 << 31 and M * (big - 8) < 1 << 31
        assert _fwd(lib, BF16, M, N, K, ldx=big, **kw) in wide64, (route, "ldx")
        assert NAMES[_fwd(lib, BF16, M, N, K, ldx=big - 8, **kw)] == route, (route, "ldx below the bound")
        if route.startswith("PH"):                                # the phase kernels also store through 32-bit offsets
            assert NAMES[_fwd(lib, BF16, M, N, K, ldy=big, **kw)] not in ("PH", "PH3_PLAIN", "PH3_OP", "PH3W_PLAIN"), (route, "ldy")
    # the weight operand: N * ldw
    assert _fwd(lib, BF16, 16384, 1024, 128, ldw=1 << 21) in wide64


# (dtype, M, N, K, keyword arguments of _fwd): what the leading-dimension contract refuses
FWD_REFUSED = [
    (BF16, 70, 100, 96, {}),                                      # bf16 N = 4 (mod 8), contiguous
    (BF16, 70, 100, 96, {"ldy": 104}),                            # ... and with an aligned pitch: a straddling 8-channel chunk would be dropped
    (BF16, 70, 96, 96, {"ldy": 100}),                             # bf16 ldy = 4 (mod 8): odd rows only 8-byte aligned
    (BF16, 16384, 1024, 128, {"ldy": 1028}),                      # ... on the persistent kernel's shape
    (BF16, 65544, 128, 576, {"ldy": 132}),                        # ... on the deep kernel's shape
    (BF16, 70, 96, 96, {"res": 1, "ldres": 100}),
    (BF16, 70, 96, 96, {"epi": 4, "aux": 1, "ldaux": 100}),
    (BF16, 70, 96, 96, {"epi": 2, "aux": 1, "ldaux": 100}),
    (BF16, 70, 96, 96, {"epi": 2, "aux": 0}),                     # GELU' without its operand
    (BF16, 70, 96, 96, {"ldx": 100}), (BF16, 70, 96, 96, {"ldw": 100}),
    (BF16, 70, 96, 96, {"ldx": 88}), (BF16, 70, 96, 96, {"ldw": 88}), (BF16, 70, 96, 96, {"ldy": 88}),      # a pitch shorter than the row
    (BF16, 70, 96, 96, {"res": 1, "ldres": 88}),
    (F32, 70, 96, 96, {"ldy": 98}), (F32, 70, 96, 96, {"res": 1, "ldres": 98}), (F32, 70, 98, 96, {}),
    (BF16, 70, 96, 96, {"rs": 1, "rps": 0}),
]


@pytest.mark.parametrize("case", FWD_REFUSED, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{'-'.join(f'{k}{v}' for k, v in c[4].items())}")
def test_fwd_refusals_agree_between_query_and_entry_point(lib, case):
    dt, M, N, K, kw = case
    assert _fwd(lib, dt, M, N, K, **kw) == EINVAL
    ldy = kw.get("ldy", N)
    rc = lib.fmmt_linear_fwd(dt, M, N, K, PTR, kw.get("ldx", K), PTR, kw.get("ldw", K), None, PTR, ldy, None, kw.get("epi", 0),
                             PTR if kw.get("aux") else None, kw.get("ldaux", ldy), PTR if kw.get("res") else None, kw.get("ldres", ldy),
                             PTR if kw.get("rs") else None, kw.get("rps", 1), None)
    assert rc == EINVAL


def test_fwd_accepts_what_the_contract_allows(lib):
    assert NAMES[_fwd(lib, BF16, 70, 96, 96, ldx=104, ldw=104, ldy=104, res=1, ldres=112)] == "NT64_K96"
    assert NAMES[_fwd(lib, F32, 70, 96, 96, ldx=100, ldw=100, ldy=100, res=1, ldres=100)] == "NT64_F32"
    assert NAMES[_fwd(lib, BF16, 70, 96, 96, ldaux=100, ldres=100)] == "NT64_K96"      # the ld of an absent operand is not looked at


def test_seg3_and_splitk_refusals_agree_between_query_and_entry_point(lib):
    # seg3: ldy = 4 (mod 8), a pitch shorter than the row
    for (M, N, K, mode, ldx, ldw, ldy) in [(70, 192, 128, 1, 128, 128, 196), (70, 192, 128, 1, 128, 128, 184), (70, 64, 192, 2, 192, 64, 68), (70, 64, 192, 2, 184, 64, 64),
                                           (70, 64, 192, 2, 192, 56, 64)]:
        assert lib.fmmt_linear_fwd_route(BF16, M, N, K, ldx, ldw, ldy, 0, 0, 0, 0, ldy, 0, ldy, 0, 1, mode) == EINVAL
        assert lib.fmmt_linear_fwd_seg3(BF16, M, N, K, PTR, ldx, PTR, PTR, PTR, ldw, mode, None, None, None, PTR, ldy, None) == EINVAL
    assert NAMES[lib.fmmt_linear_fwd_route(BF16, 70, 192, 128, 136, 136, 200, 1, 0, 0, 0, 200, 0, 200, 0, 1, 1)] == "NT_SEG3"
    # split-K: its finish kernel writes y at m * ldy + n -- ldy was never looked at
    M, N, K = 8, 128, 4096
    ws = lib.fmmt_linear_splitk_workspace(M, N, K)
    assert ws > 0
    for dt, ldy in ((BF16, 120), (BF16, 132), (F32, 120), (F32, 130), (BF16, 0), (BF16, -128)):
        assert _fwd(lib, dt, M, N, K, ldy=ldy, mode=3) == EINVAL
        assert lib.fmmt_linear_fwd_splitk(dt, M, N, K, PTR, K, PTR, K, None, PTR, ldy, PTR, ws, None) == EINVAL
    assert lib.fmmt_linear_fwd_splitk(BF16, M, N, K, PTR, K, PTR, K, None, None, N, PTR, ws, None) == EINVAL      # no output
    # bf16 N = 4 (mod 8), with an aligned pitch too: the same rule as fmmt_linear_fwd (fp32: N % 4)
    ws100 = lib.fmmt_linear_splitk_workspace(M, 100, K)
    assert ws100 > 0
    for dt, n, ldy in ((BF16, 100, 100), (BF16, 100, 104), (F32, 98, 100)):
        assert _fwd(lib, dt, M, n, K, ldy=ldy, mode=3) == EINVAL
        assert lib.fmmt_linear_fwd_splitk(dt, M, n, K, PTR, K, PTR, K, None, PTR, ldy, PTR, ws100, None) == EINVAL
    assert NAMES[_fwd(lib, F32, M, 100, K, ldy=104, mode=3)] == "NT64_F32"
    assert lib.fmmt_linear_fwd_splitk(BF16, M, N, K, PTR, K - 8, PTR, K, None, PTR, N, PTR, ws, None) == EINVAL
    assert NAMES[_fwd(lib, BF16, M, N, K, ldy=136, mode=3)] == "NT64_BK64"
    assert _fwd(lib, BF16, 70, 96, 96, mode=3) == EINVAL            # not a split-K shape
    assert _fwd(lib, BF16, 70, 96, 96, mode=4) == EINVAL


def test_large_offset_rows_put_many_rows_of_x_past_two_to_the_31_bytes():
    """a 'bigx' row is there for byte offsets of x in [2^31, 2^32): the kernels clamp rows to M - 1, so it is row (M - 1) * ldx that counts, not M * ldx.
    At least a quarter of the rows start at or above 2^31 bytes, and M * ldx stays below 2^31 elements (the guard of ph_plan / p256_plan: the row keeps its route)."""
    big = [c for c in GC.NT_CASES if "bigx" in c.layouts]
    assert {c.route for c in big} == {"P256_256", "PH3_PLAIN"}
    for c in big:
        first_past = -(-(1 << 31) // (2 * c.ldx))                  # the first row whose byte offset reaches 2^31 (bf16: 2 bytes)
        assert c.dt == "bf16" and c.M - first_past >= c.M // 4, (c.id, first_past)
        assert (c.M - 1) * c.ldx * 2 + 2 * c.K <= 1 << 32 and c.M * c.ldx < 1 << 31, c.id


def test_wgrad_refusals_agree_between_query_and_entry_point(lib):
    for (dt, M, N, K, lddy, ldx) in [(BF16, 500, 96, 96, 100, 96), (BF16, 500, 96, 96, 96, 100), (BF16, 500, 96, 96, 88, 96), (BF16, 500, 96, 96, 96, 88),
                                     (BF16, 9000, 1024, 1024, 1016, 1024), (F32, 500, 96, 96, 98, 96), (BF16, 500, 100, 96, 104, 96)]:
        for mode in (0, 1):
            assert lib.fmmt_linear_wgrad_route(dt, M, N, K, lddy, ldx, 0, 1, 0, mode) == EINVAL
        nbytes = lib.fmmt_linear_wgrad_workspace(dt, M, N, K)
        assert lib.fmmt_linear_wgrad(dt, M, N, K, PTR, lddy, PTR, ldx, PTR, PTR, None, 1, 0, PTR, nbytes, None) == EINVAL
        assert lib.fmmt_linear_wgrad_partials(dt, M, N, K, PTR, lddy, PTR, ldx, 1, None, 1, 0, PTR, nbytes, None) == EINVAL
    assert lib.fmmt_linear_wgrad_route(BF16, 500, 96, 96, 96, 96, 1, 0, 0, 0) == EINVAL           # a scale without rows_per_scale
    assert lib.fmmt_linear_wgrad_route(BF16, 500, 96, 96, 96, 96, 0, 1, 2, 0) == EINVAL           # x_epi other than GELU
    assert lib.fmmt_linear_wgrad_route(BF16, 500, 96, 96, 96, 96, 0, 1, 0, 2) == EINVAL
    # a leading dimension that is 16-byte but not 8-element... does not exist in bf16; fp32 rows of 4: the few-token and DMA kernels are bf16-only
    assert NAMES[lib.fmmt_linear_wgrad_route(F32, 500, 96, 96, 100, 100, 0, 1, 0, 0)] == "TN_F32"
