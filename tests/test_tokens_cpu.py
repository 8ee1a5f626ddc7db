"""CPU tests of the text encoder's token packing: include/fmmt_tokens.h == _lib.TOKENS_SIGNATURES == the built library (names, argument types, argument
validation before any launch), and the host-side decisions of the training steps (train_step.count_tokens / default_token_capacity / token_fit)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fmmt_dropadd_ln_bwd_map", "fmmt_dropadd_ln_fwd_map", "fmmt_mha_bwd_ragged", "fmmt_mha_fwd_ragged", "fmmt_token_layout", "fmmt_unpack_rows"]


def test_tokens_header_signatures_and_library_agree():
    from facialmmt_amd import _lib, build
    assert '#include "fmmt_tokens.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmmt_tokens.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.TOKENS_SIGNATURES) == NAMES
    others = [getattr(_lib, k) for k in dir(_lib) if k.endswith("SIGNATURES") and k != "TOKENS_SIGNATURES"]
    assert not any(set(_lib.TOKENS_SIGNATURES) & set(t) for t in others)
    assert int(re.search(r"#define FMMT_RAGGED (0x[0-9a-fA-F]+)", src).group(1), 16) == _lib.RAGGED
    assert _lib.RAGGED & (_lib.BATCH_MAJOR | _lib.GENERIC | _lib.SAVE_DG | _lib.BF16) == 0

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    for name, args in protos.items():
        want = [ctype_of(a) for a in args.split(",") if a.strip()]
        res, got = _lib.TOKENS_SIGNATURES[name]
        assert got == want and res is C.c_int, (name, len(got), len(want))
    # the mapped tails are the plain ones with the row map added in front of the stream
    for mapped, plain in (("fmmt_dropadd_ln_fwd_map", "fmmt_dropadd_ln_fwd"), ("fmmt_dropadd_ln_bwd_map", "fmmt_dropadd_ln_bwd")):
        a = list(_lib.TOKENS_SIGNATURES[mapped][1])
        assert a.pop(-2) is C.c_void_p and a == _lib.SIGNATURES[plain][1], mapped
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in protos)
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in protos)
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    p += -p % 16
    # every refusal below happens before a launch
    for bad in ((0, 5, 8), (257, 5, 8), (3, 0, 8), (3, 65536, 8), (3, 5, 0), (3, 5, 65536)):
        assert lib.fmmt_token_layout(*bad, p, p, p, p, p, p, None) == _lib.FMMT_EINVAL, bad
    assert lib.fmmt_token_layout(3, 5, 8, None, p, p, p, p, p, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_unpack_rows(3, 5, 8, 40, p, p, p, None) == _lib.FMMT_EALIGN
    assert lib.fmmt_unpack_rows(3, 5, 8, 48, p, p, p + 8, None) == _lib.FMMT_EALIGN
    for bad in ((0, 5, 8, 48), (257, 5, 8, 48), (3, 0, 8, 48), (3, 5, 0, 48), (3, 5, 8, 0)):
        assert lib.fmmt_unpack_rows(*bad, p, p, p, None) == _lib.FMMT_EINVAL, bad
    code = _lib.BF16 | _lib.RAGGED

    def fwd(dtype=code, T=130, B=2, E=128, H=2, rows=200, off=p, ld=384, drop=0.0):
        return lib.fmmt_mha_fwd_ragged(dtype, T, B, E, H, rows, off, p, p, ld, p, p, ld, 0.125, drop, 0, None, p, E, p, None)
    assert fwd(dtype=_lib.BF16) == _lib.FMMT_EINVAL                    # the mode flag is part of the call
    assert fwd(dtype=_lib.F32 | _lib.RAGGED) == _lib.FMMT_EINVAL
    assert fwd(E=64, H=2) == _lib.FMMT_EINVAL                           # head_dim 32: the matrix-core kernels only
    assert fwd(rows=0) == _lib.FMMT_EINVAL and fwd(rows=261) == _lib.FMMT_EINVAL      # more rows than B * T slots
    assert fwd(off=None) == _lib.FMMT_EINVAL and fwd(drop=1.0) == _lib.FMMT_EINVAL
    assert fwd(ld=388) == _lib.FMMT_EALIGN
    assert lib.fmmt_mha_bwd_ragged(_lib.BF16, 130, 2, 128, 2, 200, p, p, p, 384, p, p, 384, 0.125, 0.0, 0, None, p, p, 128, p, p, 384, p, p, 384, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_mha_bwd_ragged(code, 130, 2, 128, 2, 200, p, p, p, 384, p, p, 384, 0.125, 0.0, 0, None, p, p, 128, p, None, 384, p, p, 384, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_dropadd_ln_fwd_map(_lib.BF16, 0, 768, 1e-5, p, p, p, p, 0.1, 0, None, 0, p, p, p, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_dropadd_ln_bwd_map(_lib.BF16, 8, 768, 1e-5, p, p, p, 0.1, 0, None, 0, p, p, p, p, p, p, 0, p, None) == _lib.FMMT_EWORKSPACE


def test_token_counts_capacity_and_fit_on_the_host():
    from facialmmt_amd import train_step as ts
    m = torch.zeros(3, 20)
    for b, n in enumerate((20, 5, 12)):
        m[b, :n] = 1
    assert ts.count_tokens(m) == (37, True)
    assert ts.count_tokens(m.long().tolist()) == (37, True)
    assert ts.default_token_capacity(m, granule=8) == 40 and ts.default_token_capacity(m, granule=64) == 0       # 64 rows: no fewer than the 60 padded ones
    assert ts.TOKEN_GRANULE in (64, 128, 256)
    assert ts.token_fit(m, 40) and ts.token_fit(m, 37) and not ts.token_fit(m, 0)
    with pytest.raises(ValueError, match="token_capacity=36"):
        ts.token_fit(m, 36)
    holed = m.clone()
    holed[0, 3] = 0
    assert ts.count_tokens(holed) == (36, False)
    assert not ts.token_fit(holed, 40) and not ts.token_fit(holed, 8)     # a hole: the padded path, whatever the count
    assert ts.default_token_capacity(holed, granule=8) == 0
    left = torch.zeros(2, 6)
    left[:, 2:] = 1                                                        # padded on the left: no prefix either
    assert ts.count_tokens(left) == (8, False)
    assert ts.default_token_capacity(torch.zeros(2, 6)) == 0
    with pytest.raises(ValueError):
        ts.count_tokens(torch.zeros(5))
