"""CPU tests of the ragged-batch feature: the ABI surface of include/fmmt_ragged.h and the torch formulation of the frame filter with padded rows."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_header_signatures_and_library_agree():
    """include/fmmt_ragged.h (included by fmmt.h) == _lib.RAGGED_SIGNATURES == the symbols of the built library: names, every argument's type and the
    return type, as test_pool_head_header_signatures_and_library_agree does for the pooling head; argument validation happens before any launch, so
    it runs without a GPU"""
    from facialmmt_amd import _lib, build
    assert "ragged.hip" in build.SOURCES
    assert '#include "fmmt_ragged.h"' in open(os.path.join(ROOT, "include", "fmmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmmt_ragged.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(fmmt_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert sorted(protos) == sorted(_lib.RAGGED_SIGNATURES) == ["fmmt_batchnorm1d_bwd_n", "fmmt_batchnorm1d_fwd_n", "fmmt_pack_frames", "fmmt_select_frames_fwd_n"]
    assert not set(_lib.RAGGED_SIGNATURES) & set(_lib.SIGNATURES) and not set(_lib.RAGGED_SIGNATURES) & set(_lib.POOL_HEAD_SIGNATURES)

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = " ".join(decl.replace("const", " ").split()[:-1])        # drop the parameter's name
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}[base]
    returns = {m.group(2): m.group(1) for m in re.finditer(r"\b(int|size_t)\s+(fmmt_\w+)\s*\(", src)}
    for name, args in protos.items():
        want = [ctype_of(a) for a in args.split(",") if a.strip()]
        res, got = _lib.RAGGED_SIGNATURES[name]
        assert got == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g is not w], len(got), len(want))
        assert res is {"int": C.c_int, "size_t": C.c_size_t}[returns[name]], name
    # the masked entry points are the unmasked ones with the row-count pointer added: the rest of the argument list is shared
    for masked, plain, at in (("fmmt_batchnorm1d_fwd_n", "fmmt_batchnorm1d_fwd", 3), ("fmmt_batchnorm1d_bwd_n", "fmmt_batchnorm1d_bwd", 3),
                              ("fmmt_select_frames_fwd_n", "fmmt_select_frames_fwd", 14)):
        a = list(_lib.RAGGED_SIGNATURES[masked][1])
        assert a.pop(at) is C.c_void_p and a == _lib.SIGNATURES[plain][1], masked
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in protos)
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in protos)
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    p += -p % 16
    assert lib.fmmt_pack_frames(3, 5, 8, 40, p, p, p, p, None) == _lib.FMMT_EALIGN           # a row that is no multiple of 16 bytes
    assert lib.fmmt_pack_frames(3, 5, 8, 48, p, p, p + 8, p, None) == _lib.FMMT_EALIGN
    for bad in ((0, 5, 8, 48), (257, 5, 8, 48), (3, 0, 8, 48), (3, 5, 0, 48), (3, 5, 65536, 48), (3, 5, 8, 0)):
        assert lib.fmmt_pack_frames(*bad, p, p, p, p, None) == _lib.FMMT_EINVAL, bad
    assert lib.fmmt_pack_frames(3, 5, 8, 48, None, p, p, p, None) == _lib.FMMT_EINVAL
    none11 = [None] * 11
    assert lib.fmmt_batchnorm1d_fwd_n(0, 40, 512, None, None, None, None, None, None, 0.1, 1e-5, 1, None, None, None, None) == _lib.FMMT_EINVAL   # no row count
    assert lib.fmmt_batchnorm1d_fwd_n(5, 40, 512, p, None, None, None, None, None, 0.1, 1e-5, 1, None, None, None, None) == _lib.FMMT_EINVAL
    assert lib.fmmt_batchnorm1d_bwd_n(0, 0, 512, p, *none11[:5], 1, *none11[:4]) == _lib.FMMT_EINVAL
    assert lib.fmmt_select_frames_fwd_n(0, 9000, 7, 2, 6, 16, None, None, None, None, 0.5, None, None, None, p, None) == _lib.FMMT_EINVAL


def _filter_case(case):
    """the two cases of tests/test_gpu_ragged_ops.py: B = 2, Lv = 6, num_imgs = [5, 2], 12 rows of preds of which 7 are faces"""
    g = torch.Generator().manual_seed(11)
    B, Lv, D, NL, cap, num_imgs, thr = 2, 6, 16, 7, 12, [5, 2], 0.5
    n = sum(num_imgs)
    near_uniform = torch.softmax(0.05 * torch.randn(cap, NL, generator=g), dim=1)
    one_hot = torch.eye(NL)[torch.randint(0, NL, (cap,), generator=g)] * 0.97 + 0.03 / NL
    passes = torch.tensor([1, 0, 1, 1, 0, 0, 1] + [1, 0, 1, 0, 1] if case == "mixed" else [0] * n + [1] * (cap - n), dtype=torch.bool)
    preds = torch.where(passes.view(-1, 1), one_hot, near_uniform)
    vin = torch.randn(B, Lv, D, generator=g)
    vmask = torch.zeros(B, Lv)
    for u, k in enumerate(num_imgs):
        vmask[u, :k] = 1
    return preds, vin, vmask, num_imgs, thr, n, torch.randn(B, Lv, D + NL, generator=g)


@pytest.mark.parametrize("case", ["mixed", "padded_only"])
def test_select_frames_torch_formulation_ignores_padded_rows(case):
    from facialmmt_amd.train_step import select_frames
    from oracle.train_glue import select_frames_loop
    preds, vin, vmask, num_imgs, thr, n, dout = _filter_case(case)
    pr = preds[:n].clone().requires_grad_(True)
    want, want_mask = select_frames_loop(pr, vin, vmask, num_imgs, thr)
    (want * dout).sum().backward()
    pd = preds.clone().requires_grad_(True)
    got, got_mask = select_frames(pd, vin, vmask, torch.tensor(num_imgs), thr, n_valid=torch.tensor([n, n], dtype=torch.int32))
    (got * dout).sum().backward()
    assert torch.equal(got.detach(), want.detach()) and torch.equal(got_mask, want_mask)
    assert torch.equal(pd.grad[:n], pr.grad) and float(pd.grad[n:].abs().max()) == 0.0
    if case == "padded_only":
        assert torch.equal(got_mask, vmask)
        _, other_mask = select_frames(preds, vin, vmask, torch.tensor(num_imgs), thr)      # every row counted: the padded rows flip the branch
        assert not torch.equal(other_mask, vmask)


def test_frame_total_is_checked_on_the_host_for_lists_and_cpu_tensors():
    from facialmmt_amd.train_step import check_frame_total
    check_frame_total([5, 2], 6, 12)
    check_frame_total([9, 9], 6, 12)                            # counts clamp to Lv, as the packing kernel clamps them
    check_frame_total(torch.tensor([6, 6]), 6, 12)
    for bad in ([6, 6], torch.tensor([6, 6])):
        with pytest.raises(ValueError, match="frame_capacity=8"):
            check_frame_total(bad, 6, 8)
