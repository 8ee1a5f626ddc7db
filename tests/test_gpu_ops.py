"""GPU parity of every C-ABI entry point against a plain fp64 torch restatement of the same op
(tests/support_op_cases.py holds the cases: forward and backward, fp32 at ~1e-5 and bf16 at ~1e-2 relative to
the tensor scale, ragged M/N/K tails, PatchMerging gather, shifted windows with masks, packed and
separate k/v, dropout statistics, BatchNorm train/eval)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(fn_name):
    from tests import support_op_cases as P
    P.RES.clear()
    P.section(getattr(P, fn_name))
    bad = [n for n, ok in P.RES if not ok]
    assert P.RES and not bad, f"{fn_name}: failed cases: {bad}"


@pytest.mark.parametrize("case", ["t_linear", "t_linear_large", "t_wgrad", "t_wgrad_large", "t_mlp_fused", "t_gelu_tail", "t_layernorm", "t_wattn", "t_mha", "t_misc"])
def test_op_parity(case):
    assert torch.cuda.is_available()
    _run(case)


def test_argument_errors_raise_on_gpu():
    from facialmmt_amd import _lib, ops
    dev = torch.device("cuda:0")
    with pytest.raises(_lib.FmmtError, match="EINVAL"):
        ops.linear_raw(torch.zeros(8, 100, device=dev, dtype=torch.bfloat16), torch.zeros(96, 100, device=dev, dtype=torch.bfloat16), None)
    with pytest.raises(_lib.FmmtError):
        ops.mha_core(torch.zeros(4, 1, 500, device=dev), torch.zeros(4, 1, 1000, device=dev), None, 4, 1.0)
    with pytest.raises(_lib.FmmtError, match="unsupported activation dtype"):
        ops.layer_norm(torch.zeros(4, 96, device=dev, dtype=torch.float16), torch.ones(96, device=dev), torch.zeros(96, device=dev))


def test_mha_entry_points_refuse_bad_pitches_and_null_operands():
    """fmmt_mha_fwd / _bwd / _avg_weights hold their leading dimensions and pointers to the rules of the ragged entry points (include/fmmt.h): a pitch
    that is not a multiple of 16 bytes is FMMT_EALIGN (it used to fall to the VALU kernels, whose 16-byte vector accesses it would have misaligned),
    a pitch below E and a NULL required operand or output FMMT_EINVAL.  A refused call launches nothing: the outputs keep their NaN fill."""
    from facialmmt_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    EINVAL, EALIGN = -1, -2
    Lq, Lk, B, nh = 5, 7, 2, 2
    for dt, per16 in ((torch.bfloat16, 8), (torch.float32, 4)):
        for E in (128, 64):
            code, es = _lib.dtype_code(dt), torch.empty((), dtype=dt).element_size()
            W = E + 16                                              # the allocations are wide enough for every pitch tried below
            q, out, dout, dq = (torch.full((Lq * B, W), float("nan"), device=dev, dtype=dt) for _ in range(4))
            kv, dkv = (torch.full((Lk * B, 2 * W), float("nan"), device=dev, dtype=dt) for _ in range(2))
            lse = torch.full((B * nh * Lq,), float("nan"), device=dev)
            wts = torch.full((B * Lq * Lk,), float("nan"), device=dev)
            P = lambda t, off=0: t.data_ptr() + off * es

            def fwd(ldq=E, ldkv=2 * E, ldo=E, q_=P(q), k_=P(kv), v_=P(kv, E), out_=P(out), lse_=P(lse), flags=0):
                return lib.fmmt_mha_fwd(code | flags, Lq, Lk, B, E, nh, q_, ldq, k_, v_, ldkv, 0.125, None, 0.0, 0, None, out_, ldo, lse_, st)

            def bwd(ldq=E, ldkv=2 * E, ldo=E, lddq=E, lddkv=2 * E, q_=P(q), k_=P(kv), v_=P(kv, E), out_=P(out), dout_=P(dout), lse_=P(lse), dq_=P(dq), dk_=P(dkv),
                    dv_=P(dkv, E), flags=0):
                return lib.fmmt_mha_bwd(code | flags, Lq, Lk, B, E, nh, q_, ldq, k_, v_, ldkv, 0.125, None, 0.0, 0, None, out_, dout_, ldo, lse_, dq_, lddq, dk_, dv_,
                                        lddkv, st)

            def avg(ldq=E, ldkv=2 * E, q_=P(q), k_=P(kv), lse_=P(lse), w_=P(wts)):
                return lib.fmmt_mha_avg_weights(code, Lq, Lk, B, E, nh, q_, ldq, k_, ldkv, 0.125, None, 0.0, 0, None, lse_, w_, st)

            off = per16 // 2                                        # bf16: ld = 4 (mod 8); fp32: ld = 2 (mod 4) -- rows 8 bytes off a 16-byte boundary
            for flags in (0, _lib.BATCH_MAJOR):
                for name in ("ldq", "ldkv", "ldo"):
                    assert fwd(flags=flags, **{name: (2 * E if name == "ldkv" else E) + off}) == EALIGN, (dt, E, name)
                    assert fwd(flags=flags, **{name: E - per16}) == EINVAL, (dt, E, name)
                for name in ("ldq", "ldkv", "ldo", "lddq", "lddkv"):
                    assert bwd(flags=flags, **{name: (2 * E if name.endswith("kv") else E) + off}) == EALIGN, (dt, E, name)
                    assert bwd(flags=flags, **{name: E - per16}) == EINVAL, (dt, E, name)
            assert fwd(ldq=E + 1) == EALIGN and bwd(lddq=E + 1) == EALIGN   # an odd pitch: 2-byte aligned rows in bf16
            for name in ("ldq", "ldkv"):
                assert avg(**{name: (2 * E if name == "ldkv" else E) + off}) == EALIGN and avg(**{name: E - per16}) == EINVAL, (dt, E, name)
            for name in ("q_", "k_", "v_", "out_", "lse_"):
                assert fwd(**{name: None}) == EINVAL, (dt, E, name)
            for name in ("q_", "k_", "v_", "out_", "dout_", "lse_", "dq_", "dk_", "dv_"):
                assert bwd(**{name: None}) == EINVAL, (dt, E, name)
            for name in ("q_", "k_", "lse_", "w_"):
                assert avg(**{name: None}) == EINVAL, (dt, E, name)
            torch.cuda.synchronize()
            for t in (out, dq, dkv, lse, wts):
                assert bool(torch.isnan(t).all())                   # nothing was launched
    # the pitches every caller passes (E / 2E / E and 3E / 3E / 3E) and a wider multiple of 16 bytes are accepted
    E, dt = 128, torch.bfloat16
    q, out = torch.zeros(Lq * B, E + 8, device=dev, dtype=dt), torch.zeros(Lq * B, E + 24, device=dev, dtype=dt)
    kv = torch.zeros(Lk * B, 2 * E + 16, device=dev, dtype=dt)
    lse = torch.zeros(B * nh * Lq, device=dev)
    assert lib.fmmt_mha_fwd(_lib.BF16, Lq, Lk, B, E, nh, q.data_ptr(), E + 8, kv.data_ptr(), kv.data_ptr() + 2 * E, 2 * E + 16, 0.125, None, 0.0, 0, None, out.data_ptr(),
                            E + 24, lse.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lse).all())
