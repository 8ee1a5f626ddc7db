"""GPU tests of the text encoder on real tokens only (include/fmmt_tokens.h; train_step PACK_NOTE):

* the attention core's ragged mode against the padded batch-major call it restates -- EQUAL on the real rows, forward and backward, with and
  without dropout;
* the sublayer tails with a row map against the call on the padded layout;
* pack / unpack and the token layout;
* the whole fused encoder on packed rows against fp32, at the bar of tests/test_gpu_text_encoder.py;
* GraphedTargetStep with token packing against the same step on the padded layout; the capacity check; a mask with a hole and the update behind it;
* three frame capacities with the fused update: a packed capture and a padded twin per capacity;
* the eager TargetStep, which packs every batch into its own capacity, with the text encoder's dropout off and on."""
import copy
import types

import pytest
import torch

from tests import test_gpu_text_encoder as TE

pytestmark = pytest.mark.gpu

E, NH = TE.E, TE.NH
SENTINEL = 12345.0


def _mask(lens, T, dev):
    m = torch.zeros(len(lens), T, device=dev)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    return m


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the attention core
# ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T,lens", [(130, (130, 77, 64, 129, 2)), (512, (400, 512, 2, 449))])
def test_ragged_attention_equals_the_padded_call_on_the_real_rows(T, lens, p):
    """16 heads x 64.  The padded call: fmmt_mha_fwd / _bwd | FMMT_BATCH_MAJOR on (B, T) with key_bias = -30000 on the padded keys and -- what the
    encoder's padded rows receive, whose outputs nobody reads -- zero dout on the padded queries.  The ragged call on the packed real rows (five
    filler rows of garbage behind them) must give the same BITS for out and lse on the real rows and for dq, dk, dv: a fully masked key tile adds
    exact zeros to the padded call's accumulators.  lse entries of padded queries keep the sentinel; the filler rows of out / dqkv are zeros."""
    from facialmmt_amd import _lib, ops
    dev = torch.device("cuda:0")
    torch.manual_seed(31)
    B, total = len(lens), sum(lens)
    cap = total + 5
    seed = torch.tensor([0x7ea51234], device=dev, dtype=torch.int64)
    mask = _mask(lens, T, dev)
    real = mask.bool()
    qkv = torch.randn(B, T, 3 * E, device=dev).to(torch.bfloat16)
    dout = (torch.randn(B, T, E, device=dev) * mask[..., None]).to(torch.bfloat16)
    kb = torch.where(real, 0.0, -30000.0).float().contiguous()
    out_ref, lse_ref = ops.mha_packed_bm_fwd_raw(qkv, NH, 0.125, p, 0, seed, kb)
    d_ref = ops.mha_packed_bm_bwd_raw(qkv, out_ref, dout, lse_ref, NH, 0.125, p, 0, seed, kb)

    lay = ops.token_layout_raw(mask, cap)
    assert lay.seq_len.tolist() == list(lens) and lay.counts.tolist() == [total, total]
    garbage = lambda w: torch.full((5, w), 3.0e4, device=dev, dtype=torch.bfloat16)
    qkv_p = torch.cat([qkv[real], garbage(3 * E)]).contiguous()
    dout_p = torch.cat([dout[real], garbage(E)]).contiguous()
    out = torch.full((cap, E), SENTINEL, device=dev, dtype=torch.bfloat16)
    lse = torch.full((B, NH, T), SENTINEL, device=dev)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    code = _lib.BF16 | _lib.RAGGED
    qp, kp, vp = (qkv_p.data_ptr() + i * E * 2 for i in range(3))
    _lib.check(lib.fmmt_mha_fwd_ragged(code, T, B, E, NH, cap, lay.seq_off.data_ptr(), lay.seq_len.data_ptr(), qp, 3 * E, kp, vp, 3 * E, 0.125, p, 0,
                                       seed.data_ptr(), out.data_ptr(), E, lse.data_ptr(), st), "fwd")
    assert torch.equal(out[:total], out_ref[real])
    assert (out[total:] == 0).all()
    lse_ref = lse_ref.view(B, NH, T)
    qreal = real[:, None, :].expand(B, NH, T)
    assert torch.equal(lse[qreal], lse_ref[qreal])
    assert (lse[~qreal] == SENTINEL).all()
    dqkv = torch.full((cap, 3 * E), SENTINEL, device=dev, dtype=torch.bfloat16)
    dq, dk, dv = (dqkv.data_ptr() + i * E * 2 for i in range(3))
    _lib.check(lib.fmmt_mha_bwd_ragged(code, T, B, E, NH, cap, lay.seq_off.data_ptr(), lay.seq_len.data_ptr(), qp, 3 * E, kp, vp, 3 * E, 0.125, p, 0,
                                       seed.data_ptr(), out.data_ptr(), dout_p.data_ptr(), E, lse.data_ptr(), dq, 3 * E, dk, dv, 3 * E, st), "bwd")
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.equal(dqkv[:total, i * E:(i + 1) * E], d_ref[real][:, i * E:(i + 1) * E]), name
    assert (dqkv[total:] == 0).all()
    assert float(d_ref[real].float().abs().max()) > 0 and torch.isfinite(dqkv.float()).all()
    # the helpers the autograd node uses are the same two calls
    out2, lse2 = ops.mha_ragged_fwd_raw(qkv_p, lay, NH, 0.125, p, 0, seed)
    assert torch.equal(out2, out) and torch.equal(lse2.view(B, NH, T)[qreal], lse[qreal])
    assert torch.equal(ops.mha_ragged_bwd_raw(qkv_p, lay, out2, dout_p, lse2, NH, 0.125, p, 0, seed), dqkv)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the sublayer tails
# ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [768, 1024])
def test_tails_with_the_row_map_equal_the_padded_call(C):
    """M = 37 packed rows of a 3 x 20 padded layout, p = 0.1.  The padded call gets zero input and zero dy on its padded rows (a zero row's
    LayerNorm' is zero: it adds nothing to any column sum).  Forward, dx and dh are row-wise: EQUAL.  d gamma, d beta and the bias gradient are sums
    over rows that the two calls group differently (4 and 7 workgroups): held to the padded call by the 8e-3 x max bar of
    tests/test_gpu_text_encoder.py::_embedding_case."""
    from facialmmt_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(32)
    lens, T, p, eps, salt = (20, 5, 12), 20, 0.1, 1e-5, 5 << 40
    mask = _mask(lens, T, dev)
    real = mask.bool().reshape(-1)
    seed = torch.tensor([424242], device=dev, dtype=torch.int64)
    lay = ops.token_layout_raw(mask, 37)
    assert lay.row_map.tolist() == real.nonzero().reshape(-1).tolist()
    pad = lambda: (torch.randn(3 * T, C, device=dev) * real[:, None]).to(torch.bfloat16)
    h, res, dy = pad(), pad(), pad()
    gm = (1 + 0.1 * torch.randn(C, device=dev)).to(torch.bfloat16)
    bt = (0.1 * torch.randn(C, device=dev)).to(torch.bfloat16)
    xs_ref, y_ref = ops.plm_tail_fwd_raw(h, res, gm, bt, eps, p, 0, seed, salt)
    ref = ops.plm_tail_bwd_raw(dy, xs_ref, gm, eps, p, 0, seed, salt)
    xs, y = ops.plm_tail_fwd_raw(h[real].contiguous(), res[real].contiguous(), gm, bt, eps, p, 0, seed, salt, lay.row_map)
    got = ops.plm_tail_bwd_raw(dy[real].contiguous(), xs, gm, eps, p, 0, seed, salt, lay.row_map)
    assert torch.equal(xs, xs_ref[real]) and torch.equal(y, y_ref[real])
    dropped = ((xs.float() - res[real].float()) == 0) & (h[real] != 0)
    assert 0.05 < dropped.float().mean().item() < 0.15                       # the mask is there, and it is the padded call's
    # without the map the packed rows would draw another mask
    xs_plain, _ = ops.plm_tail_fwd_raw(h[real].contiguous(), res[real].contiguous(), gm, bt, eps, p, 0, seed, salt)
    assert not torch.equal(xs_plain, xs)
    assert torch.equal(got[0], ref[0][real]) and torch.equal(got[1], ref[1][real])
    for a, r, name in zip(got[2:], ref[2:], ("dgamma", "dbeta", "dbias")):
        err, bar = (a.float() - r.float()).abs().max().item(), 8e-3 * r.float().abs().max().item() + 1e-6
        print(f"C={C} {name}: max|packed - padded| {err:.3e}, bar {bar:.3e}")
        assert err <= bar, name


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. layout, pack, unpack
# ------------------------------------------------------------------------------------------------------------------------------------

def test_layout_pack_and_unpack_round_trip():
    """lens including 0 and T; zeros in the filler and at padded positions; each direction is the other's backward; a mask with a hole or too many
    tokens is reported in counts and cut to the capacity"""
    from facialmmt_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(33)
    lens, T, cap = (6, 0, 3, 1), 6, 16
    total = sum(lens)
    mask = _mask(lens, T, dev)
    real = mask.bool()
    lay = ops.token_layout_raw(mask.long(), cap)
    assert lay.seq_len.tolist() == list(lens) and lay.seq_off.tolist() == [0, 6, 6, 9] and lay.len64.tolist() == list(lens)
    assert lay.counts.tolist() == [total, total]
    want = [b * T + t for b, n in enumerate(lens) for t in range(n)] + [len(lens) * T + r for r in range(total, cap)]
    assert lay.row_map.tolist() == want
    x = torch.randn(len(lens), T, 8, device=dev).requires_grad_(True)       # 32-byte rows
    pk = ops.pack_rows(x, lay)
    assert pk.shape == (cap, 8) and torch.equal(pk[:total], x.detach()[real]) and (pk[total:] == 0).all()
    up = ops.unpack_rows(pk, lay)
    assert torch.equal(up, x.detach() * mask[..., None])
    g = torch.randn_like(up)
    (gx,) = torch.autograd.grad(up, x, g)
    assert torch.equal(gx, g * mask[..., None])                              # through both backwards: padded positions get no gradient
    w = torch.randn(cap, 8, device=dev).requires_grad_(True)
    (gw,) = torch.autograd.grad(ops.unpack_rows(w, lay), w, g)
    assert torch.equal(gw[:total], g[real]) and (gw[total:] == 0).all()
    bf = torch.randn(len(lens), T, E, device=dev).to(torch.bfloat16)         # the encoder's row
    assert torch.equal(ops.unpack_rows(ops.pack_rows(bf, lay), lay), bf * mask[..., None].to(torch.bfloat16))
    holed = mask.clone()
    holed[0, 2] = 0
    lh = ops.token_layout_raw(holed, cap)
    assert lh.seq_len.tolist() == [2, 0, 3, 1] and lh.counts.tolist() == [6, total - 1]
    small = ops.token_layout_raw(mask, 8)                                    # 10 tokens into 8 rows: cut, nothing out of bounds
    assert small.seq_len.tolist() == [6, 0, 2, 0] and small.counts.tolist() == [8, total] and small.row_map.tolist() == want[:8]
    pk8 = ops.pack_rows(x.detach(), small)
    assert torch.equal(pk8, x.detach()[real][:8])


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the whole encoder on packed rows
# ------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def encoders():
    dev = torch.device("cuda:0")
    ref = TE._roberta(dev).float().train()
    stock = copy.deepcopy(ref).to(torch.bfloat16).train()
    fused = copy.deepcopy(stock)
    assert TE._fuse(fused) == (4, 2) and fused._fmmt_fused_ffn == 2 and fused._fmmt_box.all_attention_fused
    return ref, stock, fused


@pytest.mark.parametrize("case", sorted(TE.ENCODER_CASES))
def test_whole_encoder_on_packed_rows_against_fp32(encoders, case, monkeypatch):
    """geometry, cases, inputs and the per-tensor bar (FACTOR x the stock bf16 module's relative L2 to fp32 + SLACK) of
    tests/test_gpu_text_encoder.py::test_whole_encoder_at_roberta_large_geometry_against_fp32, the fused encoder on packed rows (capacity: the real
    tokens rounded up to 64).  What differs from that test is the loss, for all three modules alike: it reads the real tokens only (dy is zero
    on the padded rows, the output is compared on the real rows) -- the use the packing is valid for; packed, the padded rows come back as zeros."""
    from facialmmt_amd import ops
    ref, stock, fused = encoders
    dev = torch.device("cuda:0")
    B, S, lens = TE.ENCODER_CASES[case]
    g = torch.Generator(device=dev).manual_seed(11)
    ids = torch.randint(3, 50265, (B, S), generator=g, device=dev)
    ids[:, 0] = 0
    mask = _mask(lens, S, dev)
    ids[mask == 0] = 1
    ids[1, 5:9] = 7
    dy = torch.randn(B, S, E, generator=g, device=dev) * mask[..., None]
    cap = (sum(lens) + 63) // 64 * 64
    assert cap < B * S
    outs = []
    n = None
    for m in (ref, stock, fused):
        for p in m.parameters():
            p.grad = None
        if m is fused:
            n = TE._counters(monkeypatch)
            box = fused._fmmt_box
            box.capacity = cap
            y = m(ids, mask.to(torch.float32)).last_hidden_state
            box.capacity = 0
            lay = box.take_layout()
            assert lay is not None and tuple(y.shape) == (1, cap, E) and box.take_layout() is None
            assert torch.isfinite(y.float()).all()                  # the filler rows included: they run through the layers like any row ...
            y = ops.unpack_rows(y[0], lay)
            assert (y[mask == 0] == 0).all()                        # ... and never come back
        else:
            y = m(ids, mask.to(torch.float32)).last_hidden_state
        y.backward(dy.to(y.dtype))
        outs.append(((y.detach().float() * mask[..., None]), {k: p.grad.detach().float() for k, p in m.named_parameters() if p.grad is not None}))
        monkeypatch.undo()
    assert n == {"PlmSelfAttnFn": 2, "PlmFfnFn": 2, "PlmEmbeddingFn": 3}, n
    (yr, gr), (ys, gs), (yf, gf) = outs
    assert set(gr) == set(gs) == set(gf)
    ratios = {}
    for k, r in [("last_hidden_state", yr)] + sorted(gr.items()):
        if k.endswith("key.bias"):
            continue
        s, f = (ys, yf) if k == "last_hidden_state" else (gs[k], gf[k])
        rs = TE._rel(s, r)
        ratios[k] = (TE._check_close(k, f, r, TE.FACTOR * rs + TE.SLACK, 4e-2), rs)
    worst = max(ratios, key=lambda k: ratios[k][0] / (ratios[k][1] + 1e-9))
    print(f"\n{case} packed into {cap} rows: worst fused / stock relative L2 {worst}: {ratios[worst][0]:.3e} / {ratios[worst][1]:.3e}; "
          f"median ratio {sorted(a / (b + 1e-9) for a, b in ratios.values())[len(ratios) // 2]:.3f}")
    pos = torch.cumsum((ids != 1).int(), 1) * (ids != 1).int() + 1
    for table, used in (("embeddings.word_embeddings.weight", ids), ("embeddings.position_embeddings.weight", pos)):
        gw = gf[table]
        assert (gw[1] == 0).all(), table
        named = torch.zeros(gw.shape[0], dtype=torch.bool, device=dev)
        named[used.reshape(-1)] = True
        named[1] = False
        assert (gw[~named] == 0).all(), table
        assert (gw[named].abs().sum(1) > 0).all(), table
    # a forward without a capacity runs padded again
    assert tuple(fused(ids, mask.to(torch.float32)).last_hidden_state.shape) == (B, S, E)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. the graphed step
# ------------------------------------------------------------------------------------------------------------------------------------

B_UTT, LV, CAP = 2, 6, 12


def _small_roberta(p=0.0):
    from transformers import RobertaConfig, RobertaModel
    torch.manual_seed(3)
    cfg = RobertaConfig(vocab_size=1000, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=514,
                        type_vocab_size=1, pad_token_id=1, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    return RobertaModel(cfg, add_pooling_layer=False)


def _step(dev, token_capacity, frame_capacity=CAP, adamw=False, exchange=False):
    """the models and batch of tests/test_gpu_ragged_step.py (fp32 fusion stack and Swin, tau = 1e5, dropout and DropPath off, SGD, frame capacity 12)
    with a two-layer bf16 RoBERTa (2 heads x 64) under MasterWeights as the text encoder, so that the fused encoder -- the thing that packs -- runs.
    `exchange` (needs an initialised process group): under GradientAverager(always=True, hooks=False, bucket_mb=1), the two-piece mode"""
    import bench
    from facialmmt_amd import models, synth
    from facialmmt_amd.config import default_args
    from facialmmt_amd.train_step import GraphedTargetStep, HFAdamW, MasterWeights, step_parameters
    cfg = default_args(get_vision_utt_max_lens=LV, get_audio_utt_max_lens=24, trg_accumulation_steps=1, plm_module=_small_roberta(),
                       hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, crossmodal_attn_dropout_TA=0.0, crossmodal_attn_dropout_TA_V=0.0,
                       tau=1e5, FacialEmoImpor_threshold=0.1)
    cfg.compute_dtype = torch.float32
    swin = models.SwinForAffwildClassification(cfg)
    mm = models.MultiModalTransformerForClassification(cfg)
    plm_state = copy.deepcopy(mm.roberta.state_dict())
    synth.fill_state_dict(swin, seed=100)
    synth.fill_state_dict(mm, seed=200)
    mm.roberta.load_state_dict(plm_state)                         # the encoder keeps its own initialisation (LayerNorm weights of 1, small matrices)
    for m in swin.modules():
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    swin.to(dev).train()
    mm.to(dev).train()
    args = types.SimpleNamespace(utts=B_UTT, frames=LV, dtype="fp32", plm="roberta-large", input="float", resize="pil")
    batch = list(bench.synth_batch(args, dev, 0, cfg))
    batch[0] = batch[0] % 1000
    batch[0][batch[1] == 0] = 1                                   # padded positions hold the padding id
    batch[8] = batch[8].view(B_UTT, LV, 3, 224, 224)
    batch[9] = [5, 2]
    vmask = torch.zeros(B_UTT, LV, device=dev)
    vmask[0, :5] = 1
    vmask[1, :2] = 1
    batch[6] = vmask
    masters = MasterWeights(mm.roberta, torch.bfloat16)
    if adamw:                                                     # the fused update, whose hand-over takes one pinned table per capture
        opt = HFAdamW(step_parameters(mm, masters), lr=torch.tensor(1e-5, device=dev), weight_decay=0.01)
    else:
        opt = torch.optim.SGD(step_parameters(mm, masters), lr=0.05)
    avg = None
    if exchange:
        from facialmmt_amd.parallel import GradientAverager
        avg = GradientAverager(step_parameters(mm, masters), hooks=False, bucket_mb=1, always=True)
    step = GraphedTargetStep(swin, mm, opt, None, cfg, tuple(batch), autocast_dtype=None, masters=masters, frame_capacity=frame_capacity,
                             token_capacity=token_capacity, averager=avg)
    return step, mm, masters, tuple(batch)


def _sample(mm, masters):
    """a parameter sample after the update: the text encoder's fp32 masters (first / last layer, embeddings) and the fusion stack's head"""
    named = dict(mm.named_parameters())
    by_id = {id(p): m for p, m in masters.pairs()}
    keys = [k for k in named if k.startswith("roberta.") and (".layer.0." in k or ".layer.1." in k or "embeddings" in k)] + ["text_linear.weight", "classifier.weight"]
    return {k: by_id.get(id(named[k]), named[k]).detach().float().clone() for k in keys}


def test_graphed_step_on_packed_tokens_matches_the_padded_step():
    """one step packed (the default capacity) and one with token_capacity=0 from the same state: the loss, the kept-frame mask and a parameter sample
    after the update within the bars tests/test_gpu_step_oracle.py::compare_trajectory applies to the padded step against its fp64 reference -- loss to
    2e-4 x max(1, |loss|), equal masks, parameters to 1e-4 x max(1, max|p|).  Then: more tokens than the capacity raise before anything is copied;
    a mask with a hole replays the padded twin and gives what the padded step gives."""
    from facialmmt_amd import train_step as ts
    dev = torch.device("cuda:0")
    runs = {}
    for side, tc in (("packed", None), ("padded", 0)):
        step, mm, masters, batch = _step(dev, tc)
        total, prefix = ts.count_tokens(batch[1])
        assert prefix and 0 < total < batch[1].numel()
        if side == "packed":
            assert step.token_capacity == (total + ts.TOKEN_GRANULE - 1) // ts.TOKEN_GRANULE * ts.TOKEN_GRANULE and (CAP, False) in step._captures
            assert getattr(mm, "text_token_capacity", 0) == 0       # nobody else who calls the model runs packed
        else:
            assert step.token_capacity == 0 and not [k for k in step._captures if not k[1]]
        before = _sample(mm, masters)
        loss, kept = step(batch)
        torch.cuda.synchronize()
        after = _sample(mm, masters)
        assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith("roberta."))      # the encoder was stepped
        runs[side] = (float(loss), kept.clone(), after, step, mm, masters, batch)
    (l1, k1, p1, step, mm, masters, batch), (l0, k0, p0, step0, mm0, masters0, _) = runs["packed"], runs["padded"]
    assert step.token_replays == {"packed": 1, "padded": 0}
    print(f"loss packed {l1:.9f} padded {l0:.9f}")
    assert abs(l1 - l0) <= 2e-4 * max(1.0, abs(l0))
    assert torch.equal(k1, k0) and float(k0.sum()) > 0
    worst = max(((p1[k] - p0[k]).abs().max().item() / max(1.0, p0[k].abs().max().item()), k) for k in p0)
    print(f"parameters after the update: worst {worst[1]} {worst[0]:.3e} of max(1, max|p|)")
    assert worst[0] <= 1e-4, worst
    # over capacity: a mask of ones
    full = batch[:1] + (torch.ones_like(batch[1]),) + batch[2:]
    i_before, sample = step.i_batch, _sample(mm, masters)
    with pytest.raises(ValueError, match=f"token_capacity={step.token_capacity}"):
        step(full)
    torch.cuda.synchronize()
    assert step.i_batch == i_before and all(torch.equal(sample[k], v) for k, v in _sample(mm, masters).items())
    with pytest.raises(ValueError, match="token_capacity"):
        ts.GraphedTargetStep(step.swin, mm, step.opt, None, step.args, batch, autocast_dtype=None, masters=masters, frame_capacity=CAP, token_capacity=64)
    with pytest.raises(NotImplementedError):
        ts.GraphedTargetStep(step.swin, mm, step.opt, None, step.args, batch, autocast_dtype=None, masters=masters, token_capacity=1024, pipeline_swin=True)
    # a hole: the padded twin, and what the padded step computes for the same batch (both stepped once so far, from the same state, within 1e-4)
    holed_mask = batch[1].clone()
    holed_mask[0, 3] = 0
    holed = batch[:1] + (holed_mask,) + batch[2:]
    la, ka = step(holed)
    lb, kb = step0(holed)
    torch.cuda.synchronize()
    assert step.token_replays == {"packed": 1, "padded": 1}
    print(f"holed mask: loss {float(la):.9f} (twin) {float(lb):.9f} (padded step)")
    assert abs(float(la) - float(lb)) <= 2e-4 * max(1.0, abs(float(lb))) and torch.equal(ka, kb)
    # the update behind the twin's replay took the twin's gradients: the parameters follow the padded step's through its second update
    pa, pb = _sample(mm, masters), _sample(mm0, masters0)
    assert any(not torch.equal(p1[k], pa[k]) for k in pa if k.startswith("roberta."))
    worst = max(((pa[k] - pb[k]).abs().max().item() / max(1.0, pb[k].abs().max().item()), k) for k in pb)
    print(f"parameters after the twin's update: worst {worst[1]} {worst[0]:.3e} of max(1, max|p|)")
    assert worst[0] <= 1e-4, worst
    l2, _ = step(batch)                                           # and packed again
    l2b, _ = step0(batch)
    assert step.token_replays == {"packed": 2, "padded": 1} and abs(float(l2) - float(l2b)) <= 2e-4 * max(1.0, abs(float(l2b)))


def test_graphed_step_with_three_frame_capacities_packs_and_keeps_a_twin_per_capacity():
    """frame_capacity=(8, 10, 12) with the fused update (HFAdamW: the hand-over takes a pinned table per capture) and packing on: six
    forward/backward captures.  A packed replay in the smallest capacity, a twin's replay (mask with a hole) in the middle one, a packed replay in the
    largest; against the same calls of the step built with token_capacity=0: losses to 2e-4 x max(1, |loss|), equal masks, and the total gradient norm
    the hand-over leaves behind every call -- the gradients the update then reads, the twin's through the twin's own table -- to 1e-4 relative
    (tests/test_gpu_step_oracle.py::compare_trajectory's bars).  No parameter comparison: Adam's first updates are lr x sign(g), which turns the rounding
    noise of an analytically zero gradient (the key bias) into a full-size difference."""
    dev = torch.device("cuda:0")
    caps = (8, 10, 12)
    got = {}
    for side, tc in (("packed", None), ("padded", 0)):
        step, mm, masters, batch = _step(dev, tc, frame_capacity=caps, adamw=True)
        assert step.fused is not None and step.handover is not None
        if side == "packed":
            assert step.token_capacity > 0 and sorted(c for c, packed in step._captures if not packed) == list(caps)
            assert sorted(step.twin_capture_bytes) == sorted(step.twin_capture_reserved_bytes) == list(caps) == sorted(step.capture_bytes)
        holed = batch[1].clone()
        holed[0, 3] = 0
        calls = [batch[:9] + ([5, 2],) + batch[10:], batch[:1] + (holed,) + batch[2:9] + ([5, 4],) + batch[10:], batch[:9] + ([6, 5],) + batch[10:]]
        out = []
        for b in calls:
            vm = _mask(b[9], LV, dev)
            loss, kept = step(b[:6] + (vm,) + b[7:])
            out.append((float(loss), kept.clone(), step.capacity, float(step.fused.norm)))
        torch.cuda.synchronize()
        assert [o[2] for o in out] == list(caps) and step.replays == {c: 1 for c in caps}
        assert step.token_replays == ({"packed": 2, "padded": 1} if side == "packed" else {"packed": 0, "padded": 0})
        got[side] = out
    for (l1, k1, _, n1), (l0, k0, _, n0) in zip(got["packed"], got["padded"]):
        print(f"three capacities: loss packed step {l1:.9f} padded step {l0:.9f}; total norm {n1:.6e} {n0:.6e}")
        assert abs(l1 - l0) <= 2e-4 * max(1.0, abs(l0)) and torch.equal(k1, k0)
        assert n0 > 0 and abs(n1 - n0) <= 1e-4 * n0


@pytest.mark.parametrize("p_text", [0.0, 0.1])
def test_eager_step_packs_every_batch_into_its_own_capacity(p_text):
    """p_text = 0.1: the text encoder's hidden and attention dropout on, the generator reseeded in front of each step's call -- the embeddings' torch
    dropout, the seed words of the fused nodes and every draw behind the text branch are then the same on both sides, and the packed side draws the
    padded side's masks only if the row map reaches the tails and the feed-forward node and the ragged attention keeps the padded counters.
    TargetStep (nothing captured): token_capacity=None packs each batch into its own token count rounded up to TOKEN_GRANULE, 0 keeps the padded
    layout; one step each from the same state -- loss to 2e-4 x max(1, |loss|), equal masks, the fp32 parameters above the encoder to 1e-4 x
    max(1, max|p|) (the bars of test_graphed_step_on_packed_tokens_matches_the_padded_step).  An explicit capacity below the batch's tokens raises; a mask
    with a hole runs padded; the model's own attribute is back to 0 behind every call."""
    import bench
    from facialmmt_amd import models, synth
    from facialmmt_amd import train_step as ts
    from facialmmt_amd.config import default_args
    dev = torch.device("cuda:0")
    runs = {}
    for side, tc in (("packed", None), ("padded", 0), ("small", 64)):
        cfg = default_args(get_vision_utt_max_lens=LV, get_audio_utt_max_lens=24, trg_accumulation_steps=1, plm_module=_small_roberta(p_text),
                           hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, crossmodal_attn_dropout_TA=0.0, crossmodal_attn_dropout_TA_V=0.0,
                           tau=1e5, FacialEmoImpor_threshold=0.1)
        cfg.compute_dtype = torch.float32
        swin, mm = models.SwinForAffwildClassification(cfg), models.MultiModalTransformerForClassification(cfg)
        plm_state = copy.deepcopy(mm.roberta.state_dict())
        synth.fill_state_dict(swin, seed=100)
        synth.fill_state_dict(mm, seed=200)
        mm.roberta.load_state_dict(plm_state)
        for m in swin.modules():
            if hasattr(m, "drop_prob"):
                m.drop_prob = 0.0
        swin.to(dev).train()
        mm.to(dev).train()
        mm.roberta.to(torch.bfloat16)
        ts.use_colsum_bias_gradients(mm.roberta)
        assert ts.fuse_text_encoder(mm.roberta) == (4, 2) and ts.token_box(mm) is not None
        args = types.SimpleNamespace(utts=B_UTT, frames=LV, dtype="fp32", plm="roberta-large", input="float", resize="pil")
        batch = list(bench.synth_batch(args, dev, 0, cfg))
        batch[0] = batch[0] % 1000
        batch[0][batch[1] == 0] = 1
        batch[8] = batch[8].view(B_UTT, LV, 3, 224, 224)
        batch[9] = [5, 2]
        batch[6] = _mask((5, 2), LV, dev)
        step = ts.TargetStep(swin, mm, torch.optim.SGD(mm.parameters(), lr=0.05), None, cfg, autocast_dtype=None, frame_capacity=CAP, token_capacity=tc)
        total, prefix = ts.count_tokens(batch[1])
        if side == "small":
            with pytest.raises(ValueError, match="token_capacity=64"):
                step(tuple(batch))
            assert step.i_batch == 0
            continue
        torch.manual_seed(77)
        loss, kept = step(tuple(batch))
        torch.cuda.synchronize()
        assert step.token_rows == ((total + ts.TOKEN_GRANULE - 1) // ts.TOKEN_GRANULE * ts.TOKEN_GRANULE if side == "packed" else 0)
        assert mm.text_token_capacity == 0
        runs[side] = (float(loss), kept.clone(), {k: mm.state_dict()[k].detach().float().clone() for k in ("text_linear.weight", "classifier.weight")})
        if side == "packed":
            holed = batch[1].clone()
            holed[1, 2] = 0
            step(tuple(batch[:1] + [holed] + batch[2:]))
            assert step.token_rows == 0
            # an exception between the choice and the forward leaves the model on the padded layout
            tight = ts.TargetStep(swin, mm, step.opt, None, cfg, autocast_dtype=None, frame_capacity=4)
            with pytest.raises(ValueError, match="frame_capacity=4"):
                tight(tuple(batch))
            assert tight.token_rows > 0 and mm.text_token_capacity == 0
    (l1, k1, p1), (l0, k0, p0) = runs["packed"], runs["padded"]
    print(f"eager, text dropout {p_text}: loss packed {l1:.9f} padded {l0:.9f}")
    assert abs(l1 - l0) <= 2e-4 * max(1.0, abs(l0)) and torch.equal(k1, k0) and float(k0.sum()) > 0
    for k in p0:
        assert (p1[k] - p0[k]).abs().max().item() <= 1e-4 * max(1.0, p0[k].abs().max().item()), k
