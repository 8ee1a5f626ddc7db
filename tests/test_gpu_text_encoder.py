"""GPU tests of the fused text encoder (train_step.fuse_text_encoder: ops.PlmSelfAttnFn, PlmFfnFn, PlmSublayerTailFn, PlmEmbeddingFn over
csrc/plm_fused.hip and csrc/mha_mfma.hip) at the benchmark's RoBERTa-large geometry and at the edges of its inputs:

* the whole encoder (hidden 1024, 16 heads, FFN 4096, 4 x 512 tokens with ragged key padding: partly and fully masked 64-key tiles; a ragged
  130-token batch) against an fp32 copy, next to the stock bf16 module's own distance from it;
* the attention core and the feed-forward node with dropout at the benchmark shape, against fp32 torch on the mask the kernels drew;
* the embedding weight gradient over its whole promised range (T <= 32768 indices: past 64 KiB of LDS);
* attention masks that are not per-key padding (sequence packing, causal) take the stock attention, not the first query row's mask;
* a chunked feed-forward (config.chunk_size_feed_forward) draws a fresh dropout mask per chunk.

The small-shape tests of the same code are in test_gpu_glue.py."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

E, NH, FF = 1024, 16, 4096                                   # bench.py plm_config("roberta-large"): the layer geometry


def _roberta(dev, vocab=50265, layers=2, p_hidden=0.0, p_attn=0.0, **kw):
    from transformers import RobertaConfig, RobertaModel
    torch.manual_seed(0)
    cfg = RobertaConfig(vocab_size=vocab, hidden_size=E, num_hidden_layers=layers, num_attention_heads=NH, intermediate_size=FF,
                        max_position_embeddings=514, type_vocab_size=1, pad_token_id=1, hidden_dropout_prob=p_hidden,
                        attention_probs_dropout_prob=p_attn, **kw)
    return RobertaModel(cfg, add_pooling_layer=False).to(dev)


def _fuse(m):
    """what MasterWeights does to the bf16 text encoder of the benchmark"""
    from facialmmt_amd.train_step import fuse_text_encoder, use_colsum_bias_gradients
    use_colsum_bias_gradients(m)
    return fuse_text_encoder(m)


def _counters(monkeypatch):
    """call counters on the fused nodes' entry points (the fused path is really taken)"""
    from facialmmt_amd import ops
    n = {}
    for name in ("PlmSelfAttnFn", "PlmFfnFn", "PlmEmbeddingFn"):
        cls = getattr(ops, name)
        real = cls.apply
        n[name] = 0

        def wrap(*a, _real=real, _name=name):
            n[_name] += 1
            return _real(*a)
        monkeypatch.setattr(cls, "apply", wrap)
    return n


def _rel(a, r):
    return ((a.double() - r.double()).norm() / (r.double().norm() + 1e-30)).item()


def _drop_inv(p):
    """the kernels' realised 1 / keep rate: 2^16 / (2^16 - round(p 2^16)) (fmmt_common.h attn_drop_setup / elem_drop_setup)"""
    t = min(int(float(torch.tensor(p, dtype=torch.float32) * 65536.0) + 0.5), 65535)
    return 65536.0 / (65536.0 - t)


def _check_close(name, a, r, rel_tol, abs_frac):
    rel = _rel(a, r)
    scale = r.abs().max().item() + 1e-6
    err = (a.float() - r.float()).abs().max().item()
    assert rel <= rel_tol and err <= abs_frac * scale, (name, rel, rel_tol, err, scale)
    return rel


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the whole encoder at RoBERTa-large geometry, dropout off
# ------------------------------------------------------------------------------------------------------------------------------------

# (B, S, real tokens per row): bench.py pads keys 400..511; 2 real tokens leave seven fully masked key tiles; 449 cuts a tile after its first key
ENCODER_CASES = {"bench_512": (4, 512, (512, 400, 2, 449)), "ragged_130": (3, 130, (130, 77, 129))}
# fused relative L2 to fp32 <= FACTOR x the stock bf16 module's + SLACK, per tensor.  Measured on the MI355X: worst ratio 1.03 (a value / query bias
# gradient of layer 1), median 0.97 in both cases
FACTOR, SLACK = 1.2, 1e-3


@pytest.fixture(scope="module")
def encoders():
    dev = torch.device("cuda:0")
    ref = _roberta(dev).float().train()
    stock = copy.deepcopy(ref).to(torch.bfloat16).train()
    fused = copy.deepcopy(stock)
    assert _fuse(fused) == (4, 2) and fused._fmmt_fused_ffn == 2
    return ref, stock, fused


@pytest.mark.parametrize("case", sorted(ENCODER_CASES))
def test_whole_encoder_at_roberta_large_geometry_against_fp32(encoders, case, monkeypatch):
    ref, stock, fused = encoders
    dev = torch.device("cuda:0")
    B, S, lens = ENCODER_CASES[case]
    g = torch.Generator(device=dev).manual_seed(11)
    ids = torch.randint(3, 50265, (B, S), generator=g, device=dev)
    ids[:, 0] = 0
    mask = torch.zeros(B, S, device=dev)
    for i, n in enumerate(lens):
        mask[i, :n] = 1
    ids[mask == 0] = 1                                          # padded positions: id 1, so their position ids hit padding_idx 1 too
    ids[1, 5:9] = 7                                             # a repeated word
    dy = torch.randn(B, S, E, generator=g, device=dev)
    outs = []
    n = None
    for m in (ref, stock, fused):
        for p in m.parameters():
            p.grad = None
        if m is fused:
            n = _counters(monkeypatch)
        y = m(ids, mask.to(torch.float32)).last_hidden_state
        y.backward(dy.to(y.dtype))
        outs.append((y.detach().float(), {k: p.grad.detach().float() for k, p in m.named_parameters() if p.grad is not None}))
        monkeypatch.undo()
    assert n == {"PlmSelfAttnFn": 2, "PlmFfnFn": 2, "PlmEmbeddingFn": 3}, n      # per layer one attention + one FFN; one call per table
    (yr, gr), (ys, gs), (yf, gf) = outs
    assert set(gr) == set(gs) == set(gf)
    ratios = {}
    for k, r in [("last_hidden_state", yr)] + sorted(gr.items()):
        if k.endswith("key.bias"):                              # mathematically zero: rounding noise on every side
            continue
        s, f = (ys, yf) if k == "last_hidden_state" else (gs[k], gf[k])
        rs = _rel(s, r)
        rf = _check_close(k, f, r, FACTOR * rs + SLACK, 4e-2)
        ratios[k] = (rf, rs)
    worst = max(ratios, key=lambda k: ratios[k][0] / (ratios[k][1] + 1e-9))
    print(f"\n{case}: worst fused / stock relative L2 {worst}: {ratios[worst][0]:.3e} / {ratios[worst][1]:.3e}; "
          f"median ratio {sorted(a / (b + 1e-9) for a, b in ratios.values())[len(ratios) // 2]:.3f}")
    # the embedding tables' padding rows and every row no token names: exactly zero
    pos = torch.cumsum((ids != 1).int(), 1) * (ids != 1).int() + 1          # RoBERTa's position ids: padding_idx for padded tokens
    for table, used in (("embeddings.word_embeddings.weight", ids), ("embeddings.position_embeddings.weight", pos)):
        gw = gf[table]
        assert (gw[1] == 0).all(), table
        named = torch.zeros(gw.shape[0], dtype=torch.bool, device=dev)
        named[used.reshape(-1)] = True
        named[1] = False
        assert (gw[~named] == 0).all(), table
        assert (gw[named].abs().sum(1) > 0).all(), table


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the fused nodes at the benchmark shape, dropout on
# ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,lens", [(512, (400, 512, 2, 449)), (130, (130, 77, 64, 129))])
def test_attention_core_with_dropout_at_the_benchmark_shape(S, lens):
    """ops.PlmSelfAttnFn with p = 0.1, 16 heads x 64, key padding with partly and fully masked key tiles: the keep-mask is read back with one probe
    launch per 64-key block (q = k = 0, no bias: every probability is 1 / S; values one-hot on that block's keys), its kept fraction is 1 - p; forward
    and the seven gradients against fp32 torch on that mask with the key bias applied."""
    from facialmmt_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(21)
    B, H, D, p = len(lens), NH, 64, 0.1
    seed = torch.tensor([0x5eed1234], device=dev, dtype=torch.int64)
    keep = torch.zeros(B, H, S, S, dtype=torch.bool, device=dev)               # (batch, head, query, key)
    for j in range(0, S, 64):
        w = min(64, S - j)
        probe = torch.zeros(B, S, 3 * E, device=dev, dtype=torch.bfloat16)
        one_hot = torch.zeros(S, D, device=dev, dtype=torch.bfloat16)
        one_hot[j:j + w, :w] = torch.eye(w, device=dev, dtype=torch.bfloat16)
        probe[..., 2 * E:] = one_hot.repeat(1, H)[None]
        o, _ = ops.mha_packed_bm_fwd_raw(probe, H, 0.125, p, 0, seed, None)
        o = o.view(B, S, H, D).permute(0, 2, 1, 3)[..., :w]
        assert ((o == 0) | (o.float() - _drop_inv(p) / S).abs().le(2e-2 / S)).all(), j      # 0 or inv / S, nothing else
        keep[..., j:j + w] = o != 0
    frac = keep.float().mean().item()
    assert abs(frac - (1 - p)) < 0.005, frac
    x = torch.randn(B, S, E, device=dev).to(torch.bfloat16)
    w = (torch.randn(3 * E, E, device=dev) * E ** -0.5).to(torch.bfloat16)
    b = (0.1 * torch.randn(3 * E, device=dev)).to(torch.bfloat16)
    kb = torch.zeros(B, S, device=dev)
    for i, n in enumerate(lens):
        kb[i, n:] = -30000.0
    dy = torch.randn(B, S, E, device=dev).to(torch.bfloat16)
    xin = x.clone().requires_grad_(True)
    ws = [w[i * E:(i + 1) * E].clone().requires_grad_(True) for i in range(3)]
    bs = [b[i * E:(i + 1) * E].clone().requires_grad_(True) for i in range(3)]
    y = ops.PlmSelfAttnFn.apply(xin, *ws, *bs, w, b, H, 0.125, p, seed, kb)
    grads = torch.autograd.grad(y, [xin] + ws + bs, dy)
    xr = x.float().requires_grad_(True)
    wr, br = w.float().requires_grad_(True), b.float().requires_grad_(True)
    qkv = torch.nn.functional.linear(xr, wr, br).view(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    sc = qkv[0] @ qkv[1].transpose(-1, -2) * 0.125 + kb[:, None, None, :]
    pr = torch.softmax(sc, dim=-1) * keep.float() * _drop_inv(p)
    yr = (pr @ qkv[2]).transpose(1, 2).reshape(B, S, E)
    gx, gw, gb = torch.autograd.grad(yr, [xr, wr, br], dy.float())
    _check_close("y", y, yr, 1e-2, 3e-2)
    refs = [gx] + [gw[i * E:(i + 1) * E] for i in range(3)] + [gb[i * E:(i + 1) * E] for i in range(3)]
    for a, r_, name in zip(grads, refs, ("dx", "dWq", "dWk", "dWv", "dbq", "dbk", "dbv")):
        if name == "dbk":                                                      # mathematically zero
            continue
        _check_close(name, a, r_, 2e-2, 4e-2)


def test_ffn_node_with_dropout_at_the_benchmark_shape():
    """ops.PlmFfnFn (the RoBERTa-large feed-forward half, 4 x 512 tokens, p = 0.1): the keep-mask read back by the fmmt_plm_dropadd_ln_fwd ones / zeros
    probe at the same (M, C, seed, salt); forward and the gradients of x, W1, b1, W2, b2, gamma, beta against fp32 torch on that mask."""
    from facialmmt_amd import _lib, ops
    dev = torch.device("cuda:0")
    torch.manual_seed(22)
    B, S, p, eps, salt = 4, 512, 0.1, 1e-5, 3 << 40
    M = B * S
    seed = torch.tensor([987654321], device=dev, dtype=torch.int64)
    x = torch.randn(B, S, E, device=dev).to(torch.bfloat16)
    w1 = (torch.randn(FF, E, device=dev) * E ** -0.5).to(torch.bfloat16)
    b1 = (0.1 * torch.randn(FF, device=dev)).to(torch.bfloat16)
    w2 = (torch.randn(E, FF, device=dev) * FF ** -0.5).to(torch.bfloat16)
    b2 = (0.1 * torch.randn(E, device=dev)).to(torch.bfloat16)
    gm = (1 + 0.1 * torch.randn(E, device=dev)).to(torch.bfloat16)
    bt = (0.1 * torch.randn(E, device=dev)).to(torch.bfloat16)
    ones, zeros = torch.ones(M, E, device=dev, dtype=torch.bfloat16), torch.zeros(M, E, device=dev, dtype=torch.bfloat16)
    probe, junk = torch.empty_like(ones), torch.empty_like(ones)
    _lib.check(_lib.load().fmmt_plm_dropadd_ln_fwd(M, E, eps, ones.data_ptr(), zeros.data_ptr(), gm.data_ptr(), bt.data_ptr(), p, 0, seed.data_ptr(), salt,
                                                   probe.data_ptr(), junk.data_ptr(), torch.cuda.current_stream().cuda_stream), "probe")
    keep = (probe != 0).view(B, S, E)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.005
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2, gm, bt)]
    y = ops.PlmFfnFn.apply(*leaves[:5], leaves[5], leaves[6], eps, p, seed, salt)
    y_again = ops.PlmFfnFn.apply(x, w1, b1, w2, b2, gm, bt, eps, p, seed, salt)
    assert torch.equal(y, y_again)
    dy = torch.randn(B, S, E, device=dev).to(torch.bfloat16)
    grads = torch.autograd.grad(y, leaves, dy)
    rl = [t.float().requires_grad_(True) for t in (x, w1, b1, w2, b2, gm, bt)]
    h = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(rl[0], rl[1], rl[2])), rl[3], rl[4])
    yr = torch.nn.functional.layer_norm(h * keep.float() * _drop_inv(p) + rl[0], (E,), rl[5], rl[6], eps)
    refs = torch.autograd.grad(yr, rl, dy.float())
    _check_close("y", y, yr, 1e-2, 3e-2)
    for a, r_, name in zip(grads, refs, ("dx", "dW1", "db1", "dW2", "db2", "dgamma", "dbeta")):
        _check_close(name, a, r_, 2e-2, 4e-2)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the embedding weight gradient over its whole promised range
# ------------------------------------------------------------------------------------------------------------------------------------

def _embedding_case(dev, V, C, T, pad, positions=False):
    from facialmmt_amd import ops
    if positions:
        ids = (torch.arange(T, device=dev) % 512) + 2                           # every id T / 512 times
    else:
        ids = torch.randint(0, V, (T,), device=dev)
        if V > 8:
            ids[::20] = 2                                                       # a separator every 20 tokens
            ids[5:9] = pad if pad is not None else 3
    ids = ids.view(4, -1) if T % 4 == 0 else ids.view(1, -1)
    w = torch.randn(V, C, device=dev).to(torch.bfloat16).requires_grad_(True)
    dy = torch.randn(*ids.shape, C, device=dev).to(torch.bfloat16)
    (g,) = torch.autograd.grad(ops.PlmEmbeddingFn.apply(ids, w, pad), w, dy)
    wr = w.detach().float().requires_grad_(True)
    (gr,) = torch.autograd.grad(torch.nn.functional.embedding(ids, wr, pad), wr, dy.float())
    assert (g.float() - gr).abs().max().item() <= 8e-3 * gr.abs().max().item() + 1e-6, (V, C, T)
    assert ((g.float() != 0) & (gr == 0)).sum().item() == 0, (V, C, T)          # rows no token names stay zero
    if pad is not None:
        assert (g[pad] == 0).all()


def test_embedding_weight_gradient_over_the_whole_index_range():
    """fmmt_embedding_bwd (ops.PlmEmbeddingFn) against torch's fp32 embedding backward up to T = 32768 indices, the limit of include/fmmt.h and of the
    Python guard: both sides of T = 15888, where the kernel's bitmap + list pass 64 KiB of LDS; a small T first, so that a limit set once from the first
    call's need would fail the large ones."""
    dev = torch.device("cuda:0")
    torch.manual_seed(6)
    _embedding_case(dev, 50265, 1024, 1000, 1)
    for T in (15887, 15888, 20000, 32768):
        _embedding_case(dev, 50265, 1024, T, 1)
    _embedding_case(dev, 514, 1024, 32768, 1, positions=True)
    _embedding_case(dev, 1, 1024, 32768, None)                                   # the predicated column-sum kernel
    _embedding_case(dev, 2, 1024, 32768, None)


def test_embedding_weight_gradient_beyond_the_limit(monkeypatch):
    """T = 32769: the C entry point answers FMMT_EINVAL; a fused nn.Embedding takes torch's own path for that many indices (and the fused one at
    32768), with the same gradient as torch."""
    from facialmmt_amd import _lib, ops
    from facialmmt_amd.train_step import fuse_text_encoder
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    T, V, C = 32769, 16, 8
    ids = torch.randint(0, V, (T,), device=dev)
    dy = torch.randn(T, C, device=dev).to(torch.bfloat16)
    dw = torch.zeros(V, C, device=dev, dtype=torch.bfloat16)
    rc = _lib.load().fmmt_embedding_bwd(T, C, V, ids.data_ptr(), -1, dy.data_ptr(), dw.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.FMMT_EINVAL
    emb = torch.nn.Embedding(50265, 1024, padding_idx=1).to(dev).to(torch.bfloat16)
    fuse_text_encoder(emb)
    calls = []
    real = ops.PlmEmbeddingFn.apply
    monkeypatch.setattr(ops.PlmEmbeddingFn, "apply", lambda *a: (calls.append(a[0].numel()), real(*a))[1])
    for T in (32769, 32768):
        ids = torch.randint(0, 50265, (1, T), device=dev)
        ids[0, :50] = 1
        dy = torch.randn(1, T, 1024, device=dev).to(torch.bfloat16)
        (g,) = torch.autograd.grad(emb(ids), emb.weight, dy)
        wr = emb.weight.detach().float().requires_grad_(True)
        (gr,) = torch.autograd.grad(torch.nn.functional.embedding(ids, wr, 1), wr, dy.float())
        assert (g.float() - gr).abs().max().item() <= 8e-3 * gr.abs().max().item() + 1e-6, T
        assert (g[1] == 0).all()
    assert calls == [32768]


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. masks that are not per-key are not reduced to one
# ------------------------------------------------------------------------------------------------------------------------------------

def _packing_mask(B, S, dev):
    cuts = [(0, 40, 96), (0, 30, 70, 96)]
    m = torch.zeros(B, 1, S, S, dtype=torch.bool, device=dev)
    for i in range(B):
        c = cuts[i % len(cuts)]
        for a, b in zip(c[:-1], c[1:]):
            m[i, 0, a:b, a:b] = True
    return m


@pytest.fixture(scope="module")
def small_pair():
    dev = torch.device("cuda:0")
    stock = _roberta(dev, vocab=1000).to(torch.bfloat16).train()
    fused = copy.deepcopy(stock)
    assert _fuse(fused) == (4, 2)
    return stock, fused


@pytest.mark.parametrize("kind", ["packing_bool", "packing_additive", "causal", "padding_2d", "padding_2d_transposed"])
def test_masks_that_are_not_per_key_take_the_stock_attention(small_pair, kind, monkeypatch):
    """a (B, 1, S, S) mask from the caller -- block-diagonal sequence packing, boolean or additive, or causal -- reaches the layers unchanged and must not
    become a per-key bias from its first query row: the fused encoder matches the stock one without calling the fused attention core.  A (B, S) padding
    mask still takes it, also one laid out transposed (a view of a time-major (S, B) buffer: the kernels read the per-key bias row-major)."""
    stock, fused = small_pair
    dev = torch.device("cuda:0")
    B, S = 2, 96
    g = torch.Generator(device=dev).manual_seed(5)
    ids = torch.randint(3, 1000, (B, S), generator=g, device=dev)
    if kind.startswith("padding_2d"):
        mask = torch.ones(B, S, device=dev, dtype=torch.long)
        mask[0, 85:] = 0
        mask[1, 70:] = 0
        if kind == "padding_2d_transposed":
            mask = mask.t().contiguous().t()
            assert mask.stride() == (1, B)
    elif kind == "causal":
        mask = torch.ones(S, S, dtype=torch.bool, device=dev).tril().expand(B, 1, S, S).contiguous()
    else:
        mask = _packing_mask(B, S, dev)
        if kind == "packing_additive":
            mask = torch.where(mask, 0.0, -1e9).to(torch.bfloat16)
    dy = torch.randn(B, S, E, generator=g, device=dev).to(torch.bfloat16)
    outs = []
    n = None
    for m in (stock, fused):
        for p in m.parameters():
            p.grad = None
        if m is fused:
            n = _counters(monkeypatch)
        y = m(input_ids=ids, attention_mask=mask).last_hidden_state
        y.backward(dy)
        outs.append((y.detach().float(), {k: p.grad.detach().float() for k, p in m.named_parameters() if p.grad is not None}))
        monkeypatch.undo()
    (y0, g0), (y1, g1) = outs
    assert (y0 - y1).abs().max().item() <= 3e-2 * max(1.0, y0.abs().max().item()), (y0 - y1).abs().max().item()
    assert set(g0) == set(g1)
    for k in g0:
        if k.endswith("key.bias"):
            continue
        scale = g0[k].abs().max().item() + 1e-6
        assert (g0[k] - g1[k]).abs().max().item() <= 4e-2 * scale, (k, (g0[k] - g1[k]).abs().max().item(), scale)
    assert n["PlmSelfAttnFn"] == (2 if kind.startswith("padding_2d") else 0), n
    assert n["PlmFfnFn"] == 2


def test_encoder_reached_without_the_models_hook_takes_the_stock_attention(small_pair, monkeypatch):
    """the mask record lives for one forward of the whole model: the encoder stack called on its own (no record) takes the stock attention, also
    right after a forward of the model"""
    stock, fused = small_pair
    dev = torch.device("cuda:0")
    n = _counters(monkeypatch)
    ids = torch.randint(3, 1000, (2, 64), device=dev)
    fused(input_ids=ids)
    assert n["PlmSelfAttnFn"] == 2
    h = torch.randn(2, 64, E, device=dev).to(torch.bfloat16)
    y = fused.encoder(h, attention_mask=torch.ones(2, 1, 64, 64, dtype=torch.bool, device=dev).tril())
    y = y[0] if isinstance(y, tuple) else y.last_hidden_state
    assert n["PlmSelfAttnFn"] == 2 and torch.isfinite(y.float()).all()


def test_gradient_checkpointing_keeps_the_stock_attention(small_pair, monkeypatch):
    """with activation checkpointing the layers re-run in the backward, after the model's forward cleared its mask record: the encoder then takes the
    stock attention in the forward as well (the recomputation must rebuild the same graph), and matches the stock module"""
    stock, fused = small_pair
    dev = torch.device("cuda:0")
    ckpt = copy.deepcopy(stock)
    assert _fuse(ckpt) == (4, 2)
    ckpt.gradient_checkpointing_enable()
    assert ckpt.is_gradient_checkpointing
    ids = torch.randint(3, 1000, (2, 64), device=dev)
    mask = torch.ones(2, 64, device=dev, dtype=torch.long)
    mask[1, 40:] = 0
    dy = torch.randn(2, 64, E, device=dev).to(torch.bfloat16)
    outs = []
    n = None
    for m in (stock, ckpt):
        for p in m.parameters():
            p.grad = None
        if m is ckpt:
            n = _counters(monkeypatch)
        y = m(input_ids=ids, attention_mask=mask).last_hidden_state
        y.backward(dy)
        outs.append((y.detach().float(), {k: p.grad.detach().float() for k, p in m.named_parameters() if p.grad is not None}))
        monkeypatch.undo()
    assert n["PlmSelfAttnFn"] == 0, n
    (y0, g0), (y1, g1) = outs
    assert (y0 - y1).abs().max().item() <= 3e-2 * max(1.0, y0.abs().max().item())
    assert set(g0) == set(g1)
    for k in g0:
        if k.endswith("key.bias"):
            continue
        scale = g0[k].abs().max().item() + 1e-6
        assert (g0[k] - g1[k]).abs().max().item() <= 4e-2 * scale, (k, (g0[k] - g1[k]).abs().max().item(), scale)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. a chunked feed-forward draws a fresh dropout mask per chunk
# ------------------------------------------------------------------------------------------------------------------------------------

def test_chunked_feed_forward_draws_a_mask_per_chunk():
    """config.chunk_size_feed_forward = S / 2: transformers calls feed_forward_chunk once per half of the sequence.  On an input whose halves are equal
    (attention without dropout keeps them equal) the output halves are equal with p = 0 and differ with p = 0.1; with p = 0 the layer matches the
    stock one."""
    dev = torch.device("cuda:0")
    B, S = 2, 128
    stock = _roberta(dev, vocab=1000, layers=1, chunk_size_feed_forward=S // 2).to(torch.bfloat16).train()
    fused = copy.deepcopy(stock)
    assert _fuse(fused) == (2, 1)
    layer, slayer = fused.encoder.layer[0], stock.encoder.layer[0]
    assert layer.chunk_size_feed_forward == S // 2
    box = layer.output._fmmt_seed
    torch.manual_seed(9)
    half = torch.randn(B, S // 2, E, device=dev).to(torch.bfloat16)
    x = torch.cat([half, half], 1)

    def run(mod, p):
        mod.output.dropout.p = p
        box.draw(dev)                                           # what the model's pre-hook does before a training forward
        with torch.enable_grad():
            y = mod(x.clone().requires_grad_(True))
        return (y[0] if isinstance(y, tuple) else y).float()

    y0 = run(layer, 0.0)
    assert _rel(y0[:, :S // 2], y0[:, S // 2:]) < 1e-2
    y1 = run(layer, 0.1)
    assert _rel(y1[:, :S // 2], y1[:, S // 2:]) > 0.05, _rel(y1[:, :S // 2], y1[:, S // 2:])
    ys = run(slayer, 0.0)
    assert (y0 - ys).abs().max().item() <= 3e-2 * max(1.0, ys.abs().max().item())
