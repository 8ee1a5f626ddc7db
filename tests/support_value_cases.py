"""Hard input VALUES for the normalisation, softmax and GELU kernels: generators, fp64 references, the class-local metric and the yardstick that
tests/test_value_cases_cpu.py (no GPU: the right restatement passes, each wrong one is flagged) and tests/test_gpu_value_edges.py (the kernels) share.
Importable without a GPU.

Why.  Every other parity test draws unit normals, where a one-pass variance, a softmax that drops or mis-rescales its running max, or an `eps`
outside the square root is as good as the right thing.  The classes below are the inputs on which they are not.

Rows of a normalisation input (`norm_rows`), interleaved so that every wave and lane position sees every class:
    unit      z                                  the control
    offset    1000 + z (fp32); drawn from {1024, 1032, 1040} (bf16: the representable grid there): |mean| >> std, E[x^2] - E[x]^2 cancels
    outlier   z with two channels per row times +-300 (at least 300 in magnitude), at channel 0, C - 1 and moving positions
    tiny      1e-3 z: variance 1e-6 < eps, so where eps is added matters
    const0 / const1024   every element equal: variance 0
    big       1e15 z: squares reach 1e31, their sum over 1536 channels still fits fp32

Scores of an attention input (`mha_inputs`, `KEY_BIAS_KINDS`): `sharp` (logit std 30), `shift+` / `shift-` (every logit of a row near +-500, spread O(1):
inf / inf or 0 / 0 without max subtraction), and key_bias variants: -10000 on trailing keys (whole 64-key tiles included), -inf on the leading 8 / 64 / 70
keys, on scattered keys, on all keys but one, and finfo.min in place of -inf.  A batch element whose keys are ALL at -inf is outside the contract
(include/fmmt.h) and is not generated.

Metric (`class_errors`): per class, max|got - ref| over that class's elements divided by max|ref| over the SAME elements -- the global max|ref| that
support_op_cases.report() divides by lets an outlier channel or a `big` row hide any error elsewhere.  The outlier class is split into its outlier
channels and its ordinary ones.

Yardstick (`bound`): ref is the fp64 restatement on the same, already rounded, inputs; a case passes at max(base, K * stock) where `base` is the tolerance
the op's existing test holds it to and `stock` is the same metric of the stock torch composition of the op in the same element type on the same inputs
(several of these classes cost accuracy in ANY fp32 / bf16 implementation: the fp32 mean of 1000 + z is already off by 1e-4 sigma).  Constant rows have a
derived bound instead (`const_row_bound`)."""
import math

import torch

# The yardstick's factor: the smallest power of two that clears every honest kernel with a factor 2 to spare.  Measured on an MI355X over the 1380
# judged figures of tests/test_gpu_value_edges.py; per family, the largest got / stock among the figures above `base` (K decides nothing below it):
#     batch_norm_1d   bf16 1.85 (n=2 train, dx of `big`)    fp32 1.23 (n=2 train, y of offset)
#     mha_core        fp32 1.33 (70x130, dq on shift+)      bf16 0.22;  batch-major 0.19, ragged 0.26 (dq on shift+-);  avg_weights: none above base
#     layer_norm      fp32 0.90 (C=768, y of offset), merge 0.81, residual 0.16;  bf16: none above base
#     mlp_ln          fp32 0.38, bf16 1.00;  window_block bf16 1.00, fp32 none (bf16 y - x of an offset row IS the output's rounding, kernel and stock alike)
#     window_attn     bf16 0.57 (dqkv, sharp, shifted), fp32 none;  patch_proj_ln fp32 0.46, patch_embed_u8_ln fp32 0.48, bf16 none
#     dropadd_ln, Plm tail / ffn / layer_norm, ce_loss, emotion_head, pool_head: none above base
# so K = 4 (2 x 1.85 = 3.7).  tests/test_value_cases_cpu.py holds the other side: each deliberately wrong restatement misses max(base, K * stock) by
# >= 10x (the closest: 15x, a row-scaled intermediate in the ordinary channels of an outlier row; the one-pass variance misses by 340x or more).
K = 4.0

NORM_CLASSES = ("unit", "offset", "outlier", "tiny", "const0", "const1024", "big")
CONST_CLASSES = {"const0": 0.0, "const1024": 1024.0}
BF16_OFFSET_GRID = (1024.0, 1032.0, 1040.0)
OUTLIER_GAIN = 300.0
LN_CHANNELS = (96, 192, 384, 768, 1536)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def randn(shape, seed):
    return torch.randn(shape, generator=_gen(seed), dtype=torch.float32)


def outlier_channels(k, C):
    """the two outlier channels of the k-th outlier row: (0, C - 1) first, then moving positions; always distinct"""
    if k == 0:
        return 0, C - 1
    if k == 1:
        return C - 1, C // 2
    a = (k * 53) % C
    b = (a + C // 3 + k) % C
    return a, (b if b != a else (a + 1) % C)


def norm_rows(M, C, dtype, seed=0, classes=NORM_CLASSES):
    """-> (x (M, C) `dtype` on the CPU, class_of_row (M,) int64 index into `classes`, outlier_mask (M, C) bool).  Row r has class r % len(classes)."""
    z = randn((M, C), seed)
    cls = torch.arange(M) % len(classes)
    x = z.clone()
    omask = torch.zeros((M, C), dtype=torch.bool)
    count = {}
    for r in range(M):
        name = classes[int(cls[r])]
        k = count.get(name, 0)
        count[name] = k + 1
        if name == "offset":
            if dtype == torch.bfloat16:
                pick = torch.randint(0, len(BF16_OFFSET_GRID), (C,), generator=_gen(seed * 1000 + r))
                x[r] = torch.tensor(BF16_OFFSET_GRID)[pick]
                x[r, 0], x[r, -1] = BF16_OFFSET_GRID[0], BF16_OFFSET_GRID[-1]      # never a constant row: that is another class
            else:
                x[r] = 1000.0 + z[r]
        elif name == "outlier":
            a, b = outlier_channels(k, C)
            for ch, gain in ((a, OUTLIER_GAIN), (b, -OUTLIER_GAIN)):      # |z| raised to 1 there: every row of the class has its outliers
                x[r, ch] = gain * torch.sign(z[r, ch]) * z[r, ch].abs().clamp_min(1.0)
            omask[r, a] = omask[r, b] = True
        elif name == "tiny":
            x[r] = 1e-3 * z[r]
        elif name in CONST_CLASSES:
            x[r] = CONST_CLASSES[name]
        elif name == "big":
            x[r] = 1e15 * z[r]
        else:
            assert name == "unit", name
    return x.to(dtype), cls, omask


def const_row_bound(gamma, c, eps):
    """|y - beta| on a row whose elements all equal c: the worst that rounding 1 / C can do to the mean is |c| 2^-22 relative... times rstd <= 1 / sqrt(eps),
    times the largest |gamma|.  Exactly 0 for c = 0, and for a power-of-two C (1 / C is exact)."""
    return float(gamma.abs().max()) * abs(c) * 2.0 ** -22 / math.sqrt(eps)


# ------------------------------------------------------------------------------------------------------------------------ references (fp64)
def layer_norm64(x, gamma, beta, eps=1e-5):
    """oracle/swin.py layer_norm on fp64 copies of the (already rounded) operands; gradients flow to whatever requires them"""
    from oracle import swin as OS
    return OS.layer_norm(x, gamma, beta, eps)


def heads(t, nh):
    """(L, B, E) -> (B, nh, L, hd)"""
    L, B, E = t.shape
    return t.reshape(L, B, nh, E // nh).permute(1, 2, 0, 3)


def attention(q, k, v, nh, scale, key_bias=None):
    """softmax(scale q k^T + key_bias) v per (batch element, head) in the operands' own type and on their device: fp64 operands give the reference,
    fp32 / bf16 ones the stock composition.  q (Lq, B, E), k / v (Lk, B, E), key_bias (B, Lk) or None -> (Lq, B, E)"""
    Lq, B, E = q.shape
    s = (heads(q, nh) * scale) @ heads(k, nh).transpose(-1, -2)
    if key_bias is not None:
        s = s + key_bias.to(s.dtype)[:, None, None, :]
    return (torch.softmax(s, -1) @ heads(v, nh)).permute(2, 0, 1, 3).reshape(Lq, B, E)


# ------------------------------------------------------------------------------------------------------------------------ attention inputs
SCORE_KINDS = ("unit", "sharp", "shift+", "shift-")
KEY_BIAS_KINDS = ("tail-10000", "lead8", "lead64", "lead70", "scatter", "one", "fmin")
SHIFT = 500.0


def mha_inputs(kind, Lq, Lk, B, E, nh, dtype, seed=0):
    """-> q (Lq, B, E), k, v (Lk, B, E) in `dtype` on the CPU; the logits are scale * q . k per head with scale = hd^-0.5.
    sharp: q and k times sqrt(30), logit std 30.
    shift+-: with u the unit vector along (1, .., 1) of a head, k = z_k + SHIFT u and q = (z_q minus its u component) +- sqrt(hd) u, so that
    scale q . k = +-SHIFT + scale (z_q' . z_k) +- (z_k . u): every logit of a row within a few units of +-500."""
    hd = E // nh
    q, k, v = randn((Lq, B, E), seed + 1), randn((Lk, B, E), seed + 2), randn((Lk, B, E), seed + 3)
    if kind == "sharp":
        q, k = q * math.sqrt(30.0), k * math.sqrt(30.0)
    elif kind in ("shift+", "shift-"):
        sign = 1.0 if kind == "shift+" else -1.0
        u = torch.full((hd,), hd ** -0.5)
        qh = q.reshape(Lq, B, nh, hd)
        qh = qh - (qh @ u)[..., None] * u + sign * math.sqrt(hd) * u
        q = qh.reshape(Lq, B, E)
        k = (k.reshape(Lk, B, nh, hd) + SHIFT * u).reshape(Lk, B, E)
    else:
        assert kind == "unit", kind
    return q.to(dtype), k.to(dtype), v.to(dtype)


def key_bias(kind, B, Lk, seed=0):
    """-> (B, Lk) fp32.  Batch element 0 carries the named pattern in its plain form; the others a variation of it on top of a smooth O(1) bias, so
    that a pattern and the general case share a launch.  `one_key` (below) names the surviving key of kind "one"."""
    kb = randn((B, Lk), seed + 7) * 0.5
    kb[0] = 0.0
    ninf = float("-inf")
    for b in range(B):
        if kind == "tail-10000":
            kb[b, max(1, Lk - (70 if b == 0 else 3 + b)):] = -10000.0          # Lk = 130: keys 60.. -- the whole tile [64, 128) and both partial ones
        elif kind in ("lead8", "lead64", "lead70", "fmin"):
            n = {"lead8": 8, "lead64": 64, "lead70": 70, "fmin": 70}[kind]
            n = min(n + (b if b else 0), Lk - 1)
            kb[b, :n] = torch.finfo(torch.float32).min if kind == "fmin" else ninf
        elif kind == "scatter":
            idx = torch.arange(Lk)
            kb[b, (idx * (b + 2) + b) % 3 == 0] = ninf
            kb[b, Lk // 2] = 0.25                                              # at least one key stays
        elif kind == "one":
            keep = one_key(b, Lk)
            row = torch.full((Lk,), ninf)
            row[keep] = kb[b, keep]
            kb[b] = row
        else:
            raise ValueError(kind)
    assert bool(torch.isfinite(kb).any(dim=1).all()), "a batch element with every key at -inf is outside the contract"
    return kb


def one_key(b, Lk):
    return (Lk - 1, 5, Lk // 2, 0)[b % 4] % Lk


# ------------------------------------------------------------------------------------------------------------------------ logits of the loss heads
LOGIT_KINDS = ("unit", "pm1e4", "ahead100", "equal")


def logits(kind, B, NL, seed=0):
    """(B, NL) fp32 logits and (B,) labels: unit normals; +-1e4; one class ahead by 100 (the label's, or another one, alternating); all classes equal"""
    x = randn((B, NL), seed + 11)
    y = torch.randint(0, NL, (B,), generator=_gen(seed + 12))
    if kind == "pm1e4":
        x = torch.where(x > 0, torch.full_like(x, 1e4), torch.full_like(x, -1e4)) + x
    elif kind == "ahead100":
        lead = (y + torch.arange(B) % 2) % NL
        x[torch.arange(B), lead] += 100.0
    elif kind == "equal":
        x = torch.full((B, NL), 3.0)
    else:
        assert kind == "unit", kind
    return x, y


# ------------------------------------------------------------------------------------------------------------------------ metric and yardstick
def rel_err(got, ref, mask=None):
    """max|got - ref| / max|ref| over the elements `mask` selects (all without one); a non-finite `got` gives inf.  Where the reference is exactly 0
    over the selection the error is returned absolute (nothing to scale by)."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    if mask is not None:
        g, r = g[mask], r[mask]
    if g.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    err, scale = float((g - r).abs().max()), float(r.abs().max())
    return err / scale if scale > 0.0 else err


def class_masks(cls, classes, omask=None):
    """name -> (M,) or (M, C) bool mask; the outlier class is split into `outlier/ch` (its outlier channels) and `outlier/rest`"""
    out = {}
    for i, name in enumerate(classes):
        rows = cls == i
        if not bool(rows.any()):
            continue
        if name == "outlier" and omask is not None:
            out["outlier/ch"] = omask & rows[:, None]
            out["outlier/rest"] = (~omask) & rows[:, None]
        else:
            out[name] = rows[:, None].expand(-1, omask.shape[1]) if omask is not None else rows
    return out


def class_errors(got, ref, cls, classes, omask=None, skip=()):
    """per class: rel_err over that class's elements (row-wise tensors (M, C))"""
    return {name: rel_err(got, ref, m) for name, m in class_masks(cls, classes, omask).items() if name not in skip}


def global_errors(got, ref, cls, classes, omask=None, skip=()):
    """the metric this module replaces: the same per-class max|err|, over the GLOBAL max|ref| (what support_op_cases.report() judges)"""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(r.abs().max())
    return {name: float((g[m] - r[m]).abs().max()) / scale for name, m in class_masks(cls, classes, omask).items() if name not in skip}


def bound(base, stock):
    return max(base, K * stock)


TABLE = []          # (case, class / output, got, stock, bound): every judged figure of a run, printed by the tests


def judge(case, got_errs, stock_errs, base, failures):
    """got_errs / stock_errs: dicts from class_errors (or {output name: rel_err}); appends to `failures` what misses max(base, K * stock)"""
    for name, e in got_errs.items():
        s = stock_errs[name]
        bar = bound(base, s)
        TABLE.append((case, name, e, s, bar))
        ratio = e / s if s > 0 else float("inf") if e > 0 else 0.0
        print(f"{'ok  ' if e <= bar else 'MISS'} {case:52s} {name:13s} got={e:.3e} stock={s:.3e} got/stock={ratio:8.3g} bound={bar:.3e} (base {base:g})", flush=True)
        if not e <= bar:
            failures.append(f"{case} [{name}]: {e:.3e} > max(base {base:g}, {K:g} x stock {s:.3e})")
