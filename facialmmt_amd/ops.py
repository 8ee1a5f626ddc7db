"""Host side of the C ABI: torch.autograd.Functions whose forward/backward are calls into
libfmmt_hip.so through ctypes (facialmmt_amd/_lib.py).  PyTorch is used for what it is good at here
-- device memory (caching allocator), streams, autograd bookkeeping -- never for the arithmetic of
the hot path.  Every op raises if the library is missing or a launch fails (no fallback)."""
from __future__ import annotations

import math
import weakref

import torch
from torch.autograd import Function

from . import _lib
from ._lib import EPI_GELU, EPI_GELU_BWD, EPI_GELU_DG, EPI_MUL_AUX, EPI_NONE, SAVE_DG, check, dtype_code


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _c16(t: torch.Tensor) -> torch.Tensor:
    """contiguous AND 16-byte aligned: a view that starts at an odd offset of its storage (a residual sliced out of a packed buffer) is copied rather than
    handed to a kernel that would answer FMMT_EALIGN (round-5 ADVICE)"""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _need_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise _lib.FmmtError(f"{what}: the hot path runs on the GPU only (got a {t.device} tensor); "
                             f"the CPU restatement lives in oracle/ and is test infrastructure")


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _seed_args(seed):
    """a dropout seed as the entry points take it, (seed_i, seed_t): a python int, or a 1-element int64 CUDA tensor the kernel reads at run time
    (graph-replay safe) with 0 in the integer's place"""
    seed_t = seed if isinstance(seed, torch.Tensor) else None
    return (0 if seed_t is not None else int(seed)), seed_t


# ------------------------------------------------------------------------------------------------
# raw launch helpers (no autograd)
# ------------------------------------------------------------------------------------------------
def linear_raw(x2, w, bias, *, epi=EPI_NONE, y_pre=None, aux=None, res=None, rowscale=None, rows_per_scale=1):
    """y[M,N] = epi(x2[M,K] @ w[N,K]^T + bias) ; y = res + rowscale*y.  x2, w same dtype, contiguous."""
    M, K = x2.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=x2.dtype, device=x2.device)
    lib = _lib.load()
    if epi == EPI_NONE and res is None and rowscale is None and K >= 4096:
        nbytes = lib.fmmt_linear_splitk_workspace(M, N, K)
        if nbytes:                                       # skinny, very long K (embedding head): split-K kernel
            ws = _ws(nbytes, x2.device)
            rc = lib.fmmt_linear_fwd_splitk(dtype_code(x2.dtype), M, N, K, _p(x2), K, _p(w), K, _p(bias), _p(y), N,
                                            _p(ws), nbytes, _st())
            check(rc, f"fmmt_linear_fwd_splitk(M={M},N={N},K={K})")
            return y
    rc = lib.fmmt_linear_fwd(dtype_code(x2.dtype), M, N, K, _p(x2), K, _p(w), K, _p(bias), _p(y), N, _p(y_pre),
                             epi, _p(aux), N, _p(res), N, _p(rowscale), rows_per_scale, _st())
    check(rc, f"fmmt_linear_fwd(M={M},N={N},K={K})")
    return y


def wgrad_partials_raw(dy2, x2, want_bias, ws, nbytes, rowscale=None, rows_per_scale=1, x_gelu=False):
    """the split contraction of the weight gradient (one MFMA kernel launch) into fp32 partials in `ws`"""
    M, N = dy2.shape
    K = x2.shape[1]
    rc = _lib.load().fmmt_linear_wgrad_partials(dtype_code(dy2.dtype), M, N, K, _p(dy2), N, _p(x2), K, 1 if want_bias else 0,
                                                _p(rowscale), rows_per_scale, EPI_GELU if x_gelu else EPI_NONE, _p(ws), nbytes, _st())
    check(rc, f"fmmt_linear_wgrad_partials(M={M},N={N},K={K})")


def wgrad_raw(dy2, x2, want_bias, rowscale=None, rows_per_scale=1, x_gelu=False, out=None):
    """dw[N,K] fp32 = (s*dy2)^T @ x2 ; db[N] fp32 = colsum(s*dy2).  x_gelu: x2 holds a pre-activation, contract with gelu(x2)."""
    M, N = dy2.shape
    K = x2.shape[1]
    lib = _lib.load()
    if out is not None:                                  # contiguous fp32 destinations (row slices of a packed weight gradient)
        dw, db = out
        assert dw.shape == (N, K) and dw.dtype == torch.float32 and dw.is_contiguous() and (not want_bias or (db.shape == (N,) and db.is_contiguous()))
    else:
        dw = torch.empty((N, K), dtype=torch.float32, device=dy2.device)
        db = torch.empty((N,), dtype=torch.float32, device=dy2.device) if want_bias else None
    nbytes = lib.fmmt_linear_wgrad_workspace(dtype_code(dy2.dtype), M, N, K)
    ws = _ws(nbytes, dy2.device)
    if M <= 2048:
        # few-token problems: one entry point (single split -> the contraction kernel writes dw / db itself, no reduce launch;
        # 769..2048 tokens: one launch where linear_tn_few_kernel applies, partials + finish inside the library otherwise)
        rc = lib.fmmt_linear_wgrad(dtype_code(dy2.dtype), M, N, K, _p(dy2), N, _p(x2), K, _p(dw), _p(db), _p(rowscale), rows_per_scale,
                                   EPI_GELU if x_gelu else EPI_NONE, _p(ws), nbytes, _st())
        check(rc, f"fmmt_linear_wgrad(M={M},N={N},K={K})")
        return dw, db
    wgrad_partials_raw(dy2, x2, want_bias, ws, nbytes, rowscale, rows_per_scale, x_gelu)
    rc = lib.fmmt_linear_wgrad_finish(dtype_code(dy2.dtype), M, N, K, _p(dw), _p(db), _p(ws), nbytes, _st())
    check(rc, f"fmmt_linear_wgrad_finish(M={M},N={N},K={K})")
    return dw, db


_CAST_CACHE: dict = {}          # id(parameter) -> {(offset, shape, stride, dtype, transpose): (version, shadow)}


def _lp(w: torch.Tensor, dtype, transpose: bool = False) -> torch.Tensor:
    """Parameter in the activation dtype (fp32 master -> bf16 shadow in throughput mode), optionally
    transposed+contiguous (the input-gradient GEMM wants W^T row-major).  Shadows are cached per parameter OBJECT
    (for a view such as in_proj_weight[a:b]: its base) and version, and dropped when that object dies -- an
    address-based key would hand a new model the shadows of a freed one that happened to occupy the same memory.
    They are rebuilt only after an optimizer step touched the master copy.

    Operands: while a graph is captured outside a pinned_scope (every fp32 step, a bf16 one with PIN_SHADOWS off) the result is a FRESH tensor
    that nothing else keeps alive.  A caller that hands two of them to one launch must hold both in variables until the launch is enqueued:
    `_p(_lp(a)), _p(_lp(b))` frees the first before the second is allocated, the allocator gives the second the same block, and the kernel
    reads b through both pointers (found by tests/test_gpu_step_oracle.py: the captured fp32 auxiliary step's gradients below Swin stage 1)."""
    base = w._base if w._base is not None else w
    wd = w.detach()
    if wd.dtype == dtype and not transpose:
        return wd.contiguous()
    capturing = wd.is_cuda and torch.cuda.is_current_stream_capturing()
    key = (w.storage_offset(), tuple(w.shape), tuple(w.stride()), dtype, transpose)
    if capturing and _PIN_SCOPE:                            # only inside the capture of a step that refreshes them (pinned_scope)
        pin = _PINNED.get(id(base))
        if pin is not None and key in pin:
            return pin[key]                                  # refreshed by PinnedShadows.refresh() at the head of the graph
    sub = None if capturing else _CAST_CACHE.get(id(base))   # inside a hipGraph the cast must be part of the graph
    if sub is not None:
        hit = sub.get(key)
        if hit is not None and hit[0] == w._version:
            return hit[1]
    out = wd.to(dtype)
    out = out.t().contiguous() if transpose else out.contiguous()
    if capturing:
        return out
    if sub is None:
        sub = _CAST_CACHE[id(base)] = {}
        weakref.finalize(base, _CAST_CACHE.pop, id(base), None)
    sub[key] = (w._version, out)
    return out


_PINNED: dict = {}              # id(parameter) -> {key: static shadow}: consulted only while a graph is being captured
_PIN_SCOPE: list = []           # PinnedShadows objects whose owners are capturing right now (pinned_scope)


class pinned_scope:
    """`with pinned_scope(shadows):` around the capture of a step whose graph starts with shadows.refresh().  Only inside it does
    `_lp` hand out the static shadows: any other capture (graph_multimodal, a user's own graph) would otherwise bake in shadows that
    nothing in ITS graph refreshes -- stale weights after the first optimizer step."""

    def __init__(self, shadows):
        self.shadows = shadows

    def __enter__(self):
        if self.shadows is not None:
            _PIN_SCOPE.append(self.shadows)
        return self

    def __exit__(self, *exc):
        if self.shadows is not None:
            _PIN_SCOPE.remove(self.shadows)
        return False


class PinnedShadows:
    """Static bf16 shadows (W and W^T) of the parameters a captured training step reads, refreshed by ONE launch.

    Inside a HIP graph a shadow cannot come from the version-keyed cache (a replay does not bump versions), so every Linear
    re-cast -- and, for the input-gradient GEMM, re-transposed -- its weight inside the graph: ~250 cast and ~110 transpose
    launches of 4-9 us per step (2.2 ms of the step's 76).  Here the shadows every `_lp` call of the eager warm-up passes
    produced (the cache knows exactly which (view, dtype, transpose) combinations the step uses) become static tensors;
    while a graph is captured `_lp` hands them out without launching anything, and `refresh()` -- captured at the head of the
    graph -- rebuilds all of them from the current parameter values with fmmt_cast_batch.  Eager calls never see them."""

    def __init__(self, params):
        import numpy as np
        recs, self.keep = [], []
        tiles = 0
        for p in params:
            sub = _CAST_CACHE.get(id(p))
            if not sub or not p.is_cuda or p.dtype not in (torch.float32, torch.bfloat16):
                continue
            pins = _PINNED.setdefault(id(p), {})
            if not pins:
                weakref.finalize(p, _PINNED.pop, id(p), None)
            for key, (_, shadow) in sub.items():
                off, shape, stride, dtype, transpose = key
                if dtype != torch.bfloat16 or len(shape) != 2 or stride[1] != 1:
                    continue
                rows, cols = shape
                dst = pins.get(key)                          # shared with another captured step over the same parameters
                if dst is None:
                    dst = pins[key] = torch.empty_like(shadow)   # [rows, cols] or [cols, rows], contiguous
                self.keep.append((p, dst))
                tr, tc = (rows + 63) // 64, (cols + 63) // 64
                # `off` is the view's ABSOLUTE offset in the storage (a parameter may itself be a view of a flat buffer)
                recs.append((p.untyped_storage().data_ptr() + off * p.element_size(), dst.data_ptr(), rows, cols, stride[0],
                             (1 if transpose else 0) | (2 if p.dtype == torch.float32 else 0), tiles, tc))
                tiles += tr * tc
        self.n, self.tiles = len(recs), tiles
        self.desc = None
        if recs:
            arr = np.zeros(len(recs), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("ld", "<i4"),
                                                      ("flags", "<i4"), ("tb", "<i4"), ("tc", "<i4")]))
            for i, r in enumerate(recs):
                arr[i] = r
            self.desc = torch.from_numpy(arr.view(np.uint8).copy()).to(self.keep[0][1].device)

    def refresh(self):
        if self.desc is not None:
            check(_lib.load().fmmt_cast_batch(self.n, self.tiles, _p(self.desc), _st()), "fmmt_cast_batch")

    def release(self):
        for p, dst in self.keep:
            pins = _PINNED.get(id(p))
            if pins:
                for k in [k for k, v in pins.items() if v is dst]:
                    del pins[k]


# ------------------------------------------------------------------------------------------------
# Linear:  y = res + rowscale * (x W^T + b)
# ------------------------------------------------------------------------------------------------
class LinearFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, res, rowscale, rows_per_scale):
        _need_cuda(x, "linear")
        K = x.shape[-1]
        x2 = x.reshape(-1, K).contiguous()
        w = _lp(weight, x.dtype)
        res2 = res.reshape(-1, weight.shape[0]).contiguous() if res is not None else None
        y = linear_raw(x2, w, bias.detach() if bias is not None else None, res=res2, rowscale=rowscale,
                       rows_per_scale=rows_per_scale)
        ctx.save_for_backward(x2, weight, rowscale)
        ctx.has_bias = bias is not None
        ctx.has_res = res is not None
        ctx.rps = rows_per_scale
        ctx.xshape = x.shape
        return y.reshape(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight, rowscale = ctx.saved_tensors
        N = weight.shape[0]
        dy2 = dy.reshape(-1, N).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = linear_raw(dy2, _lp(weight, dy2.dtype, transpose=True), None, rowscale=rowscale, rows_per_scale=ctx.rps).reshape(ctx.xshape)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = wgrad_raw(dy2, x2, ctx.has_bias, rowscale, ctx.rps)
        dres = dy if ctx.has_res else None
        return dx, dw, db, dres, None, None


def linear(x, weight, bias=None, res=None, rowscale=None, rows_per_scale=1):
    return LinearFn.apply(x, weight, bias, res, rowscale, rows_per_scale)


class InProjFn(Function):
    """q = query W[:E]^T + b[:E],  [k | v] = key W[E:]^T + b[E:]  for the packed in-projection of the cross-modal attention
    (multihead_attention.py:137-158: in_proj_q / in_proj_kv slice in_proj_weight (3E, E)).  As two Linear calls on parameter
    slices, autograd's SliceBackward zero-fills a full-size gradient per slice, copies the slice in and adds the two -- ten
    small launches per attention for weight and bias; here the two weight-gradient launches write straight into the row
    ranges of ONE (3E, E) gradient."""

    @staticmethod
    def forward(ctx, query, key, weight, bias):
        _need_cuda(query, "in_proj")
        E = weight.shape[1]
        q2 = query.reshape(-1, E).contiguous()
        k2 = key.reshape(-1, E).contiguous()
        wq, wkv = weight[:E], weight[E:]
        bq, bkv = (bias.detach()[:E], bias.detach()[E:]) if bias is not None else (None, None)
        q = linear_raw(q2, _lp(wq, query.dtype), bq)
        kv = linear_raw(k2, _lp(wkv, key.dtype), bkv)
        ctx.save_for_backward(q2, k2, weight)
        ctx.has_bias = bias is not None
        ctx.shapes = (query.shape, key.shape)
        return q.reshape(*query.shape[:-1], E), kv.reshape(*key.shape[:-1], 2 * E)

    @staticmethod
    def backward(ctx, dq, dkv):
        q2, k2, weight = ctx.saved_tensors
        E = weight.shape[1]
        dq2 = dq.reshape(-1, E).contiguous()
        dkv2 = dkv.reshape(-1, 2 * E).contiguous()
        dquery = dkey = dw = db = None
        if ctx.needs_input_grad[0]:
            dquery = linear_raw(dq2, _lp(weight[:E], dq2.dtype, transpose=True), None).reshape(ctx.shapes[0])
        if ctx.needs_input_grad[1]:
            dkey = linear_raw(dkv2, _lp(weight[E:], dkv2.dtype, transpose=True), None).reshape(ctx.shapes[1])
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            dw = torch.empty((3 * E, E), dtype=torch.float32, device=dq2.device)
            db = torch.empty((3 * E,), dtype=torch.float32, device=dq2.device) if ctx.has_bias else None
            wgrad_raw(dq2, q2, ctx.has_bias, out=(dw[:E], db[:E] if db is not None else None))
            wgrad_raw(dkv2, k2, ctx.has_bias, out=(dw[E:], db[E:] if db is not None else None))
        return dquery, dkey, dw, db


def in_proj_q_kv(query, key, weight, bias):
    return InProjFn.apply(query, key, weight, bias)


# ------------------------------------------------------------------------------------------------
# MLP:  y = res + rowscale * (gelu(x W1^T + b1) W2^T + b2)      (Mlp of Swin; fc1/gelu/fc2 of the
# cross-modal layer).  GELU lives in fc1's epilogue, GELU' in the epilogue of fc2's input-gradient GEMM.
# ------------------------------------------------------------------------------------------------
def colsum_raw(x2, out_dtype=None):
    """out[n] = sum_m x2[m][n] (fmmt_colsum): x2 (M, N) contiguous bf16 / fp32; result in out_dtype (x2's dtype or fp32)"""
    M, N = x2.shape
    out_dtype = out_dtype or x2.dtype
    out = torch.empty((N,), dtype=out_dtype, device=x2.device)
    check(_lib.load().fmmt_colsum(dtype_code(x2.dtype), dtype_code(out_dtype), M, N, _p(x2), N, _p(out), _st()), f"fmmt_colsum(M={M},N={N})")
    return out


class PlmLayerNormFn(torch.autograd.Function):
    """torch's layer_norm forward, fmmt_layernorm_bwd_bf16 backward (bf16 activations and bf16 affine parameters: the text
    encoder's LayerNorms).  torch's backward is three launches (input gradient, partial and final gamma / beta sums); this is
    two, and saves nothing but x (the row statistics are recomputed in fp32)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ctx.save_for_backward(x, weight)
        ctx.eps = eps
        return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        C = x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        dy2 = dy.reshape(-1, C).contiguous()
        M = x2.shape[0]
        lib = _lib.load()
        dx = torch.empty_like(x2)
        dw = torch.empty_like(weight)
        db = torch.empty_like(weight)
        nbytes = lib.fmmt_layernorm_bwd_bf16_workspace(M, C)
        ws = _ws(nbytes, x.device)
        check(lib.fmmt_layernorm_bwd_bf16(M, C, float(ctx.eps), _p(dy2), _p(x2), _p(weight.detach().contiguous()), _p(dx), _p(dw), _p(db),
                                          _p(ws), nbytes, _st()), f"fmmt_layernorm_bwd_bf16(M={M},C={C})")
        return dx.reshape(x.shape), dw, db, None


def adamw_batch(n, blocks, desc, lr, step, total_norm, beta1, beta2, eps, weight_decay, max_norm, hf=False):
    """fmmt_adamw_batch: clip + AdamW + bf16 twins over the tensors of a descriptor table (train_step.FusedClipAdamW);
    hf: transformers.AdamW's update (the reference's optimizer class) instead of torch.optim.AdamW's"""
    check(_lib.load().fmmt_adamw_batch(n, blocks, _p(desc), _p(lr), _p(step), _p(total_norm), float(beta1), float(beta2), float(eps),
                                       float(weight_decay), float(max_norm), 1 if hf else 0, _st()), "fmmt_adamw_batch")


def adamw_batch_guarded(n, blocks, desc, lr, step, total_norm, beta1, beta2, eps, weight_decay, max_norm, hf=False):
    """fmmt_adamw_batch_guarded: adamw_batch that touches nothing when `total_norm` (required) holds a NaN or an inf.  `step` is the update count
    BEFORE this update and is only read -- guard_commit, behind it on the same stream, advances it; on a finite norm the bits are adamw_batch's
    with the step word one higher"""
    if total_norm is None:
        raise ValueError("adamw_batch_guarded: total_norm is what the guard decides on; it cannot be None")
    check(_lib.load().fmmt_adamw_batch_guarded(n, blocks, _p(desc), _p(lr), _p(step), _p(total_norm), float(beta1), float(beta2), float(eps),
                                               float(weight_decay), float(max_norm), 1 if hf else 0, _st()), "fmmt_adamw_batch_guarded")


def _group_tables(n, n_groups, group_of, groups, what):
    if group_of.dtype != torch.int32 or not group_of.is_contiguous() or group_of.numel() != n:
        raise ValueError(f"{what}: group_of is a contiguous int32 tensor with one entry per descriptor record ({n})")
    if groups.dtype != torch.uint8 or not groups.is_contiguous() or groups.numel() != n_groups * _lib.ADAMW_GROUP_BYTES or n_groups < 1:
        raise ValueError(f"{what}: groups is a contiguous uint8 tensor of n_groups >= 1 records of {_lib.ADAMW_GROUP_BYTES} bytes (include/fmmt_groups.h)")
    return _p(group_of), _p(groups)


def adamw_groups(n, blocks, desc, n_groups, group_of, groups, step, total_norm, max_norm, hf=False):
    """fmmt_adamw_groups: adamw_batch with lr / betas / eps / weight decay per record -- record i is stepped with groups[group_of[i]] (`groups`:
    n_groups records of _lib.ADAMW_GROUP_FIELDS as a uint8 device tensor, `group_of`: int32, one per record, every entry in [0, n_groups): the
    caller's to check, train_step.group_plan does); one step word, one norm word and one max_norm for all groups"""
    go, gr = _group_tables(n, n_groups, group_of, groups, "adamw_groups")
    check(_lib.load().fmmt_adamw_groups(n, blocks, _p(desc), n_groups, go, gr, _p(step), _p(total_norm), float(max_norm), 1 if hf else 0, _st()),
          "fmmt_adamw_groups")


def adamw_groups_guarded(n, blocks, desc, n_groups, group_of, groups, step, total_norm, max_norm, hf=False):
    """fmmt_adamw_groups_guarded: adamw_groups that touches nothing when `total_norm` (required) holds a NaN or an inf; `step` is the update count
    BEFORE this update and is only read -- guard_commit, behind it on the same stream, advances it (as adamw_batch_guarded to adamw_batch)"""
    if total_norm is None:
        raise ValueError("adamw_groups_guarded: total_norm is what the guard decides on; it cannot be None")
    go, gr = _group_tables(n, n_groups, group_of, groups, "adamw_groups_guarded")
    check(_lib.load().fmmt_adamw_groups_guarded(n, blocks, _p(desc), n_groups, go, gr, _p(step), _p(total_norm), float(max_norm), 1 if hf else 0,
                                                _st()), "fmmt_adamw_groups_guarded")


def grad_handover_raw(n, blocks, table, partial, norm_out):
    """fmmt_grad_handover over a device table of `n` records (train_step.FusedHandOver's layout; `blocks` blocks of 4096 elements, one fp32 word
    of `partial` each): every gradient into its fp32 slot and the norm of all of them into `norm_out`, on the current stream of the table's device"""
    check(_lib.load().fmmt_grad_handover(n, blocks, _p(table), _p(partial), _p(norm_out), torch.cuda.current_stream(table.device).cuda_stream),
          f"fmmt_grad_handover(n={n},blocks={blocks})")


def _guard_words(words):
    if words.dtype != torch.int64 or not words.is_contiguous() or words.numel() != _lib.GUARD_WORDS:
        raise ValueError(f"words: a contiguous int64 tensor of {_lib.GUARD_WORDS} entries (include/fmmt_guard.h)")
    return _p(words)


def guard_commit(total_norm, step, words):
    """fmmt_guard_commit, behind adamw_batch_guarded on the same stream: finite norm -> step += 1, applied += 1; else skipped += 1; last_norm = the
    norm's bits (`words`: train_step.TrainMonitor's)"""
    check(_lib.load().fmmt_guard_commit(_p(total_norm), _p(step), _guard_words(words), _st()), "fmmt_guard_commit")


def monitor_loss(loss, scale, words):
    """fmmt_monitor_loss: the fp32 device scalar `loss` times `scale` (the accumulation factor the step divided it by) into the monitor's double
    sum when finite, counted as non-finite otherwise"""
    if loss.dtype != torch.float32 or loss.numel() != 1:
        raise ValueError("monitor_loss: one float32 value on the device")
    check(_lib.load().fmmt_monitor_loss(_p(loss), float(scale), _guard_words(words), _st()), "fmmt_monitor_loss")


def param_digest(n, blocks, desc, out=None, partial=None):
    """fmmt_param_digest over adamw_batch's descriptor table (`n` records, `blocks` blocks of 4096 elements): six int64 words on the device --
    (S1, S2) of the parameters, of the first and of the second moments, S1 = sum of the elements' 32 bits, S2 = that sum weighted with
    (element index + 1) + (record index + 1) * 2^32, both mod 2^64 (include/fmmt_digest.h).  The words are uint64 bit patterns in an int64
    tensor (compare them, or view them as uint64 on the host).  `out`: a contiguous int64 tensor of six entries to write into; `partial`:
    6 * blocks int64 words of scratch (default: allocated per call).  Asynchronous on the current stream."""
    if out is None:
        out = torch.empty(6, dtype=torch.int64, device=desc.device)
    elif out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != 6:
        raise ValueError("param_digest: out is a contiguous int64 tensor of six entries")
    if partial is None:
        partial = torch.empty(6 * max(int(blocks), 1), dtype=torch.int64, device=desc.device)
    elif partial.dtype != torch.int64 or not partial.is_contiguous() or partial.numel() < 6 * blocks:
        raise ValueError("param_digest: partial is a contiguous int64 tensor of at least 6 * blocks entries")
    check(_lib.load().fmmt_param_digest(n, blocks, _p(desc), _p(partial), _p(out), _st()), "fmmt_param_digest")
    return out


def _stats_rows(t, rows, what):
    if t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != 4 or t.shape[0] < rows:
        raise ValueError(f"table_stats: {what} is a contiguous int32 tensor of at least {rows} rows of four words (include/fmmt_stats.h)")
    return _p(t)


def table_stats(which, n, blocks, desc, partial, stats, norm=None, bad_stats=None, bad_words=None):
    """fmmt_table_stats over adamw_batch's descriptor table (`n` records, `blocks` blocks of 4096 elements): per record the fp32 sum of squares,
    the largest magnitude that is not a NaN and the count of NaN / inf elements of field `which` (_lib.STATS_G / _P / _M / _V) into `stats`, (n, 4)
    int32 rows of _lib.STATS_FIELDS; `partial`: (blocks, 4) int32 rows of scratch.  `norm` (one fp32 device word, the one the guarded update reads):
    when it holds a NaN or an inf, `stats` is also copied into `bad_stats` (as `stats`), `bad_words[0]` (int64, two words) counts the bad update
    and `bad_words[1]` names the first record with a non-finite element or sum, -1 for none.  Two launches on the current stream, no atomics,
    capture-safe; train_step.GradReport owns the buffers."""
    if norm is None and (bad_stats is not None or bad_words is not None):
        raise ValueError("table_stats: bad_stats / bad_words are written on a non-finite `norm`; they cannot be given without it")
    if norm is not None and (norm.dtype != torch.float32 or norm.numel() != 1):
        raise ValueError("table_stats: norm is one float32 value on the device")
    if bad_words is not None and (bad_words.dtype != torch.int64 or not bad_words.is_contiguous() or bad_words.numel() != _lib.STATS_BAD_WORDS):
        raise ValueError(f"table_stats: bad_words is a contiguous int64 tensor of {_lib.STATS_BAD_WORDS} entries")
    check(_lib.load().fmmt_table_stats(int(which), n, blocks, _p(desc), _stats_rows(partial, blocks, "partial"), _stats_rows(stats, n, "stats"), _p(norm),
                                       None if bad_stats is None else _stats_rows(bad_stats, n, "bad_stats"), _p(bad_words), _st()), "fmmt_table_stats")
    return stats


class VendorLinearFn(torch.autograd.Function):
    """y = x W^T + b with the vendor library's GEMMs (torch.nn.functional.linear / matmul) and fmmt_colsum for the bias gradient:
    the text encoder's Linear layers (few thousand tokens: hipBLASLt's ground; its autograd formula spends a memset and a
    multi-block reduction, 25 us, on every bias gradient).  dx and dW are the calls autograd would make, bit for bit."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dy.matmul(weight)
        if ctx.needs_input_grad[1]:
            dw = dy2.t().mm(x.reshape(-1, x.shape[-1]))
        if ctx.needs_input_grad[2]:
            db = colsum_raw(dy2.contiguous())
        return dx, dw, db


def plm_tail_fwd_raw(h2, r2, gamma, beta, eps, p, seed_i, seed_t, salt, row_map=None):
    """fmmt_plm_dropadd_ln_fwd on (M, C) bf16 operands: returns (xsum, y).  row_map (int32 (M,), packed rows): fmmt_dropadd_ln_fwd_map -- row r draws
    the dropout mask of row row_map[r]"""
    M, C = h2.shape
    xsum, y = torch.empty_like(h2), torch.empty_like(h2)
    if row_map is not None:
        check(_lib.load().fmmt_dropadd_ln_fwd_map(_lib.BF16, M, C, float(eps), _p(h2), _p(r2), _p(gamma), _p(beta), float(p), seed_i, _p(seed_t), int(salt), _p(xsum),
                                                  _p(y), _p(row_map), _st()), f"fmmt_dropadd_ln_fwd_map(M={M},C={C})")
        return xsum, y
    check(_lib.load().fmmt_plm_dropadd_ln_fwd(M, C, float(eps), _p(h2), _p(r2), _p(gamma), _p(beta), float(p), seed_i, _p(seed_t), int(salt), _p(xsum), _p(y), _st()),
          f"fmmt_plm_dropadd_ln_fwd(M={M},C={C})")
    return xsum, y


def plm_tail_bwd_raw(dy2, xsum, gamma, eps, p, seed_i, seed_t, salt, row_map=None):
    """fmmt_plm_dropadd_ln_bwd (row_map: fmmt_dropadd_ln_bwd_map): returns (dx = the residual's gradient, dh = the dense output's, dgamma, dbeta, dbias)"""
    M, C = xsum.shape
    lib = _lib.load()
    dx, dh = torch.empty_like(xsum), torch.empty_like(xsum)
    dgamma, dbeta, dbias = torch.empty_like(gamma), torch.empty_like(gamma), torch.empty_like(gamma)
    nbytes = lib.fmmt_plm_dropadd_ln_bwd_workspace(M, C)
    ws = _ws(nbytes, xsum.device)
    if row_map is not None:
        check(lib.fmmt_dropadd_ln_bwd_map(_lib.BF16, M, C, eps, _p(dy2), _p(xsum), _p(gamma), p, seed_i, _p(seed_t), salt, _p(dx), _p(dh), _p(dgamma), _p(dbeta), _p(dbias),
                                          _p(ws), nbytes, _p(row_map), _st()), f"fmmt_dropadd_ln_bwd_map(M={M},C={C})")
        return dx, dh, dgamma, dbeta, dbias
    check(lib.fmmt_plm_dropadd_ln_bwd(M, C, eps, _p(dy2), _p(xsum), _p(gamma), p, seed_i, _p(seed_t), salt, _p(dx), _p(dh), _p(dgamma), _p(dbeta), _p(dbias), _p(ws), nbytes,
                                      _st()), f"fmmt_plm_dropadd_ln_bwd(M={M},C={C})")
    return dx, dh, dgamma, dbeta, dbias


def plm_gelu_bwd_colsum_raw(dact2, pre2):
    """fmmt_plm_gelu_bwd_colsum on (M, H) bf16: returns (dpre = dact * gelu'(pre), dbias = colsum(dpre))"""
    M, H = pre2.shape
    lib = _lib.load()
    dpre = torch.empty_like(pre2)
    dbias = torch.empty((H,), dtype=pre2.dtype, device=pre2.device)
    nbytes = lib.fmmt_plm_gelu_bwd_colsum_workspace(M, H)
    ws = _ws(nbytes, pre2.device)
    check(lib.fmmt_plm_gelu_bwd_colsum(M, H, _p(dact2), _p(pre2), _p(dpre), _p(dbias), _p(ws), nbytes, _st()), f"fmmt_plm_gelu_bwd_colsum(M={M},H={H})")
    return dpre, dbias


class PlmEmbeddingFn(torch.autograd.Function):
    """torch.nn.functional.embedding with the weight gradient of fmmt_embedding_bwd: the text encoder's word / position / token-type tables (transformers'
    *Embeddings, src/models.py:75-91).  torch's backward for <= 3072 indices is a 110-170 us launch per table (+ a fill) at the very end of the text encoder's
    backward; this is the fill + 5-10 us, deterministic, sums in fp32 with one rounding.  bf16 weight (V, C), C % 8 == 0, C <= 2048; at most 32768 indices."""

    @staticmethod
    def forward(ctx, ids, weight, padding_idx):
        ctx.save_for_backward(ids)
        ctx.cfg = (tuple(weight.shape), -1 if padding_idx is None else int(padding_idx))
        return torch.nn.functional.embedding(ids, weight, padding_idx)

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        (V, C), pad = ctx.cfg
        ids1 = ids.reshape(-1).contiguous()
        if ids1.dtype != torch.int64:
            ids1 = ids1.long()
        dy2 = _c16(dy.reshape(-1, C))
        dw = torch.empty((V, C), dtype=dy.dtype, device=dy.device)
        check(_lib.load().fmmt_embedding_bwd(ids1.numel(), C, V, _p(ids1), pad, _p(dy2), _p(dw), _st()), f"fmmt_embedding_bwd(T={ids1.numel()},C={C},V={V})")
        return None, dw, None


class PlmFfnFn(torch.autograd.Function):
    """y = LayerNorm(dropout(gelu(x W1^T + b1) W2^T + b2) + x): the feed-forward half of a BERT / RoBERTa layer (transformers' *Intermediate + *Output,
    src/models.py:75-91) as ONE autograd node.  Forward: the launches of the two modules (vendor GEMMs, torch's exact GELU, fmmt_plm_dropadd_ln_fwd).  Backward:
    the tail's launch + reduction, the two GEMMs behind it, d(pre) = d(act) gelu'(pre) together with b1's gradient in ONE pass (fmmt_plm_gelu_bwd_colsum; stock:
    GeluBackward + a column sum), and the input gradient d(pre) W1 + (the residual's gradient) as ONE GEMM with an accumulate epilogue (addmm_ into the tail's own dx buffer) instead
    of a GEMM and autograd's add.  Per layer and step 3 launches and two passes over the (tokens x 4096) matrix fewer."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, eps, p, seed, salt, row_map=None):
        pre = torch.nn.functional.linear(x, w1, b1)
        act = torch.nn.functional.gelu(pre)
        h = torch.nn.functional.linear(act, w2, b2)
        C = h.shape[-1]
        x2 = _c16(x.reshape(-1, C))
        seed_i, seed_t = _seed_args(seed)
        xsum, y = plm_tail_fwd_raw(h.reshape(-1, C), x2, gamma.detach(), beta.detach(), eps, p, seed_i, seed_t, salt, row_map)
        ctx.save_for_backward(x2, w1, w2, pre, act, xsum, gamma, seed_t)
        ctx.cfg = (float(eps), float(p), seed_i, int(salt))
        ctx.row_map = row_map                                   # packed rows (TokenLayout.row_map, no gradient): the padded call's dropout mask
        return y.reshape(h.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, pre, act, xsum, gamma, seed_t = ctx.saved_tensors
        eps, p, seed_i, salt = ctx.cfg
        M, C = xsum.shape
        dx_ln, dh, dgamma, dbeta, db2 = plm_tail_bwd_raw(_c16(dy.reshape(M, C)), xsum, gamma.detach(), eps, p, seed_i, seed_t, salt, ctx.row_map)
        act2, pre2 = act.reshape(M, -1), pre.reshape(M, -1)
        dact = dh.mm(w2)
        dw2 = dh.t().mm(act2)
        dpre, db1 = plm_gelu_bwd_colsum_raw(dact, pre2)
        dx = dx_ln.addmm_(dpre, w1) if ctx.needs_input_grad[0] else None      # in place: torch.addmm would first copy dx_ln into its result (a 4 MB memcpy node per layer)
        dw1 = dpre.t().mm(x2)
        return (dx.reshape(dy.shape) if dx is not None else None), dw1, db1, dw2, db2, dgamma, dbeta, None, None, None, None, None


class PlmSublayerTailFn(torch.autograd.Function):
    """y = LayerNorm(dropout(x W^T + b) + res): a BERT / RoBERTa sublayer behind its attention / GELU (transformers' *SelfOutput / *Output,
    src/models.py:75-91) as the vendor library's GEMM + ONE launch (fmmt_plm_dropadd_ln_fwd); backward: one launch + its reduction
    (dx of the LayerNorm = the residual's gradient, the dropout'ed gradient of the dense output, d gamma, d beta and the dense bias' gradient),
    then the two GEMMs autograd would issue.  No mask is stored: it is replayed from (`seed`: python int or 1-element int64 CUDA tensor, `salt`).
    bf16 activations and parameters.  8 launches per sublayer and step become 6 of which 2 are small."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, gamma, beta, eps, p, seed, salt, row_map=None):
        h = torch.nn.functional.linear(x, weight, bias)
        C = h.shape[-1]
        seed_i, seed_t = _seed_args(seed)
        xsum, y = plm_tail_fwd_raw(h.reshape(-1, C), _c16(res.reshape(-1, C)), gamma.detach(), beta.detach(), eps, p, seed_i, seed_t, salt, row_map)
        ctx.save_for_backward(x, weight, xsum, gamma, seed_t)
        ctx.cfg = (float(eps), float(p), seed_i, int(salt))
        ctx.row_map = row_map
        return y.reshape(h.shape)

    @staticmethod
    def backward(ctx, dy):
        x, weight, xsum, gamma, seed_t = ctx.saved_tensors
        eps, p, seed_i, salt = ctx.cfg
        M, C = xsum.shape
        dx, dh, dgamma, dbeta, dbias = plm_tail_bwd_raw(_c16(dy.reshape(M, C)), xsum, gamma.detach(), eps, p, seed_i, seed_t, salt, ctx.row_map)
        dxin = dh.reshape(dy.shape).matmul(weight) if ctx.needs_input_grad[0] else None
        dw = dh.t().mm(x.reshape(-1, x.shape[-1])) if ctx.needs_input_grad[2] else None
        return dxin, dx.reshape(dy.shape), dw, dbias, dgamma, dbeta, None, None, None, None, None


class DropAddLnFn(Function):
    """y = LayerNorm(dropout(h) + res) as ONE launch per direction (fmmt_dropadd_ln_fwd / _bwd): the tail of MELDTransEncoder's two sublayers
    (modules/Transformer.py:109-137: dense -> dropout -> + input -> TF LayerNorm) behind their GEMM.  bf16 activations, fp32 (master) or bf16
    affine parameters.  Replaces fused_dropout + add + fmmt_layernorm_fwd (forward) and fmmt_layernorm_bwd + its reduction + masked_scale (backward);
    no mask is stored: it is replayed from (`seed`: python int or 1-element int64 CUDA tensor, `salt`)."""

    @staticmethod
    def forward(ctx, h, res, gamma, beta, eps, p, seed, salt):
        _need_cuda(h, "dropadd_layer_norm")
        C = h.shape[-1]
        h2, r2 = _c16(h.reshape(-1, C)), _c16(res.reshape(-1, C))
        M = h2.shape[0]
        g, b = _c16(gamma.detach()), _c16(beta.detach())
        assert h2.dtype == torch.bfloat16 and r2.dtype == torch.bfloat16 and g.dtype == b.dtype and g.dtype in (torch.float32, torch.bfloat16)
        xsum, y = torch.empty_like(h2), torch.empty_like(h2)
        seed_i, seed_t = _seed_args(seed)
        check(_lib.load().fmmt_dropadd_ln_fwd(dtype_code(g.dtype), M, C, float(eps), _p(h2), _p(r2), _p(g), _p(b), float(p), seed_i, _p(seed_t), int(salt),
                                              _p(xsum), _p(y), _st()), f"fmmt_dropadd_ln_fwd(M={M},C={C})")
        ctx.save_for_backward(xsum, g, seed_t)
        ctx.cfg = (float(eps), float(p), seed_i, int(salt))
        return y.reshape(h.shape)

    @staticmethod
    def backward(ctx, dy):
        xsum, g, seed_t = ctx.saved_tensors
        eps, p, seed_i, salt = ctx.cfg
        M, C = xsum.shape
        dy2 = _c16(dy.reshape(M, C))
        lib = _lib.load()
        dx, dh = torch.empty_like(xsum), torch.empty_like(xsum)
        dgamma, dbeta = torch.empty_like(g), torch.empty_like(g)
        nbytes = lib.fmmt_dropadd_ln_bwd_workspace(M, C)
        ws = _ws(nbytes, xsum.device)
        check(lib.fmmt_dropadd_ln_bwd(dtype_code(g.dtype), M, C, eps, _p(dy2), _p(xsum), _p(g), p, seed_i, _p(seed_t), salt, _p(dx), _p(dh), _p(dgamma),
                                      _p(dbeta), None, _p(ws), nbytes, _st()), f"fmmt_dropadd_ln_bwd(M={M},C={C})")
        return dh.reshape(dy.shape), dx.reshape(dy.shape), dgamma, dbeta, None, None, None, None


def dropadd_layer_norm(h, res, gamma, beta, eps, p, seed, salt=0):
    return DropAddLnFn.apply(h, res, gamma, beta, eps, p, seed, salt)


class PlmQkvFn(torch.autograd.Function):
    """(q, k, v) = x [Wq; Wk; Wv]^T + [bq; bk; bv] as ONE vendor GEMM over the packed weight `w_all` (3E, E) of which the three nn.Linear weights are
    row slices (train_step.fuse_text_encoder re-points them): transformers' *SelfAttention.query / key / value (src/models.py:75-91).  Backward: the
    three gradients are gathered into one (M, 3E) matrix (one copy launch), then ONE input-gradient GEMM, ONE weight-gradient GEMM whose row slices are
    the three weight gradients, one column sum.  3 + 11 launches per layer and step become 1 + 4."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, bq, bk, bv, w_all, b_all):
        ctx.save_for_backward(x, w_all)
        E = wq.shape[0]
        y = torch.nn.functional.linear(x, w_all, b_all)
        return y[..., :E], y[..., E:2 * E], y[..., 2 * E:]

    @staticmethod
    def backward(ctx, dq, dk, dv):
        x, w_all = ctx.saved_tensors
        E = w_all.shape[0] // 3
        d = torch.cat([dq, dk, dv], dim=-1)
        d2 = d.reshape(-1, 3 * E)
        dx = d.matmul(w_all) if ctx.needs_input_grad[0] else None
        dw = d2.t().mm(x.reshape(-1, x.shape[-1]))
        db = colsum_raw(d2)
        return dx, dw[:E], dw[E:2 * E], dw[2 * E:], db[:E], db[E:2 * E], db[2 * E:], None, None


class PlmSelfAttnFn(torch.autograd.Function):
    """context = softmax(q k^T * scale + key_bias) v per head with (q, k, v) = x [Wq; Wk; Wv]^T + [bq; bk; bv]: a whole transformers *SelfAttention
    (src/models.py:75-91) as ONE vendor GEMM over the packed weight + fmmt_mha_fwd on the packed batch-major projection (dtype | FMMT_BATCH_MAJOR: the
    heads are column slices of it, no head-split transposes, no copies); backward fmmt_mha_bwd writes [dq | dk | dv] in place, then the three calls
    PlmQkvFn makes.  Replaces the library attention torch's scaled_dot_product_attention dispatches to (round 6, 4 x 512 tokens x 16 heads, dropout 0.1:
    47 / 103 us forward / backward per layer against 20 / 53) together with its layout copies and the gather of the three gradients.
    x (B, S, E) bf16; head_dim 64; key_bias fp32 (B, S) or None; seed: python int or a 1-element int64 CUDA tensor (graph-replay safe); the dropout
    stream is the attention kernels' own (replayed in the backward, no mask stored)."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, bq, bk, bv, w_all, b_all, num_heads, scale, p, seed, key_bias, layout=None):
        qkv = torch.nn.functional.linear(x, w_all, b_all)
        seed_i, seed_t = _seed_args(seed)
        ctx.layout = layout
        if layout is not None:
            # packed rows (TokenLayout; x (1, cap, E)): the kernels' ragged mode, bit for bit the padded call on the real rows -- no key bias is needed,
            # a sequence's keys end where it ends
            assert key_bias is None and x.shape[0] == 1 and x.shape[1] == layout.cap, (tuple(x.shape), layout.cap)
            out, lse = mha_ragged_fwd_raw(qkv[0], layout, int(num_heads), float(scale), float(p), seed_i, seed_t)
            ctx.save_for_backward(x, w_all, qkv, out, lse, seed_t, None)
            ctx.cfg = (int(num_heads), float(scale), float(p), seed_i)
            return out[None]
        if key_bias is not None:                                 # the kernels read it as a row-major fp32 (B, S) array
            key_bias = key_bias.detach().to(torch.float32).contiguous()
            assert key_bias.shape == x.shape[:2], f"key_bias must be (B, S) = {tuple(x.shape[:2])}, got {tuple(key_bias.shape)}"
        out, lse = mha_packed_bm_fwd_raw(qkv, int(num_heads), float(scale), float(p), seed_i, seed_t, key_bias)
        ctx.save_for_backward(x, w_all, qkv, out, lse, seed_t, key_bias)
        ctx.cfg = (int(num_heads), float(scale), float(p), seed_i)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w_all, qkv, out, lse, seed_t, key_bias = ctx.saved_tensors
        num_heads, scale, p, seed_i = ctx.cfg
        E = w_all.shape[0] // 3
        if ctx.layout is not None:
            d = mha_ragged_bwd_raw(qkv[0], ctx.layout, out, _c16(dout[0]), lse, num_heads, scale, p, seed_i, seed_t)[None]
        else:
            d = mha_packed_bm_bwd_raw(qkv, out, _c16(dout), lse, num_heads, scale, p, seed_i, seed_t, key_bias)
        d2 = d.reshape(-1, 3 * E)
        dx = d.matmul(w_all) if ctx.needs_input_grad[0] else None
        dw = d2.t().mm(x.reshape(-1, x.shape[-1]))
        db = colsum_raw(d2)
        return dx, dw[:E], dw[E:2 * E], dw[2 * E:], db[:E], db[E:2 * E], db[2 * E:], None, None, None, None, None, None, None, None


def mlp_fused_raw(x2, w1l, b1, w2l, b2, res2, rowscale, rows_per_scale, h_pre, h_act=None, dg=False):
    """one launch: y = res + rowscale * (gelu(x W1^T + b1) W2^T + b2); h_pre / h_act (or None) receive the pre-activation (dg: its gelu') / activation"""
    M, C = x2.shape
    y = torch.empty((M, C), dtype=x2.dtype, device=x2.device)
    rc = _lib.load().fmmt_mlp_fwd(dtype_code(x2.dtype) | (SAVE_DG if dg else 0), M, C, _p(x2), _p(w1l), _p(b1), _p(w2l), _p(b2), _p(res2), _p(rowscale), rows_per_scale,
                                  _p(y), _p(h_pre), _p(h_act), _st())
    check(rc, f"fmmt_mlp_fwd(M={M},C={C})")
    return y


_MLP_FUSED = True            # module constants, not environment switches: the tests and probes patch them (False = always the two-launch form)
# the widths that take the fused kernels (the others: LayerNorm + two GEMM launches).  Round 6 measured stage 1 (C = 192) both ways once the derivative was stored and the
# backward's product ran on the phase kernels: Swin forward + backward 40.71 / 40.66 (fused) vs 40.40 / 40.62 ms, whole step 58.00 / 57.97 vs 57.82 / 57.57 and, another
# box, 57.57 / 57.19 vs 57.42 / 57.39 -- a wash in time; but the unfused form rounds d(LN out) and gelu' to bf16 on the way and moved the whole-Swin bf16 gradient statistics
# from < 0.10 to 0.12 relative L2 against the fp32 oracle (tests/test_gpu_swin.py): the fused kernels stay.  (The fused C = 192 kernels feed each 16-byte LDS weight read to
# two MFMAs, the GEMMs' 96 x 64 wave tiles to six: that is why they are no faster; at C = 96 the fused form moves 2.7 GB where two launches move 5.8: 1.07 against 1.59 ms.)
_MLP_FUSED_WIDTHS = (96, 192)
# fp32 (parity) models take the fused Mlp entry points too -- their element-type-generic instantiations, csrc/mlp_ref.hip -- so that the
# fp32 goldens reach the fused kernels' algorithm at 1e-3 (False: LayerNorm + two GEMM launches, as in rounds 1-3; see set_fp32_route)
_MLP_F32 = True


def _mlp_dtype_ok(dt):
    return dt == torch.bfloat16 or (_MLP_F32 and dt == torch.float32)
# The fused forward also stores the activation and fc2's weight gradient reads it (storing only the pre-activation and recomputing
# gelu() while the weight-gradient kernel stages its operand measured slower: 0.75 vs 0.40 ms per stage-0 launch; round 2)
_MLP_SAVE_H = True
# Every Mlp saves gelu'(pre-activation) instead of the pre-activation (round 6: FMMT_EPI_GELU_DG / FMMT_EPI_MUL_AUX, FMMT_SAVE_DG; False: the pre-activation and a
# GELU' evaluation in the backward, as before)
_MLP_SAVE_DG = True
# ... the FUSED kernels at these widths only.  C = 192: the forward kernel sits at the 256-register limit and the second output costs 34 spilled registers
# (round 6, same call: forward 0.724 -> 1.123 ms, backward 0.892 -> 0.809); C = 96: forward 1.08 (unchanged), backward 1.135 -> 0.886 ms
_MLP_FUSED_DG_WIDTHS = (96,)


def _mlp_fusable(x2, w1, w2, b1, b2):
    C = x2.shape[1]
    return (_MLP_FUSED and _mlp_dtype_ok(x2.dtype) and C in _MLP_FUSED_WIDTHS and w1.shape == (4 * C, C) and w2.shape == (C, 4 * C)
            and b1 is not None and b2 is not None and x2.shape[0] >= 4096)


def mlp_saves_dg(x2, w1, w2, b1, b2) -> bool:
    """does the Mlp of these operands save gelu'(pre-activation) in place of the pre-activation?  (one rule for ops.MlpFn and torch.ops.fmmt.mlp)"""
    if not (_MLP_SAVE_DG and _MLP_SAVE_H):
        return False
    return x2.shape[1] in _MLP_FUSED_DG_WIDTHS if _mlp_fusable(x2, w1, w2, b1, b2) else True


class MlpFn(Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, res, rowscale, rows_per_scale, grad_on=True):
        _need_cuda(x, "mlp")
        K = x.shape[-1]
        x2 = x.reshape(-1, K).contiguous()
        w1l, w2l = _lp(w1, x.dtype), _lp(w2, x.dtype)
        # needs_input_grad stays True under torch.no_grad() whenever a parameter requires grad, and grad mode is always off inside
        # Function.forward: the caller's grad mode comes in as `grad_on` (evaluated in the wrapper function)
        train = grad_on and any(ctx.needs_input_grad)
        h_pre = torch.empty((x2.shape[0], w1.shape[0]), dtype=x.dtype, device=x.device) if train else None
        res2 = res.reshape(-1, w2.shape[0]).contiguous() if res is not None else None
        if _mlp_fusable(x2, w1, w2, b1, b2):
            # Swin stages 0 / 1: the whole Mlp in one launch, hidden activation kept on chip (csrc/mlp_fused.hip); the
            # backward recomputes gelu(h_pre) inside the weight-gradient kernel instead of reading a stored activation
            h = torch.empty_like(h_pre) if (train and _MLP_SAVE_H) else None
            ctx.dg = mlp_saves_dg(x2, w1, w2, b1, b2)
            y = mlp_fused_raw(x2, w1l, b1.detach().float().contiguous(), w2l, b2.detach().float().contiguous(), res2, rowscale, rows_per_scale, h_pre, h, ctx.dg)
        else:
            # Swin stages 2 / 3 (and any other width): two GEMM launches.  The only thing the backward needs of the pre-activation is gelu'(.) of it,
            # so the forward's epilogue -- which evaluates gelu() there anyway, and shares its exponential -- stores THAT (FMMT_EPI_GELU_DG) and the
            # backward's input-gradient GEMM multiplies by it (FMMT_EPI_MUL_AUX: no polynomial in the epilogue, so it runs on the phase kernels)
            ctx.dg = mlp_saves_dg(x2, w1, w2, b1, b2)
            h = linear_raw(x2, w1l, b1.detach(), epi=EPI_GELU_DG if ctx.dg else EPI_GELU, y_pre=h_pre)
            y = linear_raw(h, w2l, b2.detach(), res=res2, rowscale=rowscale, rows_per_scale=rows_per_scale)
        ctx.save_for_backward(x2, w1, w2, h_pre, h, rowscale)
        ctx.rps = rows_per_scale
        ctx.has_res = res is not None
        ctx.xshape = x.shape
        return y.reshape(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, h_pre, h, rowscale = ctx.saved_tensors
        dy2 = dy.reshape(-1, w2.shape[0]).contiguous()
        # d(h_pre) = (s * dy @ W2) * gelu'(h_pre)   [fused epilogue]
        # (ctx.dg: h_pre holds the derivative itself)
        dh = linear_raw(dy2, _lp(w2, dy2.dtype, transpose=True), None, epi=EPI_MUL_AUX if ctx.dg else EPI_GELU_BWD, aux=h_pre, rowscale=rowscale,
                        rows_per_scale=ctx.rps)
        dw2, db2 = wgrad_raw(dy2, h, True, rowscale, ctx.rps) if h is not None else wgrad_raw(dy2, h_pre, True, rowscale, ctx.rps, x_gelu=True)
        dx = linear_raw(dh, _lp(w1, dy2.dtype, transpose=True), None).reshape(ctx.xshape) if ctx.needs_input_grad[0] else None
        dw1, db1 = wgrad_raw(dh, x2, True)
        return dx, dw1, db1, dw2, db2, (dy if ctx.has_res else None), None, None, None


_MLP_BWD_FUSED = True        # False = GELU' GEMM + input-gradient GEMM as two launches
# "192" adds stage 1 (one token tile per wave there: no spill, all tests pass, and 0.1 ms SLOWER per Swin forward + backward than the two
# GEMM launches + LayerNorm backward it replaces: 43.69 against 43.57 ms, same call) -- off
_MLP_BWD_WIDTHS = (96, 192)  # stage 0 and stage 1 (round 4: stage 1 measured 0.1 ms slower than the GELU' GEMM + input-gradient GEMM it replaces and stayed off; round 5, same-call A/B of whole steps: 57.56 / 57.57 against 57.67 / 57.63 ms -- on)
_MLP_BWD_LN = True           # False = fmmt_mlp_bwd_input + fmmt_layernorm_bwd


def mlp_bwd_input_raw(dy2, h_pre, w1, w2, rowscale, rows_per_scale, dg=False):
    """(dh, dx) of the Mlp: one launch where the fused kernel applies (bf16, C = 96), the two GEMM launches otherwise.  dg: h_pre holds gelu'(pre-activation)"""
    M, C = dy2.shape
    dt = dy2.dtype
    if _MLP_BWD_FUSED and _mlp_dtype_ok(dt) and C in _MLP_BWD_WIDTHS and w1.shape == (4 * C, C) and M >= 4096:
        dh = torch.empty((M, 4 * C), dtype=dt, device=dy2.device)
        dx = torch.empty_like(dy2)
        w2t, w1t = _lp(w2, dt, transpose=True), _lp(w1, dt, transpose=True)     # both alive until the launch is enqueued (_lp's note on operands)
        rc = _lib.load().fmmt_mlp_bwd_input(dtype_code(dt) | (SAVE_DG if dg else 0), M, C, _p(dy2), _p(h_pre), _p(w2t), _p(w1t),
                                            _p(rowscale), rows_per_scale, _p(dh), _p(dx), _st())
        check(rc, f"fmmt_mlp_bwd_input(M={M},C={C})")
        return dh, dx
    dh = linear_raw(dy2, _lp(w2, dt, transpose=True), None, epi=EPI_MUL_AUX if dg else EPI_GELU_BWD, aux=h_pre, rowscale=rowscale, rows_per_scale=rows_per_scale)
    return dh, linear_raw(dh, _lp(w1, dt, transpose=True), None)


class MlpLnFn(Function):
    """y = x + rowscale * Mlp(LayerNorm(x)): forward = fmmt_mlp_ln_fwd (one launch, LayerNorm formed on the operand fragments);
    backward = the Mlp's four GEMM launches on the saved LN(x) / pre-activation / activation, then fmmt_layernorm_bwd with the
    residual gradient as its `add` operand."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, eps, w1, b1, w2, b2, rowscale, rows_per_scale, grad_on=True):
        _need_cuda(x, "mlp_ln")
        C = x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        M = x2.shape[0]
        train = grad_on and any(ctx.needs_input_grad)
        dev = x.device
        g, b = ln_w.detach().float().contiguous(), ln_b.detach().float().contiguous()
        y = torch.empty_like(x2)
        xn = torch.empty_like(x2) if train else None
        mean = torch.empty(M, dtype=torch.float32, device=dev) if train else None
        rstd = torch.empty(M, dtype=torch.float32, device=dev) if train else None
        h_pre = torch.empty((M, 4 * C), dtype=x.dtype, device=dev) if train else None
        h = torch.empty_like(h_pre) if train else None
        ctx.dg = bool(train and _MLP_SAVE_DG and C in _MLP_FUSED_DG_WIDTHS)
        w1l, w2l, b1f, b2f = _lp(w1, x.dtype), _lp(w2, x.dtype), b1.detach().float().contiguous(), b2.detach().float().contiguous()
        rc = _lib.load().fmmt_mlp_ln_fwd(dtype_code(x.dtype) | (SAVE_DG if ctx.dg else 0), M, C, _p(x2), _p(g), _p(b), float(eps), _p(w1l), _p(b1f),
                                         _p(w2l), _p(b2f), _p(rowscale), rows_per_scale, _p(y), _p(xn), _p(mean), _p(rstd),
                                         _p(h_pre), _p(h), _st())
        check(rc, f"fmmt_mlp_ln_fwd(M={M},C={C})")
        ctx.save_for_backward(x2, xn, mean, rstd, g, w1, w2, h_pre, h, rowscale)
        ctx.rps = rows_per_scale
        ctx.xshape = x.shape
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, xn, mean, rstd, g, w1, w2, h_pre, h, rowscale = ctx.saved_tensors
        C = x2.shape[1]
        lib = _lib.load()
        dy2 = dy.reshape(-1, C).contiguous()
        M, dt = x2.shape[0], x2.dtype
        if _MLP_BWD_FUSED and _MLP_BWD_LN and _mlp_dtype_ok(dt) and C in _MLP_BWD_WIDTHS and M >= 4096:
            # input gradient of the Mlp AND the LayerNorm backward in one launch (fmmt_mlp_ln_bwd_input)
            dh = torch.empty((M, 4 * C), dtype=dt, device=x2.device)
            dx = torch.empty_like(x2)
            dg = torch.empty(C, dtype=torch.float32, device=x2.device)
            db = torch.empty(C, dtype=torch.float32, device=x2.device)
            nbytes = lib.fmmt_mlp_ln_bwd_input_workspace(C)
            ws = _ws(nbytes, x2.device)
            w2t, w1t = _lp(w2, dt, transpose=True), _lp(w1, dt, transpose=True)
            rc = lib.fmmt_mlp_ln_bwd_input(dtype_code(dt) | (SAVE_DG if ctx.dg else 0), M, C, _p(dy2), _p(h_pre), _p(w2t), _p(w1t),
                                           _p(rowscale), ctx.rps, _p(x2), _p(mean), _p(rstd), _p(g), _p(dh), _p(dx), _p(dg), _p(db), _p(ws), nbytes, _st())
            check(rc, f"fmmt_mlp_ln_bwd_input(M={M},C={C})")
            dw2, db2 = wgrad_raw(dy2, h, True, rowscale, ctx.rps)
            dw1, db1 = wgrad_raw(dh, xn, True)
            return dx.reshape(ctx.xshape), dg, db, None, dw1, db1, dw2, db2, None, None, None
        dh, dxn = mlp_bwd_input_raw(dy2, h_pre, w1, w2, rowscale, ctx.rps, ctx.dg)
        dw2, db2 = wgrad_raw(dy2, h, True, rowscale, ctx.rps)
        dw1, db1 = wgrad_raw(dh, xn, True)
        del dh
        dx, dg, db = layernorm_bwd_raw(dxn, x2, mean, rstd, g, add=dy2)
        return dx.reshape(ctx.xshape), dg, db, None, dw1, db1, dw2, db2, None, None, None


def mlp_ln_fusable(x, w1, w2, b1, b2):
    C = x.shape[-1]
    return (_MLP_FUSED and x.is_cuda and _mlp_dtype_ok(x.dtype) and C in _MLP_FUSED_WIDTHS and w1.shape == (4 * C, C) and w2.shape == (C, 4 * C)
            and b1 is not None and b2 is not None and x.numel() // C >= 4096)


def mlp_ln(x, ln_w, ln_b, eps, w1, b1, w2, b2, rowscale=None, rows_per_scale=1):
    """x + rowscale * Mlp(LayerNorm(x)) in one launch (Swin stages 0 / 1)"""
    return MlpLnFn.apply(x, ln_w, ln_b, eps, w1, b1, w2, b2, rowscale, rows_per_scale, torch.is_grad_enabled())


def mlp(x, w1, b1, w2, b2, res=None, rowscale=None, rows_per_scale=1):
    return MlpFn.apply(x, w1, b1, w2, b2, res, rowscale, rows_per_scale, torch.is_grad_enabled())


# ------------------------------------------------------------------------------------------------
# LayerNorm (optionally with the PatchMerging 2x2 gather folded in)
# ------------------------------------------------------------------------------------------------
def layernorm_fwd_raw(x, g, b, eps, merge_hw=0):
    """fmmt_layernorm_fwd over the last dimension of a contiguous x, g / b fp32: returns (y, mean, rstd).  merge_hw: x is a (n, merge_hw^2, C/4)
    token grid and a row of the LayerNorm is PatchMerging's 2x2-neighbour concat -> y (n, merge_hw^2 / 4, C) (Swin_Transformer.py:316-325)"""
    if merge_hw:
        n, L, Cq = x.shape
        assert L == merge_hw * merge_hw
        M, C = n * (merge_hw // 2) ** 2, 4 * Cq
        out_shape = (n, (merge_hw // 2) ** 2, C)
    else:
        C = x.shape[-1]
        M = x.numel() // C
        out_shape = x.shape
    y = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    rc = _lib.load().fmmt_layernorm_fwd(dtype_code(x.dtype), M, C, _p(x), _p(g), _p(b), float(eps), _p(y), _p(mean), _p(rstd), merge_hw, _st())
    check(rc, f"fmmt_layernorm_fwd(M={M},C={C},merge={merge_hw})")
    return y, mean, rstd


def layernorm_bwd_raw(dy, x, mean, rstd, g, add=None, merge_hw=0):
    """fmmt_layernorm_bwd on what layernorm_fwd_raw took and returned (all contiguous): (dx, dgamma, dbeta), the last two fp32.  add: a tensor of
    x's shape summed into dx (the gradient of the residual branch around a pre-norm LayerNorm)"""
    M, C = mean.numel(), g.numel()
    lib = _lib.load()
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    nbytes = lib.fmmt_layernorm_bwd_workspace(C)
    ws = _ws(nbytes, x.device)
    rc = lib.fmmt_layernorm_bwd(dtype_code(x.dtype), M, C, _p(dy), _p(x), _p(mean), _p(rstd), _p(g), _p(add), _p(dx), _p(dg), _p(db), merge_hw,
                                _p(ws), nbytes, _st())
    check(rc, f"fmmt_layernorm_bwd(M={M},C={C},merge={merge_hw}{',add' if add is not None else ''})")
    return dx, dg, db


class LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, merge_hw):
        _need_cuda(x, "layer_norm")
        x = x.contiguous()
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        y, mean, rstd = layernorm_fwd_raw(x, g, b, eps, merge_hw)
        ctx.save_for_backward(x, mean, rstd, g)
        ctx.merge_hw = merge_hw
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, g = ctx.saved_tensors
        dx, dg, db = layernorm_bwd_raw(dy.contiguous(), x, mean, rstd, g, merge_hw=ctx.merge_hw)
        return dx, dg, db, None, None


def layer_norm(x, gamma, beta, eps=1e-5, merge_hw=0):
    return LayerNormFn.apply(x, gamma, beta, eps, merge_hw)


_PATCH_LN = True             # False = projection and LayerNorm as two launches


class PatchProjLnFn(Function):
    """LayerNorm(cols W^T + b) of PatchEmbed in one launch (fmmt_patch_embed_ln_fwd); backward = fmmt_layernorm_bwd on the saved
    pre-LayerNorm rows, then the projection's weight / bias / input gradients as for any Linear."""

    @staticmethod
    def forward(ctx, cols, weight, bias, gamma, beta, eps, grad_on=True):
        _need_cuda(cols, "patch_proj_ln")
        M, K = cols.shape
        C = weight.shape[0]
        train = grad_on and any(ctx.needs_input_grad)
        dev, dt = cols.device, cols.dtype
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        y = torch.empty((M, C), dtype=dt, device=dev)
        x_pre = torch.empty_like(y) if train else None
        mean = torch.empty(M, dtype=torch.float32, device=dev) if train else None
        rstd = torch.empty(M, dtype=torch.float32, device=dev) if train else None
        rc = _lib.load().fmmt_patch_embed_ln_fwd(dtype_code(dt), M, C, K, _p(cols), _p(_lp(weight, dt)), _p(bias.detach().float().contiguous() if bias is not None else None),
                                                 _p(g), _p(b), float(eps), _p(x_pre), _p(y), _p(mean), _p(rstd), _st())
        check(rc, f"fmmt_patch_embed_ln_fwd(M={M})")
        ctx.save_for_backward(cols, weight, x_pre, mean, rstd, g)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        cols, weight, x_pre, mean, rstd, g = ctx.saved_tensors
        dy = dy.contiguous()
        dxp, dg, db = layernorm_bwd_raw(dy, x_pre, mean, rstd, g)
        dw, dbias = wgrad_raw(dxp, cols, ctx.has_bias)
        dcols =linear_raw(dxp, _lp(weight, dy.dtype, transpose=True), None) if ctx.needs_input_grad[0] else None
        return dcols, dw.view_as(weight), dbias, dg, db, None, None


def patch_proj_ln_fusable(cols, weight, norm):
    # (fp32: the same kernel template over 8 x mfma_f32_16x16x4 per 32-deep block -- the parity instantiation, csrc/patch_ln.hip)
    return (_PATCH_LN and norm is not None and cols.is_cuda and cols.dtype in (torch.bfloat16, torch.float32) and tuple(weight.shape) == (96, 48)
            and tuple(norm.weight.shape) == (96,))


def patch_proj_ln(cols, weight, bias, gamma, beta, eps):
    return PatchProjLnFn.apply(cols, weight, bias, gamma, beta, eps, torch.is_grad_enabled())


class ResidualLayerNormFn(Function):
    """(x, LN(x)) for pre-norm residual blocks `x + f(LN(x))`: the residual branch takes the first output,
    f the second.  Backward receives both incoming gradients at once, so the residual-gradient add is the
    `add` operand of the LayerNorm-backward kernel instead of a separate elementwise pass."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        _need_cuda(x, "layer_norm")
        x = x.contiguous()
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        y, mean, rstd = layernorm_fwd_raw(x, g, b, eps)
        ctx.save_for_backward(x, mean, rstd, g)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, dres, dy):
        x, mean, rstd, g = ctx.saved_tensors
        dx, dg, db = layernorm_bwd_raw(dy.contiguous(), x, mean, rstd, g, add=dres.contiguous() if dres is not None else None)
        return dx, dg, db, None


def residual_layer_norm(x, gamma, beta, eps=1e-5):
    """returns (x, LN(x)); use the returned x as the residual input of the block's last GEMM"""
    return ResidualLayerNormFn.apply(x, gamma, beta, eps)


# ------------------------------------------------------------------------------------------------
# (shifted-)window attention core on token-order qkv
# ------------------------------------------------------------------------------------------------
def window_attn_fwd_raw(qkv, tab, index_i32, m, n_img, H, W, num_heads, shift, scale, mask_is_shift):
    """fmmt_window_attn_fwd on contiguous token-order qkv (n_img*H*W, 3C), the fp32 bias table and the fp32 mask m (nW, 49, 49) or None;
    mask_is_shift: m is the standard SW-MSA mask of (H, W, shift), which the kernel derives from the window coordinates.  Returns (out, lse)"""
    C = qkv.shape[-1] // 3
    nW = (H // 7) * (W // 7)
    out = torch.empty((n_img * H * W, C), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((n_img * nW * num_heads * 49,), dtype=torch.float32, device=qkv.device)
    rc = _lib.load().fmmt_window_attn_fwd(dtype_code(qkv.dtype), n_img, H, W, C, num_heads, shift, _p(qkv), _p(tab), _p(index_i32), _p(m),
                                          m.shape[0] if m is not None else 0, int(mask_is_shift), float(scale), _p(out), _p(lse), _st())
    check(rc, f"fmmt_window_attn_fwd(n={n_img},H={H},W={W},C={C},heads={num_heads},shift={shift})")
    return out, lse


def window_attn_bwd_raw(qkv, out, dout, lse, tab, index_i32, m, n_img, H, W, num_heads, shift, scale, mask_is_shift):
    """fmmt_window_attn_bwd on window_attn_fwd_raw's operands and results: returns (dqkv, dtable), dtable fp32 as the table"""
    C = qkv.shape[-1] // 3
    lib = _lib.load()
    dqkv = torch.empty_like(qkv)
    dtable = torch.empty_like(tab)
    nbytes = lib.fmmt_window_attn_bwd_workspace(num_heads)
    ws = _ws(nbytes, qkv.device)
    rc = lib.fmmt_window_attn_bwd(dtype_code(qkv.dtype), n_img, H, W, C, num_heads, shift, _p(qkv), _p(out), _p(dout), _p(lse), _p(tab), _p(index_i32),
                                  _p(m), m.shape[0] if m is not None else 0, int(mask_is_shift), float(scale), _p(dqkv), _p(dtable), _p(ws), nbytes, _st())
    check(rc, f"fmmt_window_attn_bwd(n={n_img},H={H},W={W},C={C},heads={num_heads},shift={shift})")
    return dqkv, dtable


class WindowAttnCoreFn(Function):
    @staticmethod
    def forward(ctx, qkv, table, index_i32, mask, n_img, H, W, num_heads, shift, scale, mask_is_shift):
        _need_cuda(qkv, "window_attention")
        qkv = qkv.contiguous()
        tab = table.detach().float().contiguous()
        m = mask.detach().float().contiguous() if mask is not None else None
        ctx.cfg = (n_img, H, W, num_heads, shift, scale, mask_is_shift)
        out, lse = window_attn_fwd_raw(qkv, tab, index_i32, m, *ctx.cfg)
        ctx.save_for_backward(qkv, out, lse, tab, index_i32, m)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, tab, index_i32, m = ctx.saved_tensors
        dqkv, dtable = window_attn_bwd_raw(qkv, out, dout.contiguous(), lse, tab, index_i32, m, *ctx.cfg)
        return dqkv, dtable, None, None, None, None, None, None, None, None, None


def window_attn_core(qkv, table, index_i32, mask, n_img, H, W, num_heads, shift, scale, mask_is_shift=False):
    return WindowAttnCoreFn.apply(qkv, table, index_i32, mask, n_img, H, W, num_heads, shift, scale, mask_is_shift)


# ------------------------------------------------------------------------------------------------
# the attention half of a Swin block as ONE launch (csrc/wblock.hip): y = x + s * proj(W-MSA(LN(x) Wqkv^T + b))
# ------------------------------------------------------------------------------------------------
_WBLOCK = True               # False = always the four-launch form
_WBLOCK_WIDTHS = (96,)       # (96, 192): the four-launch block op at stage 1 as well
# fp32 (parity) models take the fused forward too -- its element-type-generic instantiation, csrc/wblock_ref.hip -- so that every fp32 golden of
# the stage-0 blocks and of the whole Swin reaches the fused kernel's algorithm at 1e-3 (False: the four fp32 launches, as in rounds 1-3)
_WBLOCK_F32 = True
_WBLOCK_BWD = True           # False: the backward re-computes qkv with a GEMM and runs fmmt_window_attn_bwd
_WBLOCK_LNBWD = True         # False: d(LN out) GEMM and LayerNorm backward as two launches


def set_fp32_route(fused: bool) -> None:
    """Which kernels an fp32 (parity-mode) model runs at Swin stages 0/1.  True (default): the element-type-generic restatements of the fused
    bf16 kernels (csrc/wblock_ref.hip, mlp_ref.hip, wattn_bwd_ref.hip) -- the parity instantiations the goldens are held to; they read weights
    as fragments from memory, spill, and run several times slower than the bf16 kernels (they exist to be checked, not to be fast).
    False: the rounds 1-3 fp32 path (LayerNorm + GEMM launches + the VALU window-attention kernels), ~2x faster in fp32 and a different
    algorithm from what the benchmark runs.  bf16 models are not affected."""
    global _MLP_F32, _WBLOCK_F32
    _MLP_F32 = bool(fused)
    _WBLOCK_F32 = bool(fused)


def window_block_fusable(x, C, num_heads, window_size, shift, mask, mask_is_shift):
    """the block-half op runs where it pays: the bf16 stage-0 geometry (C = 96, head_dim 32, 7x7 windows) with no mask or the standard
    SW-MSA mask -- fused forward kernel + recompute backward.  (C = 192 is implemented -- four forward launches, the same recompute
    backward, tests/test_gpu_wblock.py -- and reachable with _WBLOCK_WIDTHS = (96, 192), but at stage 1 the recompute backward loses: six heads
    re-read LN(x) / dy and redo 96 MFMAs per wave, 835 us per launch against 480 + 130 for the attention backward and the proj input
    gradient it replaces.)"""
    ok_dtype = x.dtype == torch.bfloat16 or (_WBLOCK_F32 and x.dtype == torch.float32 and C == 96)
    return (_WBLOCK and x.is_cuda and ok_dtype and C in _WBLOCK_WIDTHS and num_heads * 32 == C and tuple(window_size) == (7, 7)
            and ((shift == 0 and mask is None) or (shift > 0 and mask is not None and mask_is_shift)))


def window_block_raw(x2, n_img, H, W, num_heads, shift, ln_g, ln_b, eps, wqkv, bqkv, wproj, bproj, table, index_i32, scale, rowscale, save, mask=None):
    """y = x + rowscale * (proj(W-MSA(LN(x) wqkv^T + bqkv)) + bproj); returns (y, xn, attn_out, mean, rstd, lse) -- what the backward needs
    (never qkv).  C = 96: one launch (fmmt_window_block_fwd), the four saved tensors None unless `save`; C = 192: LayerNorm, qkv Linear,
    attention core, proj Linear as four launches, qkv a temporary (`mask`: the standard SW-MSA mask tensor when shift > 0)."""
    M, C = x2.shape
    dev = x2.device
    if C != 96:
        xn, mean, rstd = layernorm_fwd_raw(x2, ln_g, ln_b, eps)
        qkv = linear_raw(xn, wqkv, bqkv)
        m = mask.detach().float().contiguous() if mask is not None else None
        o, lse = window_attn_fwd_raw(qkv, table, index_i32, m, n_img, H, W, num_heads, shift, scale, m is not None)
        del qkv
        y = linear_raw(o, wproj, bproj, res=x2, rowscale=rowscale, rows_per_scale=H * W)
        return y, xn, o, mean, rstd, lse
    nW = (H // 7) * (W // 7)
    lse = torch.empty((n_img * nW * num_heads * 49,), dtype=torch.float32, device=dev)
    y = torch.empty_like(x2)
    xn = torch.empty_like(x2) if save else None
    o = torch.empty_like(x2) if save else None
    mean = torch.empty(M, dtype=torch.float32, device=dev) if save else None
    rstd = torch.empty(M, dtype=torch.float32, device=dev) if save else None
    rc = _lib.load().fmmt_window_block_fwd(dtype_code(x2.dtype), n_img, H, W, C, num_heads, shift, _p(x2), _p(ln_g), _p(ln_b), float(eps),
                                           _p(wqkv), _p(bqkv), _p(wproj), _p(bproj), _p(table), _p(index_i32), float(scale), _p(rowscale),
                                           _p(y), _p(xn), _p(o), _p(mean), _p(rstd), _p(lse), _st())
    check(rc, f"fmmt_window_block_fwd(n={n_img},H={H},W={W},C={C},heads={num_heads},shift={shift})")
    return y, xn, o, mean, rstd, lse


class WindowBlockFn(Function):
    """x -> x + rowscale * proj(attn(LN(x) Wqkv^T + bqkv)) + bproj-term, forward = fmmt_window_block_fwd.  The backward runs on what the
    forward saved (LN(x), attention output, row statistics, log-sum-exp) and recomputes qkv with one GEMM."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, eps, wqkv, bqkv, wproj, bproj, table, index_i32, mask, n_img, H, W, num_heads, shift, scale, rowscale, grad_on=True):
        _need_cuda(x, "window_block")
        C = x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        train = grad_on and any(ctx.needs_input_grad)
        g, b = ln_w.detach().float().contiguous(), ln_b.detach().float().contiguous()
        tab = table.detach().float().contiguous()
        y, xn, o, mean, rstd, lse = window_block_raw(
            x2, n_img, H, W, num_heads, shift, g, b, eps, _lp(wqkv, x.dtype), bqkv.detach().float().contiguous() if bqkv is not None else None,
            _lp(wproj, x.dtype), bproj.detach().float().contiguous() if bproj is not None else None, tab, index_i32, scale, rowscale, train, mask)
        if train:
            m = mask.detach().float().contiguous() if mask is not None else None
            ctx.save_for_backward(x2, xn, o, mean, rstd, lse, g, wqkv, bqkv, wproj, tab, index_i32, m, rowscale)
        ctx.cfg = (n_img, H, W, C, num_heads, shift, float(scale), x.shape)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, xn, o, mean, rstd, lse, g, wqkv, bqkv, wproj, tab, index_i32, m, rowscale = ctx.saved_tensors
        dx, dg, db, dwq, dbq, dwp, dbp, dtable = window_block_backward(dy, x2, xn, o, mean, rstd, lse, g, wqkv, bqkv, wproj, tab, index_i32, m, rowscale, ctx.cfg)
        return (dx, dg, db, None, dwq, dbq, dwp, dbp if ctx.needs_input_grad[7] else None, dtable,
                None, None, None, None, None, None, None, None, None, None)


def window_block_backward(dy, x2, xn, o, mean, rstd, lse, g, wqkv, bqkv, wproj, tab, index_i32, m, rowscale, cfg):
    """backward of the fused attention half on what its forward saved; returns (dx, dgamma, dbeta, dWqkv, dbqkv, dWproj, dbproj, dtable)"""
    n_img, H, W, C, num_heads, shift, scale, xshape = cfg
    lib = _lib.load()
    dt = x2.dtype
    dy2 = dy.reshape(-1, C).contiguous()
    L = H * W
    dwp, dbp = wgrad_raw(dy2, o, True, rowscale, L)             # proj weight gradient (DropPath scale on dy)
    if _WBLOCK_BWD and (dt == torch.bfloat16 or (_WBLOCK_F32 and dt == torch.float32 and C == 96)) and (m is None or shift > 0):
        # (fp32: the same entry point runs the generic restatement of the recompute kernel, csrc/wattn_bwd_ref.hip)
        # attention core backward with q, k, v and d(attention output) re-formed inside the kernel (no qkv / d(out) tensors)
        dqkv = torch.empty((x2.shape[0], 3 * C), dtype=dt, device=x2.device)
        dtable = torch.empty_like(tab)
        nbytes = lib.fmmt_window_attn_bwd_workspace(num_heads)
        ws = _ws(nbytes, x2.device)
        wql, wpl, bqf = _lp(wqkv, dt), _lp(wproj, dt), (bqkv.detach().float().contiguous() if bqkv is not None else None)
        rc = lib.fmmt_window_block_attn_bwd(dtype_code(dt), n_img, H, W, C, num_heads, shift, _p(xn), _p(dy2), _p(o), _p(lse), _p(wql),
                                            _p(bqf), _p(wpl), _p(tab), _p(index_i32),
                                            scale, _p(rowscale), _p(dqkv), _p(dtable), _p(ws), nbytes, _st())
        check(rc, "fmmt_window_block_attn_bwd")
    else:
        do = linear_raw(dy2, _lp(wproj, dt, transpose=True), None, rowscale=rowscale, rows_per_scale=L)
        qkv = linear_raw(xn, _lp(wqkv, dt), bqkv.detach() if bqkv is not None else None)
        dqkv, dtable = window_attn_bwd_raw(qkv, o, do, lse, tab, index_i32, m, n_img, H, W, num_heads, shift, scale, m is not None)
        del qkv, do
    if _WBLOCK_LNBWD and (dt == torch.bfloat16 or (_WBLOCK_F32 and dt == torch.float32)) and C == 96:
        # d(LN out) = dqkv . Wqkv, LayerNorm' and the residual gradient in one launch (fmmt_linear_ln_bwd): d(LN out) is never written
        # (fp32: the generic instantiation of the same kernel, lin_lnbwd_ref_kernel -- what the gradient goldens of the fp32 model check)
        dx = torch.empty_like(x2)
        dg = torch.empty(C, dtype=torch.float32, device=x2.device)
        db = torch.empty(C, dtype=torch.float32, device=x2.device)
        nb2 = lib.fmmt_linear_ln_bwd_workspace(C)
        ws2 = _ws(nb2, x2.device)
        rc = lib.fmmt_linear_ln_bwd(dtype_code(dt), x2.shape[0], C, 3 * C, _p(dqkv), _p(_lp(wqkv, dt, transpose=True)), _p(x2), _p(mean), _p(rstd), _p(g),
                                    _p(dy2), _p(dx), _p(dg), _p(db), _p(ws2), nb2, _st())
        check(rc, "fmmt_linear_ln_bwd(window_block)")
        dwq, dbq = wgrad_raw(dqkv, xn, bqkv is not None)
        return dx.reshape(xshape), dg, db, dwq, dbq, dwp, dbp, dtable
    dxn = linear_raw(dqkv, _lp(wqkv, dt, transpose=True), None)
    dwq, dbq = wgrad_raw(dqkv, xn, bqkv is not None)
    del dqkv
    dx, dg, db = layernorm_bwd_raw(dxn, x2, mean, rstd, g, add=dy2)      # LayerNorm backward + the residual branch's gradient
    return dx.reshape(xshape), dg, db, dwq, dbq, dwp, dbp, dtable


def window_block(x, ln_w, ln_b, eps, wqkv, bqkv, wproj, bproj, table, index_i32, mask, n_img, H, W, num_heads, shift, scale, rowscale=None):
    return WindowBlockFn.apply(x, ln_w, ln_b, eps, wqkv, bqkv, wproj, bproj, table, index_i32, mask, n_img, H, W, num_heads, shift, scale, rowscale, torch.is_grad_enabled())


# ------------------------------------------------------------------------------------------------
# cross-modal multi-head attention core (time-major)
# ------------------------------------------------------------------------------------------------
def mha_fwd_ptrs(code, Lq, Lk, B, E, num_heads, qp, ldq, kp, vp, ldkv, scale, key_bias, dropout_p, seed_i, seedp, outp, ldo, device, what=""):
    """THE call of fmmt_mha_fwd, on addresses and row pitches (in elements): `code` the dtype code with its flags, q / k / v / out at qp / kp / vp /
    outp, key_bias a (B, Lk) fp32 tensor or None, seedp the address of the int64 seed word or None (then seed_i counts).  Returns the new lse."""
    lse = torch.empty((B * num_heads * Lq,), dtype=torch.float32, device=device)
    rc = _lib.load().fmmt_mha_fwd(code, Lq, Lk, B, E, num_heads, qp, ldq, kp, vp, ldkv, scale, _p(key_bias), dropout_p, seed_i, seedp, outp, ldo,
                                  _p(lse), _st())
    check(rc, f"fmmt_mha_fwd({what}Lq={Lq},Lk={Lk},B={B},E={E},heads={num_heads})")
    return lse


def mha_bwd_ptrs(code, Lq, Lk, B, E, num_heads, qp, ldq, kp, vp, ldkv, scale, key_bias, dropout_p, seed_i, seedp, outp, doutp, ldo, lse, dqp, dkp, dvp,
                 what=""):
    """THE call of fmmt_mha_bwd, as mha_fwd_ptrs; the gradients at dqp / dkp / dvp are laid out as their operands (pitches ldq / ldkv)"""
    rc = _lib.load().fmmt_mha_bwd(code, Lq, Lk, B, E, num_heads, qp, ldq, kp, vp, ldkv, scale, _p(key_bias), dropout_p, seed_i, seedp, outp, doutp, ldo,
                                  _p(lse), dqp, ldq, dkp, dvp, ldkv, _st())
    check(rc, f"fmmt_mha_bwd({what}Lq={Lq},Lk={Lk},B={B},E={E},heads={num_heads})")


def _cols(t, E, n):
    """the addresses of the first n E-wide column slices of a packed tensor (rows [a | b | ...])"""
    return tuple(t.data_ptr() + i * E * t.element_size() for i in range(n))


def _kv_ptrs(k, v, E):
    """(k address, v address, row pitch) of separate (Lk, B, E) k, v -- or of the packed (Lk, B, 2E) [k | v] projection k when v is None"""
    return (*_cols(k, E, 2), 2 * E) if v is None else (k.data_ptr(), v.data_ptr(), E)


def _packed_qkv(qkv, E):
    """(q address, its pitch, k address, v address, their pitch) of a packed projection, rows [q | k | v]"""
    qp, kp, vp = _cols(qkv, E, 3)
    return qp, 3 * E, kp, vp, 3 * E


def mha_fwd_raw(q, k, v, num_heads, scale, dropout_p, seed_i, seed_t, key_bias):
    """fmmt_mha_fwd on contiguous time-major operands; v None = k is the packed [k | v] projection.  Returns (out, lse)."""
    Lq, B, E = q.shape
    out = torch.empty_like(q)
    lse = mha_fwd_ptrs(dtype_code(q.dtype), Lq, k.shape[0], B, E, num_heads, _p(q), E, *_kv_ptrs(k, v, E), scale, key_bias, dropout_p, seed_i, _p(seed_t),
                       _p(out), E, q.device)
    return out, lse


def mha_bwd_raw(q, k, v, out, dout, lse, num_heads, scale, dropout_p, seed_i, seed_t, key_bias):
    """fmmt_mha_bwd; returns (dq, dk, dv) with dv None when k is the packed projection (dk then holds [dk | dv])"""
    Lq, B, E = q.shape
    dq, dk = torch.empty_like(q), torch.empty_like(k)
    dv = torch.empty_like(v) if v is not None else None
    mha_bwd_ptrs(dtype_code(q.dtype), Lq, k.shape[0], B, E, num_heads, _p(q), E, *_kv_ptrs(k, v, E), scale, key_bias, dropout_p, seed_i, _p(seed_t),
                 _p(out), _p(dout), E, lse, _p(dq), *_kv_ptrs(dk, dv, E)[:2])
    return dq, dk, dv


def mha_packed_fwd_raw(qkv, L, B, num_heads, scale, dropout_p, seed_i, seed_t, key_bias, batch_major=False):
    """fmmt_mha_fwd of SELF-attention over a packed projection, rows [q | k | v] of 3E columns: the three operands are column slices of it (row
    pitch 3E), nothing is transposed or copied.  Rows in (l, b) order, or with batch_major (dtype | FMMT_BATCH_MAJOR) in (b, l) order.
    Returns (out -- (B, L, E) batch-major, (L, B, E) otherwise --, lse)."""
    E = qkv.shape[-1] // 3
    out = torch.empty((B, L, E) if batch_major else (L, B, E), dtype=qkv.dtype, device=qkv.device)
    lse = mha_fwd_ptrs(dtype_code(qkv.dtype) | (_lib.BATCH_MAJOR if batch_major else 0), L, L, B, E, num_heads, *_packed_qkv(qkv, E), scale, key_bias,
                       dropout_p, seed_i, _p(seed_t), _p(out), E, qkv.device, "batch-major, " if batch_major else "self, ")
    return out, lse


def mha_packed_bwd_raw(qkv, L, B, out, dout, lse, num_heads, scale, dropout_p, seed_i, seed_t, key_bias, batch_major=False):
    """fmmt_mha_bwd of mha_packed_fwd_raw: the gradient of the packed projection, rows [dq | dk | dv], written in place by the two kernels"""
    E = qkv.shape[-1] // 3
    dqkv = torch.empty_like(qkv)
    mha_bwd_ptrs(dtype_code(qkv.dtype) | (_lib.BATCH_MAJOR if batch_major else 0), L, L, B, E, num_heads, *_packed_qkv(qkv, E), scale, key_bias,
                 dropout_p, seed_i, _p(seed_t), _p(out), _p(dout), E, lse, *_cols(dqkv, E, 3), "batch-major, " if batch_major else "self, ")
    return dqkv


def mha_packed_bm_fwd_raw(qkv, num_heads, scale, dropout_p, seed_i, seed_t, key_bias):
    """mha_packed_fwd_raw over a batch-major qkv (B, S, 3E).  Returns (out (B, S, E), lse)."""
    return mha_packed_fwd_raw(qkv, qkv.shape[1], qkv.shape[0], num_heads, scale, dropout_p, seed_i, seed_t, key_bias, batch_major=True)


def mha_packed_bm_bwd_raw(qkv, out, dout, lse, num_heads, scale, dropout_p, seed_i, seed_t, key_bias):
    """mha_packed_bwd_raw over a batch-major qkv (B, S, 3E): (B, S, 3E) = [dq | dk | dv]"""
    return mha_packed_bwd_raw(qkv, qkv.shape[1], qkv.shape[0], out, dout, lse, num_heads, scale, dropout_p, seed_i, seed_t, key_bias, batch_major=True)


# ------------------------------------------------------------------------------------------------
# the text encoder on real tokens only (include/fmmt_tokens.h)
# ------------------------------------------------------------------------------------------------
class TokenLayout:
    """how the leading real tokens of a (B, T) padding mask lie in `cap` packed rows (fmmt_token_layout): seq_len / seq_off int32 (B,), len64 int64 (B,)
    -- the counts pack_frames / unpack_rows take --, row_map int32 (cap,) = the padded-layout row of each packed row, counts int32 (2,) = [rows packed,
    non-zeros of the mask]; all on the device, none of it read on the host"""

    def __init__(self, B, T, cap, seq_len, seq_off, len64, row_map, counts):
        self.B, self.T, self.cap = B, T, cap
        self.seq_len, self.seq_off, self.len64, self.row_map, self.counts = seq_len, seq_off, len64, row_map, counts


def token_layout_raw(mask, cap):
    """fmmt_token_layout on a (B, T) mask (any dtype: non-zero = real token; converted to int32 with one launch unless it is int32 already)"""
    _need_cuda(mask, "token_layout")
    B, T = mask.shape
    m = mask.detach()
    m = m.contiguous() if m.dtype == torch.int32 else (m != 0).to(torch.int32)
    dev, cap = m.device, int(cap)
    i32 = torch.empty(2 * B + cap + 2, dtype=torch.int32, device=dev)          # one block: seq_len | seq_off | row_map | counts
    len64 = torch.empty(B, dtype=torch.int64, device=dev)
    lay = TokenLayout(B, T, cap, i32[:B], i32[B:2 * B], len64, i32[2 * B:2 * B + cap], i32[2 * B + cap:])
    check(_lib.load().fmmt_token_layout(B, T, cap, _p(m), _p(lay.seq_len), _p(lay.seq_off), _p(len64), _p(lay.row_map), _p(lay.counts), _st()),
          f"fmmt_token_layout(B={B},T={T},cap={cap})")
    return lay


def unpack_rows_raw(src, len64, B, L):
    """fmmt_unpack_rows: (cap, ...) packed rows + int64 (B,) counts -> (B, L, ...), zeros wherever no packed row belongs"""
    _need_cuda(src, "unpack_rows")
    s = src.detach().contiguous()
    row_bytes = s[0].numel() * s.element_size()
    out = torch.empty((B, L) + tuple(s.shape[1:]), dtype=s.dtype, device=s.device)
    check(_lib.load().fmmt_unpack_rows(B, L, s.shape[0], row_bytes, _p(s), _p(len64), _p(out), _st()),
          f"fmmt_unpack_rows(B={B},L={L},cap={s.shape[0]},row_bytes={row_bytes})")
    return out


class PackRowsFn(Function):
    """(B, T, ...) -> (cap, ...): every sequence's leading seq_len rows back to back, zeros behind (fmmt_pack_frames); backward: fmmt_unpack_rows"""

    @staticmethod
    def forward(ctx, x, lay):
        ctx.lay = lay
        return pack_frames(x, lay.len64, lay.cap)[0]

    @staticmethod
    def backward(ctx, dy):
        lay = ctx.lay
        return unpack_rows_raw(dy, lay.len64, lay.B, lay.T), None


class UnpackRowsFn(Function):
    """(cap, ...) -> (B, T, ...): the inverse of PackRowsFn, zeros at the padded positions (fmmt_unpack_rows); backward: fmmt_pack_frames"""

    @staticmethod
    def forward(ctx, x, lay):
        ctx.lay = lay
        return unpack_rows_raw(x, lay.len64, lay.B, lay.T)

    @staticmethod
    def backward(ctx, dy):
        lay = ctx.lay
        return pack_frames(dy, lay.len64, lay.cap)[0], None


def pack_rows(x, lay):
    return PackRowsFn.apply(x, lay)


def unpack_rows(x, lay):
    return UnpackRowsFn.apply(x, lay)


def mha_ragged_fwd_raw(qkv, lay, num_heads, scale, dropout_p, seed_i, seed_t):
    """fmmt_mha_fwd_ragged of self-attention over a packed projection (cap, 3E), rows [q | k | v].  Returns (out (cap, E), lse (B * heads * T,) in
    the padded call's layout: entries of padded queries are not written)"""
    E = qkv.shape[-1] // 3
    cap = qkv.shape[0]
    out = torch.empty((cap, E), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((lay.B * num_heads * lay.T,), dtype=torch.float32, device=qkv.device)
    check(_lib.load().fmmt_mha_fwd_ragged(dtype_code(qkv.dtype) | _lib.RAGGED, lay.T, lay.B, E, num_heads, cap, _p(lay.seq_off), _p(lay.seq_len),
                                          *_packed_qkv(qkv, E), scale, dropout_p, seed_i, _p(seed_t), _p(out), E, _p(lse), _st()),
          f"fmmt_mha_fwd_ragged(T={lay.T},B={lay.B},E={E},heads={num_heads},rows={cap})")
    return out, lse


def mha_ragged_bwd_raw(qkv, lay, out, dout, lse, num_heads, scale, dropout_p, seed_i, seed_t):
    """fmmt_mha_bwd_ragged of mha_ragged_fwd_raw: (cap, 3E) = [dq | dk | dv], zeros in the rows behind the last sequence"""
    E = qkv.shape[-1] // 3
    cap = qkv.shape[0]
    dqkv = torch.empty_like(qkv)
    dqp, dkp, dvp = _cols(dqkv, E, 3)
    check(_lib.load().fmmt_mha_bwd_ragged(dtype_code(qkv.dtype) | _lib.RAGGED, lay.T, lay.B, E, num_heads, cap, _p(lay.seq_off), _p(lay.seq_len),
                                          *_packed_qkv(qkv, E), scale, dropout_p, seed_i, _p(seed_t), _p(out), _p(dout), E, _p(lse), dqp, 3 * E, dkp, dvp,
                                          3 * E, _st()),
          f"fmmt_mha_bwd_ragged(T={lay.T},B={lay.B},E={E},heads={num_heads},rows={cap})")
    return dqkv


class MhaCoreFn(Function):
    """q: (Lq,B,E); kv: either a packed (Lk,B,2E) tensor [k | v] (v is None) or separate k, v (Lk,B,E)."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads, scale, dropout_p, seed, key_bias=None):
        _need_cuda(q, "multihead_attention")
        q = q.contiguous()
        Lq, B, E = q.shape
        k = k.contiguous()
        v = v.contiguous() if v is not None else None
        seed_i, seed_t = _seed_args(seed)
        if key_bias is not None:
            key_bias = key_bias.detach().to(torch.float32).contiguous()
            assert key_bias.shape == (B, k.shape[0]), f"key_bias must be (B, Lk) = ({B}, {k.shape[0]}), got {tuple(key_bias.shape)}"
        out, lse = mha_fwd_raw(q, k, v, num_heads, scale, dropout_p, seed_i, seed_t, key_bias)
        ctx.save_for_backward(q, k, v, out, lse, seed_t, key_bias)
        ctx.cfg = (num_heads, scale, dropout_p, seed_i)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, seed_t, key_bias = ctx.saved_tensors
        num_heads, scale, dropout_p, seed = ctx.cfg
        dq, dk, dv = mha_bwd_raw(q, k, v, out, dout.contiguous(), lse, num_heads, scale, dropout_p, seed, seed_t, key_bias)
        return dq, dk, dv, None, None, None, None, None


def _seg_seed(seed, seed_t, i):
    """(seed_i, address of the seed word) of segment i: word i of the device seeds, or the integer seed + i"""
    return (0, seed_t.data_ptr() + 8 * i) if seed_t is not None else (int(seed) + i, None)


class MhaSegFn(Function):
    """Several independent attention problems over ROW RANGES of one time-major query tensor q (Lq_tot,B,E) and one packed key / value
    projection kv (Lk_tot,B,2E): segment i = (q0, Lq, k0, Lk) lets queries q[q0:q0+Lq] attend to kv[k0:k0+Lk].  The two directions of a
    cross-modal encoder (CrossmodalTransformer.py:60-96 called twice by src/models.py:171-177 with the roles of the modalities swapped)
    share every per-token launch when their tokens are concatenated; only the attention core has to know where a sequence ends.  One
    fmmt_mha_fwd / fmmt_mha_bwd call per segment, reading and writing the row ranges in place (no slice copies, no cat).
    seed: python int, or an int64 CUDA tensor with one word per segment (graph-replay safe)."""

    @staticmethod
    def forward(ctx, q, kv, segs, num_heads, scale, dropout_p, seed):
        _need_cuda(q, "multihead_attention")
        q, kv = q.contiguous(), kv.contiguous()
        Lq_tot, B, E = q.shape
        assert kv.shape[1:] == (B, 2 * E), f"packed [k | v] projection expected, got {tuple(kv.shape)}"
        cover_q = sorted((s[0], s[0] + s[1]) for s in segs)
        cover_k = sorted((s[2], s[2] + s[3]) for s in segs)
        for cover, tot in ((cover_q, Lq_tot), (cover_k, kv.shape[0])):       # every row written exactly once (out, dq, dkv are torch.empty)
            assert cover[0][0] == 0 and cover[-1][1] == tot and all(a[1] == b[0] for a, b in zip(cover, cover[1:])), \
                f"segments must tile the rows: {segs}"
        seed_t = seed if isinstance(seed, torch.Tensor) else None
        assert seed_t is None or seed_t.numel() >= len(segs)
        es = q.element_size()
        out = torch.empty_like(q)
        lses = []
        for i, (q0, Lq, k0, Lk) in enumerate(segs):
            qo, kp = q0 * B * E * es, kv.data_ptr() + k0 * B * 2 * E * es
            lses.append(mha_fwd_ptrs(dtype_code(q.dtype), Lq, Lk, B, E, num_heads, q.data_ptr() + qo, E, kp, kp + E * es, 2 * E, scale, None, dropout_p,
                                     *_seg_seed(seed, seed_t, i), out.data_ptr() + qo, E, q.device, f"segment {i}: "))
        ctx.save_for_backward(q, kv, out, seed_t, *lses)
        ctx.cfg = (tuple(segs), num_heads, scale, dropout_p, 0 if seed_t is not None else int(seed))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, out, seed_t, *lses = ctx.saved_tensors
        segs, num_heads, scale, dropout_p, seed = ctx.cfg
        _, B, E = q.shape
        es = q.element_size()
        dout = dout.contiguous()
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        for i, (q0, Lq, k0, Lk) in enumerate(segs):
            qo, ko = q0 * B * E * es, k0 * B * 2 * E * es
            kp, dkp = kv.data_ptr() + ko, dkv.data_ptr() + ko
            mha_bwd_ptrs(dtype_code(q.dtype), Lq, Lk, B, E, num_heads, q.data_ptr() + qo, E, kp, kp + E * es, 2 * E, scale, None, dropout_p,
                         *_seg_seed(seed, seed_t, i), out.data_ptr() + qo, dout.data_ptr() + qo, E, lses[i], dq.data_ptr() + qo, dkp, dkp + E * es,
                         f"segment {i}: ")
        return dq, dkv, None, None, None, None, None


def mha_core_segments(q, kv, segs, num_heads, scale, dropout_p=0.0, seed=0):
    return MhaSegFn.apply(q, kv, tuple(tuple(int(v) for v in s) for s in segs), num_heads, scale, float(dropout_p),
                          seed if isinstance(seed, torch.Tensor) else int(seed))


def linear_seg3_raw(x2, ws, bs, y, seg_mode):
    """fmmt_linear_fwd_seg3 into y (M, N) from x2 (M, K) and three weights of one dtype.  seg_mode 1: y[:, s N/3:(s+1) N/3] = x2 ws[s]^T + bs[s],
    ws[s] (N/3, K), bs[s] fp32 or None; seg_mode 2: y = sum_s x2[:, s K/3:(s+1) K/3] ws[s]^T, ws[s] (N, K/3), no bias.  False (nothing launched)
    where the library does not take the shape -- FMMT_EINVAL: the caller issues three linear_raw calls instead."""
    (M, K), N = x2.shape, y.shape[1]
    rc = _lib.load().fmmt_linear_fwd_seg3(dtype_code(x2.dtype), M, N, K, _p(x2), K, _p(ws[0]), _p(ws[1]), _p(ws[2]), ws[0].shape[1], seg_mode,
                                          _p(bs[0]), _p(bs[1]), _p(bs[2]), _p(y), N, _st())
    if rc == _lib.FMMT_EINVAL:
        return False
    check(rc, f"fmmt_linear_fwd_seg3(M={M},N={N},K={K})")
    return True


class SelfAttnQkvFn(Function):
    """ctx = attention(x Wq^T + bq, x Wk^T + bk, x Wv^T + bv) for SELF-attention over x (L,B,H), time-major: MELDTransEncoder's SelfAttention
    (modules/Transformer.py:64-103, three nn.Linear over the same hidden states).  The three projections are ONE launch writing a packed
    (L*B, 3H) buffer (fmmt_linear_fwd_seg3, the three weight shadows as they are: no packed copy of the parameters exists), the attention
    core reads and -- backward -- writes that layout in place (row stride 3H), the input gradient dq Wq + dk Wk + dv Wv is one launch
    (K-segmented) and the three weight / bias gradients one (3H, H) / (3H) contraction returned as row slices.
    Per layer: 4 + 13 launches become 2 + 4.  Shapes the segmented kernel does not take (fp32 parity mode, many tokens) run the same
    arithmetic as three launches per step."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, num_heads, scale, dropout_p, seed, key_bias):
        _need_cuda(x, "self_attention")
        x = x.contiguous()
        L, B, H = x.shape
        M = L * B
        x2 = x.reshape(M, H)
        ws = [_lp(w, x.dtype) for w in (wq, wk, wv)]
        bs = [b.detach().float().contiguous() if b is not None else None for b in (bq, bk, bv)]
        qkv = torch.empty((M, 3 * H), dtype=x.dtype, device=x.device)
        if not linear_seg3_raw(x2, ws, bs, qkv, 1):
            for i in range(3):
                qkv[:, i * H:(i + 1) * H] = linear_raw(x2, ws[i], bs[i])
        seed_i, seed_t = _seed_args(seed)
        if key_bias is not None:
            key_bias = key_bias.detach().to(torch.float32).contiguous()
            assert key_bias.shape == (B, L)
        out, lse = mha_packed_fwd_raw(qkv, L, B, num_heads, scale, dropout_p, seed_i, seed_t, key_bias)
        ctx.save_for_backward(x2, qkv, out, lse, seed_t, key_bias, wq, wk, wv)
        ctx.cfg = (num_heads, scale, dropout_p, seed_i, (L, B, H), tuple(b is not None for b in bs))
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, qkv, out, lse, seed_t, key_bias, wq, wk, wv = ctx.saved_tensors
        num_heads, scale, dropout_p, seed_i, (L, B, H), has_b = ctx.cfg
        dqkv = mha_packed_bwd_raw(qkv, L, B, out, dout.contiguous(), lse, num_heads, scale, dropout_p, seed_i, seed_t, key_bias)
        dx = None
        if ctx.needs_input_grad[0]:
            wt = [_lp(w, x2.dtype, transpose=True) for w in (wq, wk, wv)]
            dx = torch.empty_like(x2)
            if not linear_seg3_raw(dqkv, wt, (None, None, None), dx, 2):
                dx = sum(linear_raw(dqkv[:, i * H:(i + 1) * H].contiguous(), wt[i], None) for i in range(3))
            dx = dx.reshape(L, B, H)
        dw, db = wgrad_raw(dqkv, x2, True)
        g = []
        for i in range(3):
            g += [dw[i * H:(i + 1) * H], db[i * H:(i + 1) * H] if has_b[i] else None]
        return (dx, *g, None, None, None, None, None)


def self_attention_qkv(x, wq, bq, wk, bk, wv, bv, num_heads, scale, dropout_p=0.0, seed=0, key_bias=None):
    return SelfAttnQkvFn.apply(x, wq, bq, wk, bk, wv, bv, num_heads, scale, float(dropout_p), seed if isinstance(seed, torch.Tensor) else int(seed), key_bias)


class SelectFramesFn(Function):
    """train_step.select_frames as one launch per direction (fmmt_select_frames_fwd / _bwd; train.py:75-114)."""

    @staticmethod
    def forward(ctx, preds, vision_inputs, vision_mask, num_imgs, threshold, n_valid=None):
        _need_cuda(preds, "select_frames")
        nF, NL = preds.shape
        B, Lv, D = vision_inputs.shape
        p32 = preds.detach().float().contiguous()
        vin = vision_inputs.detach().contiguous()
        vm = vision_mask.detach().float().contiguous()
        n = num_imgs.to(device=preds.device, dtype=torch.int64).contiguous()
        out = torch.empty((B, Lv, D + NL), dtype=vin.dtype, device=vin.device)
        new_mask = torch.empty((B, Lv), dtype=torch.float32, device=vin.device)
        src = torch.empty((B, Lv), dtype=torch.int32, device=vin.device)
        if n_valid is None:
            check(_lib.load().fmmt_select_frames_fwd(dtype_code(vin.dtype), nF, NL, B, Lv, D, _p(p32), _p(vin), _p(vm), _p(n), float(threshold), _p(out),
                                                     _p(new_mask), _p(src), _st()), f"fmmt_select_frames_fwd(nF={nF},B={B},Lv={Lv},D={D})")
        else:                                                # preds rows >= n_valid are padding of a fixed-capacity batch (pack_frames)
            check(_lib.load().fmmt_select_frames_fwd_n(dtype_code(vin.dtype), nF, NL, B, Lv, D, _p(p32), _p(vin), _p(vm), _p(n), float(threshold), _p(out),
                                                       _p(new_mask), _p(src), _p(_n_valid_word(n_valid, preds.device, "select_frames")), _st()),
                  f"fmmt_select_frames_fwd_n(nF={nF},B={B},Lv={Lv},D={D})")
        ctx.save_for_backward(src)
        ctx.cfg = (nF, NL, B, Lv, D, preds.dtype)
        new_mask = new_mask.to(vision_mask.dtype)
        ctx.mark_non_differentiable(new_mask)
        return out, new_mask

    @staticmethod
    def backward(ctx, dout, _dmask):
        (src,) = ctx.saved_tensors
        nF, NL, B, Lv, D, pdt = ctx.cfg
        dout = dout.contiguous()
        dp = torch.empty((nF, NL), dtype=torch.float32, device=dout.device)
        check(_lib.load().fmmt_select_frames_bwd(dtype_code(dout.dtype), nF, NL, B, Lv, D, _p(dout), _p(src), _p(dp), _st()), "fmmt_select_frames_bwd")
        return dp.to(pdt), None, None, None, None, None


def select_frames_fusable(preds, vision_inputs, vision_mask):
    B, Lv, _ = vision_inputs.shape
    return (preds.is_cuda and vision_inputs.is_cuda and not vision_inputs.requires_grad and vision_inputs.dtype in (torch.float32, torch.bfloat16)
            and preds.shape[0] <= 8192 and B <= 256 and B * Lv <= 8192 and preds.shape[1] <= 256)


def select_frames(preds, vision_inputs, vision_mask, num_imgs, threshold, n_valid=None):
    """n_valid (1-element int32 CUDA tensor, pack_frames' counts): rows of preds at or behind it are padding and take no part in the
    "did any face pass" decision; None: every row is a face"""
    return SelectFramesFn.apply(preds, vision_inputs, vision_mask, num_imgs, float(threshold), n_valid)


# ------------------------------------------------------------------------------------------------
# dropout seeds: one device draw per scope instead of one per call site
# ------------------------------------------------------------------------------------------------
import threading as _threading


class _SeedScopes(_threading.local):                         # per thread: a scope opened by one thread never feeds another thread's draws
    def __init__(self):
        self.stack = []


_SEED_TLS = _SeedScopes()


class seed_scope:
    """`with seed_scope(device, n):` -- ONE torch.randint launch draws n int64 seed words; every draw_seed() inside the scope hands out the next
    word as a 1-element view (a plain pointer offset for the kernels) instead of launching its own draw (~5 us each inside the fusion stack's
    chain of dependent launches, three per encoder layer).  Graph-replay safe like the single draws: the one randint is part of the graph.
    Nested scopes and draws beyond n fall back to individual draws."""

    def __init__(self, device, n: int = 64, enabled: bool = True):
        self.device, self.n, self.enabled = device, int(n), enabled
        self.words, self.next = None, 0

    def __enter__(self):
        if self.enabled:
            self.words = torch.randint(0, 2 ** 62, (self.n,), device=self.device, dtype=torch.int64)
            self.next = 0
            _SEED_TLS.stack.append(self)
        return self

    def __exit__(self, *exc):
        if self.enabled:
            _SEED_TLS.stack.remove(self)
        return False


def draw_seed(device, n: int = 1):
    """n (default 1) device-resident int64 dropout seed words (see seed_scope)"""
    if _SEED_TLS.stack:
        sc = _SEED_TLS.stack[-1]
        if sc.words.device == torch.device(device) and sc.next + n <= sc.n:
            w = sc.words[sc.next:sc.next + n]
            sc.next += n
            return w
    return torch.randint(0, 2 ** 62, (n,), device=device, dtype=torch.int64)


def mha_avg_weights(q, k, lse, num_heads, scale, dropout_p=0.0, seed=0, key_bias=None):
    """head-averaged post-dropout attention probabilities (B, Lq, Lk) fp32 -- the second return value of the reference's
    MultiheadAttention.forward (multihead_attention.py:133-134) -- recomputed from q, k (the (Lk,B,E) key projection or the packed
    (Lk,B,2E) [k | v] one), the log-sum-exp of the forward and the same seed (fmmt_mha_avg_weights).  No gradient."""
    q = q.detach().contiguous()
    k = k.detach().contiguous()
    Lq, B, E = q.shape
    Lk, ldkv = k.shape[0], k.shape[2]
    seed_i, seed_t = _seed_args(seed)
    kb = key_bias.detach().to(torch.float32).contiguous() if key_bias is not None else None
    w = torch.empty((B, Lq, Lk), dtype=torch.float32, device=q.device)
    rc = _lib.load().fmmt_mha_avg_weights(dtype_code(q.dtype), Lq, Lk, B, E, num_heads, _p(q), E, _p(k), ldkv, scale, _p(kb), float(dropout_p),
                                          seed_i, _p(seed_t), _p(lse), _p(w), _st())
    check(rc, f"fmmt_mha_avg_weights(Lq={Lq},Lk={Lk},B={B},E={E},heads={num_heads})")
    return w


def mha_core(q, k, v, num_heads, scale, dropout_p=0.0, seed=0, key_bias=None, return_lse=False):
    """seed: python int, or a 1-element int64 CUDA tensor read by the kernel at run time.
    key_bias: optional (B, Lk) additive logit bias (extended attention mask), no gradient.
    return_lse: also return the saved log-sum-exp (B*heads*Lq, fp32; no gradient) -- what mha_avg_weights needs."""
    out, lse = MhaCoreFn.apply(q, k, v, num_heads, scale, float(dropout_p), seed if isinstance(seed, torch.Tensor) else int(seed), key_bias)
    return (out, lse) if return_lse else out


# ------------------------------------------------------------------------------------------------
# PatchEmbed gather, BatchNorm1d, cross-modal input embedding
# ------------------------------------------------------------------------------------------------
class PatchIm2colFn(Function):
    @staticmethod
    def forward(ctx, img):
        _need_cuda(img, "patch_embed")
        lib = _lib.load()
        img = img.contiguous()
        n = img.shape[0]
        cols = torch.empty((n * 3136, 48), dtype=img.dtype, device=img.device)
        check(lib.fmmt_patch_im2col(dtype_code(img.dtype), n, _p(img), _p(cols), _st()), "fmmt_patch_im2col")
        ctx.n = n
        return cols

    @staticmethod
    def backward(ctx, dcols):
        lib = _lib.load()
        dcols = dcols.contiguous()
        dimg = torch.empty((ctx.n, 3, 224, 224), dtype=dcols.dtype, device=dcols.device)
        check(lib.fmmt_patch_col2im(dtype_code(dcols.dtype), ctx.n, _p(dcols), _p(dimg), _st()), "fmmt_patch_col2im")
        return dimg


def patch_im2col(img):
    return PatchIm2colFn.apply(img)


_RESIZE_TABLES: dict = {}        # (mode, in_size, device) -> (int32 table [224,8], float32 lut [256]) on the device


def resize_tables(mode: str, in_size: int, device):
    """Device copies of the host-built coefficient / normalisation tables of fmmt_patch_embed_u8 (built once per flavour,
    source size and device by the library's own host function -- never by the oracle)."""
    import ctypes
    key = (mode, int(in_size), str(device))
    hit = _RESIZE_TABLES.get(key)
    if hit is not None:
        return hit
    lib = _lib.load()
    code = {"pil": _lib.RESIZE_PIL, "cv2": _lib.RESIZE_CV2}.get(mode)
    if code is None:
        raise ValueError(f"resize flavour {mode!r}: 'pil' (utils/util.py:45, pinned) or 'cv2' (utils/dataset.py:57, unpinned)")
    tab = (ctypes.c_int32 * (224 * 8))()
    lut = (ctypes.c_float * 256)()
    check(lib.fmmt_resize_table(code, int(in_size), 224, ctypes.addressof(tab), ctypes.addressof(lut)), f"fmmt_resize_table({mode},{in_size})")
    rows = lib.fmmt_resize_band_rows(ctypes.addressof(tab), 224)
    if not 0 < rows <= 8:
        raise _lib.FmmtError(f"fmmt_patch_embed_u8: a band of 4 output rows touches {rows} source rows at size {in_size} (kernel limit 8)")
    t = torch.tensor(list(tab), dtype=torch.int32).view(224, 8).to(device)
    l = torch.tensor(list(lut), dtype=torch.float32).to(device)
    _RESIZE_TABLES[key] = (code, t, l)
    return _RESIZE_TABLES[key]


def _jitter_table(jitter, img_u8, what):
    """the (n, 8) int32 device table of augment.ColorJitter (include/fmmt_jitter.h), checked against the frames it is for"""
    if not torch.is_tensor(jitter) or jitter.dtype != torch.int32 or tuple(jitter.shape) != (img_u8.shape[0], _lib.JITTER_WORDS):
        got = f"{tuple(jitter.shape)} {jitter.dtype}" if torch.is_tensor(jitter) else type(jitter).__name__
        raise ValueError(f"{what}: the ColorJitter table is ({img_u8.shape[0]}, {_lib.JITTER_WORDS}) int32, one record per frame, got {got}")
    if jitter.device != img_u8.device:
        raise ValueError(f"{what}: the ColorJitter table is on {jitter.device}, the frames on {img_u8.device}")
    return jitter.contiguous()


def _augment_table(augment, jitter, img_u8, what):
    """the (n, 20) int32 device table of augment.AffWildAugment (include/fmmt_aug.h), checked against the frames it is for; not with a jitter table"""
    if jitter is not None:
        raise ValueError(f"{what}: jitter= (the MELD transform) and augment= (the Aff-Wild2 chain, which holds a jitter record of its own) exclude each other")
    if not torch.is_tensor(augment) or augment.dtype != torch.int32 or tuple(augment.shape) != (img_u8.shape[0], _lib.AUG_WORDS):
        got = f"{tuple(augment.shape)} {augment.dtype}" if torch.is_tensor(augment) else type(augment).__name__
        raise ValueError(f"{what}: the AffWildAugment table is ({img_u8.shape[0]}, {_lib.AUG_WORDS}) int32, one record per frame, got {got}")
    if augment.device != img_u8.device:
        raise ValueError(f"{what}: the AffWildAugment table is on {augment.device}, the frames on {img_u8.device}")
    return augment.contiguous()


def _augment_scratch(n, device):
    """the contrast statistic's words and the byte image of the frames (fmmt_aug_workspace_bytes: n x 224 x 224 x 3) a call writes, then reads"""
    return (torch.empty((n, _lib.JITTER_BANDS), dtype=torch.int32, device=device), torch.empty((n, 224, 224, 3), dtype=torch.uint8, device=device))


def patch_embed_u8(img_u8: torch.Tensor, mode: str, dtype, jitter=None, augment=None) -> torch.Tensor:
    """(n, S, S, 3) uint8 crops (image layout) -> (n*3136, 48) patch matrix of Normalize(ToTensor(resize_224(img))):
    the input pre-step fused into PatchEmbed's gather (no gradient: the input is integer data).
    jitter: None, or the (n, 8) int32 table of augment.ColorJitter -- the frame's brightness / contrast / saturation / hue operations on the resized
    bytes, in front of ToTensor (fmmt_patch_embed_u8_jitter: two launches; None is the call above, through the entry point above).
    augment: None, or the (n, 20) int32 table of augment.AffWildAugment -- the Aff-Wild2 chain grayscale / jitter / Gaussian blur on the resized
    bytes and RandomErasing's noise rectangle behind the Normalize table (fmmt_patch_embed_u8_aug: three launches); not together with jitter."""
    _need_cuda(img_u8, "patch_embed_u8")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[1] != img_u8.shape[2] or img_u8.shape[3] != 3:
        raise ValueError(f"patch_embed_u8 expects (n, S, S, 3) uint8 crops, got {tuple(img_u8.shape)} {img_u8.dtype}")
    if augment is not None:
        augment = _augment_table(augment, jitter, img_u8, "patch_embed_u8")
    img_u8 = img_u8.contiguous()
    n, S = img_u8.shape[0], img_u8.shape[1]
    code, tab, lut = resize_tables(mode, S, img_u8.device)
    cols = torch.empty((n * 3136, 48), dtype=dtype, device=img_u8.device)
    if augment is not None:
        partial, ws = _augment_scratch(n, img_u8.device)
        rc = _lib.load().fmmt_patch_embed_u8_aug(dtype_code(dtype), code, n, S, _p(img_u8), _p(tab), _p(lut), _p(augment), _p(partial), _p(ws), ws.numel(),
                                                 _p(cols), _st())
        check(rc, f"fmmt_patch_embed_u8_aug(n={n},S={S},{mode})")
        return cols
    if jitter is not None:
        jitter = _jitter_table(jitter, img_u8, "patch_embed_u8")
        partial = torch.empty((n, _lib.JITTER_BANDS), dtype=torch.int32, device=img_u8.device)
        rc = _lib.load().fmmt_patch_embed_u8_jitter(dtype_code(dtype), code, n, S, _p(img_u8), _p(tab), _p(lut), _p(jitter), _p(partial), _p(cols), _st())
        check(rc, f"fmmt_patch_embed_u8_jitter(n={n},S={S},{mode})")
        return cols
    rc = _lib.load().fmmt_patch_embed_u8(dtype_code(dtype), code, n, S, _p(img_u8), _p(tab), _p(lut), _p(cols), _st())
    check(rc, f"fmmt_patch_embed_u8(n={n},S={S},{mode})")
    return cols


_PATCH_U8_LN = True          # False: the uint8 pre-step and the projection + LayerNorm as two launches (patch matrix written, then read back)


class PatchEmbedU8LnFn(Function):
    """uint8 crops -> LayerNorm(PatchEmbed projection) in ONE launch (fmmt_patch_embed_u8_ln_fwd): the bicubic resize / ToTensor / Normalize / 4x4
    gather of the reference's host pre-step (utils/util.py:43-52, utils/dataset.py:47-69) feeds the projection's MFMA operand out of LDS
    (Swin_Transformer.py:392-422).  The patch matrix is written only when a backward will need it (the projection's weight gradient);
    backward = PatchProjLnFn's (the input is integer data: no input gradient)."""

    @staticmethod
    def forward(ctx, img_u8, mode, weight, bias, gamma, beta, eps, dtype, grad_on=True, jitter=None, augment=None):
        _need_cuda(img_u8, "patch_embed_u8_ln")
        if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[1] != img_u8.shape[2] or img_u8.shape[3] != 3:
            raise ValueError(f"patch_embed_u8 expects (n, S, S, 3) uint8 crops, got {tuple(img_u8.shape)} {img_u8.dtype}")
        if augment is not None:
            augment = _augment_table(augment, jitter, img_u8, "patch_embed_u8_ln")
        img_u8 = img_u8.contiguous()
        n, S = img_u8.shape[0], img_u8.shape[1]
        code, tab, lut = resize_tables(mode, S, img_u8.device)
        M, C = n * 3136, weight.shape[0]
        train = grad_on and any(ctx.needs_input_grad)
        dev = img_u8.device
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        y = torch.empty((M, C), dtype=dtype, device=dev)
        cols = torch.empty((M, 48), dtype=dtype, device=dev) if train else None
        x_pre = torch.empty_like(y) if train else None
        mean = torch.empty(M, dtype=torch.float32, device=dev) if train else None
        rstd = torch.empty(M, dtype=torch.float32, device=dev) if train else None
        bias32 = bias.detach().float().contiguous() if bias is not None else None
        if augment is not None:          # augment.AffWildAugment's table: statistic, pixels into the byte workspace, then this launch's finish (fmmt_patch_embed_u8_aug_ln_fwd)
            partial, ws = _augment_scratch(n, dev)
            rc = _lib.load().fmmt_patch_embed_u8_aug_ln_fwd(dtype_code(dtype), code, n, S, _p(img_u8), _p(tab), _p(lut), _p(augment), _p(partial), _p(ws),
                                                            ws.numel(), _p(_lp(weight, dtype)), _p(bias32), _p(g), _p(b), float(eps),
                                                            _p(cols), _p(x_pre), _p(y), _p(mean), _p(rstd), _st())
            check(rc, f"fmmt_patch_embed_u8_aug_ln_fwd(n={n},S={S},{mode})")
        elif jitter is not None:         # augment.ColorJitter's table: the same launch behind the contrast statistic's (fmmt_patch_embed_u8_jitter_ln_fwd)
            jitter = _jitter_table(jitter, img_u8, "patch_embed_u8_ln")
            partial = torch.empty((n, _lib.JITTER_BANDS), dtype=torch.int32, device=dev)
            rc = _lib.load().fmmt_patch_embed_u8_jitter_ln_fwd(dtype_code(dtype), code, n, S, _p(img_u8), _p(tab), _p(lut), _p(jitter), _p(partial),
                                                               _p(_lp(weight, dtype)), _p(bias32), _p(g), _p(b), float(eps),
                                                               _p(cols), _p(x_pre), _p(y), _p(mean), _p(rstd), _st())
            check(rc, f"fmmt_patch_embed_u8_jitter_ln_fwd(n={n},S={S},{mode})")
        else:
            rc = _lib.load().fmmt_patch_embed_u8_ln_fwd(dtype_code(dtype), code, n, S, _p(img_u8), _p(tab), _p(lut), _p(_lp(weight, dtype)),
                                                        _p(bias32), _p(g), _p(b), float(eps),
                                                        _p(cols), _p(x_pre), _p(y), _p(mean), _p(rstd), _st())
            check(rc, f"fmmt_patch_embed_u8_ln_fwd(n={n},S={S},{mode})")
        ctx.save_for_backward(cols, weight, x_pre, mean, rstd, g)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        cols, weight, x_pre, mean, rstd, g = ctx.saved_tensors
        dxp, dg, db = layernorm_bwd_raw(dy.contiguous(), x_pre, mean, rstd, g)
        dw, dbias = wgrad_raw(dxp, cols, ctx.has_bias)
        return None, None, dw.view_as(weight), dbias, dg, db, None, None, None, None, None


def patch_embed_u8_ln_fusable(img_u8, weight, norm, dtype):
    return (_PATCH_U8_LN and _PATCH_LN and norm is not None and img_u8.is_cuda and dtype in (torch.bfloat16, torch.float32)
            and tuple(weight.shape) == (96, 48) and tuple(norm.weight.shape) == (96,) and 0 < img_u8.shape[0] <= 65535      # the entry point's frame limit
            and not any(t.data_ptr() % 16 for t in (weight, norm.weight, norm.bias)))


def patch_embed_u8_ln(img_u8, mode, weight, bias, gamma, beta, eps, dtype, jitter=None, augment=None):
    return PatchEmbedU8LnFn.apply(img_u8, mode, weight, bias, gamma, beta, eps, dtype, torch.is_grad_enabled(), jitter, augment)


def batch_norm_1d_fwd_raw(x, g, b, running_mean, running_var, momentum, eps, training):
    n, C = x.shape
    y = torch.empty_like(x)
    sm = torch.empty(C, dtype=torch.float32, device=x.device)
    si = torch.empty(C, dtype=torch.float32, device=x.device)
    rc = _lib.load().fmmt_batchnorm1d_fwd(dtype_code(x.dtype), n, C, _p(x), _p(g), _p(b), _p(running_mean), _p(running_var),
                                          momentum, eps, int(training), _p(y), _p(sm), _p(si), _st())
    check(rc, "fmmt_batchnorm1d_fwd")
    return y, sm, si


def batch_norm_1d_bwd_raw(dy, x, g, sm, si, training):
    n, C = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    rc = _lib.load().fmmt_batchnorm1d_bwd(dtype_code(x.dtype), n, C, _p(dy), _p(x), _p(g), _p(sm), _p(si), int(training),
                                          _p(dx), _p(dg), _p(db), _st())
    check(rc, "fmmt_batchnorm1d_bwd")
    return dx, dg, db


class BatchNorm1dFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, training):
        _need_cuda(x, "batch_norm")
        x = x.contiguous()
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        y, sm, si = batch_norm_1d_fwd_raw(x, g, b, running_mean, running_var, momentum, eps, training)
        ctx.save_for_backward(x, g, sm, si)
        ctx.training = bool(training)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, sm, si = ctx.saved_tensors
        dx, dg, db = batch_norm_1d_bwd_raw(dy.contiguous(), x, g, sm, si, ctx.training)
        return dx, dg, db, None, None, None, None, None


def batch_norm_1d(x, gamma, beta, running_mean, running_var, momentum, eps, training, n_valid=None):
    """n_valid (1-element int32 CUDA tensor): only the first n_valid rows of x are real -- BatchNorm1dNFn; None: every row"""
    if n_valid is not None:
        return BatchNorm1dNFn.apply(x, gamma, beta, running_mean, running_var, momentum, eps, training, n_valid)
    return BatchNorm1dFn.apply(x, gamma, beta, running_mean, running_var, momentum, eps, training)


# ------------------------------------------------------------------------------------------------
# ragged frame counts behind one fixed shape (csrc/ragged.hip, include/fmmt_ragged.h)
# ------------------------------------------------------------------------------------------------
def _n_valid_word(n_valid, device, what):
    """the device word the *_n entry points read: an int32 CUDA tensor (its first element counts: pack_frames' `counts` passes as it is)"""
    if not torch.is_tensor(n_valid) or n_valid.dtype != torch.int32 or not n_valid.is_cuda or n_valid.device != device or n_valid.numel() < 1:
        raise _lib.FmmtError(f"{what}: n_valid must be an int32 tensor on {device} (the row count is read on the device: no host synchronisation)")
    return n_valid


def pack_frames(frames, num_imgs, capacity, counts=None):
    """(B, Lv, ...) frames as the loader pads them + num_imgs (B,) -> (packed (capacity, ...), counts): the real frames in the reference's
    concatenation order (train.py:60-71: torch.cat([frames[u, :n_u] for u])) at the front, zeros behind, in ONE launch without a host
    synchronisation (fmmt_pack_frames).  counts: int32 (2,) on the device, [min(total, capacity), total]; counts is what the n_valid arguments of
    batch_norm_1d / select_frames take.  Frames behind `capacity` are dropped (counts[1] > capacity).  Any dtype whose row is a multiple of 16 bytes.
    `counts` (None: a new tensor): the contiguous int32 (2,) device tensor the kernel writes into -- several captured graphs then share one."""
    _need_cuda(frames, "pack_frames")
    if frames.dim() < 3:
        raise ValueError(f"pack_frames expects (B, Lv, ...) frames, got {tuple(frames.shape)}")
    f = frames.detach().contiguous()
    B, Lv = f.shape[0], f.shape[1]
    row_bytes = f[0, 0].numel() * f.element_size()
    n = torch.as_tensor(num_imgs).to(device=f.device, dtype=torch.int64).contiguous()
    if tuple(n.shape) != (B,):
        raise ValueError(f"pack_frames: num_imgs must hold one count per utterance ({B}), got {tuple(n.shape)}")
    capacity = int(capacity)
    packed = torch.empty((max(capacity, 0),) + tuple(f.shape[2:]), dtype=f.dtype, device=f.device)
    if counts is None:
        counts = torch.empty(2, dtype=torch.int32, device=f.device)
    elif counts.dtype != torch.int32 or tuple(counts.shape) != (2,) or counts.device != f.device or not counts.is_contiguous():
        raise ValueError("pack_frames: counts must be a contiguous int32 (2,) tensor on the frames' device")
    check(_lib.load().fmmt_pack_frames(B, Lv, capacity, row_bytes, _p(f), _p(n), _p(packed), _p(counts), _st()),
          f"fmmt_pack_frames(B={B},Lv={Lv},capacity={capacity},row_bytes={row_bytes})")
    return packed, counts


class BatchNorm1dNFn(Function):
    """BatchNorm1d over the first n_valid rows of x (fmmt_batchnorm1d_fwd_n / _bwd_n): statistics and column sums over those rows, zeros in
    y / dx behind them.  One launch per direction, as BatchNorm1dFn; n_valid == x.shape[0] gives its bits."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, training, n_valid):
        _need_cuda(x, "batch_norm")
        x = x.contiguous()
        nv = _n_valid_word(n_valid, x.device, "batch_norm_1d")
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        n, C = x.shape
        y = torch.empty_like(x)
        sm = torch.empty(C, dtype=torch.float32, device=x.device)
        si = torch.empty(C, dtype=torch.float32, device=x.device)
        check(_lib.load().fmmt_batchnorm1d_fwd_n(dtype_code(x.dtype), n, C, _p(nv), _p(x), _p(g), _p(b), _p(running_mean), _p(running_var),
                                                 momentum, eps, int(training), _p(y), _p(sm), _p(si), _st()), "fmmt_batchnorm1d_fwd_n")
        ctx.save_for_backward(x, g, sm, si, nv)
        ctx.training = bool(training)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, sm, si, nv = ctx.saved_tensors
        n, C = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        check(_lib.load().fmmt_batchnorm1d_bwd_n(dtype_code(x.dtype), n, C, _p(nv), _p(dy), _p(x), _p(g), _p(sm), _p(si), int(ctx.training),
                                                 _p(dx), _p(dg), _p(db), _st()), "fmmt_batchnorm1d_bwd_n")
        return dx, dg, db, None, None, None, None, None, None


def posemb_scale_fwd_raw(x, table, scale):
    """fmmt_posemb_scale_fwd on a contiguous time-major x (L, B, E): y = scale * x + table[position], position of (t, b) = t + 1 where
    x[t, b, 0] != 0, else 0 (CrossmodalTransformer.py:63-66)"""
    L, B, E = x.shape
    y = torch.empty_like(x)
    check(_lib.load().fmmt_posemb_scale_fwd(dtype_code(x.dtype), L, B, E, _p(x), _p(table), scale, _p(y), _st()), f"fmmt_posemb_scale_fwd(L={L},B={B},E={E})")
    return y


def scale_raw(x, scale):
    """fmmt_scale: scale * x of a contiguous x"""
    y = torch.empty_like(x)
    check(_lib.load().fmmt_scale(dtype_code(x.dtype), x.numel(), _p(x), scale, _p(y), _st()), f"fmmt_scale(n={x.numel()})")
    return y


class PosEmbScaleFn(Function):
    @staticmethod
    def forward(ctx, x, table, scale):
        _need_cuda(x, "positional_embedding")
        ctx.scale = scale
        return posemb_scale_fwd_raw(x.contiguous(), table, scale)

    @staticmethod
    def backward(ctx, dy):
        return scale_raw(dy.contiguous(), ctx.scale), None, None


def posemb_scale(x, table, scale):
    return PosEmbScaleFn.apply(x, table, float(scale))


# ------------------------------------------------------------------------------------------------
# evaluation (csrc/eval.hip): forward only
# ------------------------------------------------------------------------------------------------
def _no_grad_only(what, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what} is forward only (evaluation): call it under torch.no_grad() or on detached tensors")


def emotion_head_raw(feats, w1, b1, w2, b2, tau, gumbel=None):
    """fmmt_emotion_head_fwd on tensors: feats (N, K) bf16 / fp32 (any row stride that is a multiple of 4), w1 (64, K), b1 (64,), w2 (NL, 64),
    b2 (NL,) fp32, gumbel (N, NL) fp32 or None.  Returns (preds (N, NL) fp32, importance (N,) fp32)."""
    _need_cuda(feats, "emotion_head")
    _no_grad_only("emotion_head", feats, w1, b1, w2, b2, gumbel)
    if feats.dim() != 2 or w1.dim() != 2 or w2.dim() != 2:
        raise _lib.FmmtError("emotion_head: feats (N, K), w1 (H, K), w2 (NL, H)")
    N, K = feats.shape
    H, NL = w1.shape[0], w2.shape[0]
    if w1.shape[1] != K or w2.shape[1] != H or b1.shape != (H,) or b2.shape != (NL,):
        raise _lib.FmmtError(f"emotion_head: shapes do not chain: feats {tuple(feats.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}")
    f = feats.detach()
    if f.stride(1) != 1 or f.stride(0) % 4 or f.stride(0) < K or f.data_ptr() % 16:
        f = _c16(f)
    ws = [t.detach() for t in (w1, b1, w2, b2)]
    if any(t.dtype != torch.float32 for t in ws):
        raise _lib.FmmtError("emotion_head: the head's parameters are read as fp32 (the module's own; no shadow copies)")
    ws = [t if t.is_contiguous() else t.contiguous() for t in ws]
    g = None
    if gumbel is not None:
        if tuple(gumbel.shape) != (N, NL):
            raise _lib.FmmtError(f"emotion_head: gumbel must be (N, NL) = ({N}, {NL}), got {tuple(gumbel.shape)}")
        g = gumbel.detach().float().contiguous()
    preds = torch.empty((N, NL), dtype=torch.float32, device=f.device)
    imp = torch.empty((N,), dtype=torch.float32, device=f.device)
    if N == 0:
        return preds, imp
    check(_lib.load().fmmt_emotion_head_fwd(dtype_code(f.dtype), N, K, H, NL, _p(f), f.stride(0), _p(ws[0]), _p(ws[1]), _p(ws[2]), _p(ws[3]), _p(g), float(tau),
                                            _p(preds), _p(imp), _st()), f"fmmt_emotion_head_fwd(N={N},K={K},H={H},NL={NL})")
    return preds, imp


def emotion_head(feats, linear, classifier, tau, gumbel=None):
    """The target-task head of SwinForAffwildClassification at inference (src/models.py:28-32) and the importance score of train.py:186-188 as one
    launch: `linear` / `classifier` are the module's two nn.Linear layers, `gumbel` the noise F.gumbel_softmax would add (None: no noise).
    Returns (preds, importance)."""
    return emotion_head_raw(feats, linear.weight, linear.bias, classifier.weight, classifier.bias, tau, gumbel)


def gumbel_noise(n, num_labels, device, dtype=torch.float32):
    """the noise of F.gumbel_softmax, drawn exactly as it draws it (one exponential_ over a logits-shaped tensor of the logits' dtype): the same
    generator state gives the same numbers"""
    return -torch.empty((n, num_labels), dtype=dtype, device=device).exponential_().log()


def eval_accumulate(logits, labels, acc, logits_out=None, out_offset=0, pred=True):
    """fmmt_eval_accumulate: logits (B, NL) bf16 / fp32, labels (B,) int64 (negative: ignored), acc: int64 CUDA tensor of 2 + NL * NL words --
    [0] the loss sum (the bits of a double), [1] the row count, [2:] the confusion matrix [label][argmax] -- updated in place; logits_out
    (capacity, NL) fp32 receives the rows at [out_offset, out_offset + B).  Returns the argmax (B,) int32, or None with pred=False."""
    _need_cuda(logits, "eval_accumulate")
    _no_grad_only("eval_accumulate", logits)
    if logits.dim() != 2 or labels.shape != (logits.shape[0],):
        raise _lib.FmmtError("eval_accumulate: logits (B, NL), labels (B,)")
    B, NL = logits.shape
    if acc.dtype != torch.int64 or acc.numel() != 2 + NL * NL or not acc.is_contiguous() or not acc.is_cuda:
        raise _lib.FmmtError(f"eval_accumulate: acc must be a contiguous int64 CUDA tensor of {2 + NL * NL} words")
    lg = logits.detach()
    if lg.stride(1) != 1:
        lg = lg.contiguous()
    lab = labels.detach().to(device=lg.device, dtype=torch.int64).contiguous()
    cap = 0
    if logits_out is not None:
        if logits_out.dtype != torch.float32 or logits_out.dim() != 2 or logits_out.shape[1] != NL or not logits_out.is_contiguous():
            raise _lib.FmmtError("eval_accumulate: logits_out must be a contiguous fp32 (capacity, NL) tensor")
        cap = logits_out.shape[0]
    out = torch.empty((B,), dtype=torch.int32, device=lg.device) if pred else None
    a = acc.data_ptr()
    check(_lib.load().fmmt_eval_accumulate(dtype_code(lg.dtype), B, NL, _p(lg), lg.stride(0), _p(lab), a, a + 8, a + 16, _p(out), _p(logits_out), int(out_offset),
                                           int(cap), _st()), f"fmmt_eval_accumulate(B={B},NL={NL})")
    return out


def _eval_collect_args(who, logits, labels, acc, cursor, logits_out, labels_out, pred_out):
    """the checks eval_accumulate_at and eval_accumulate_rows share -> (logits, labels, address of acc, capacity, B, NL)"""
    _need_cuda(logits, who)
    _no_grad_only(who, logits)
    if logits.dim() != 2 or labels.shape != (logits.shape[0],):
        raise _lib.FmmtError(f"{who}: logits (B, NL), labels (B,)")
    B, NL = logits.shape
    dev = logits.device
    if acc.dtype != torch.int64 or acc.numel() != 2 + NL * NL or not acc.is_contiguous() or acc.device != dev:
        raise _lib.FmmtError(f"{who}: acc must be a contiguous int64 CUDA tensor of {2 + NL * NL} words")
    if not torch.is_tensor(cursor) or cursor.dtype != torch.int64 or cursor.numel() != 1 or cursor.device != dev:
        raise _lib.FmmtError(f"{who}: cursor must be an int64 tensor of one word on the logits' device")
    if (not torch.is_tensor(logits_out) or logits_out.dtype != torch.float32 or logits_out.dim() != 2 or logits_out.shape[1] != NL
            or not logits_out.is_contiguous() or logits_out.device != dev):
        raise _lib.FmmtError(f"{who}: logits_out must be a contiguous fp32 (capacity, NL) tensor on the logits' device")
    cap = logits_out.shape[0]
    for name, t, dt in (("labels_out", labels_out, torch.int64), ("pred_out", pred_out, torch.int32)):
        if t is None and name == "pred_out":
            continue
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (cap,) or not t.is_contiguous() or t.device != dev:
            raise _lib.FmmtError(f"{who}: {name} must be a contiguous {dt} ({cap},) tensor on the logits' device (logits_out's rows)")
    lg = logits.detach()
    if lg.stride(1) != 1:
        lg = lg.contiguous()
    lab = labels.detach().to(device=dev, dtype=torch.int64).contiguous()
    return lg, lab, acc.data_ptr(), cap, B, NL


def eval_accumulate_at(logits, labels, acc, cursor, logits_out, labels_out, pred_out=None):
    """fmmt_eval_accumulate_at: eval_accumulate with the destination row in a DEVICE word, so that a captured graph collects a split.  cursor: int64
    CUDA tensor of one word; row i of the batch goes to logits_out[cursor + i] ((capacity, NL) fp32), labels_out[cursor + i] ((capacity,) int64)
    and pred_out[cursor + i] ((capacity,) int32, optional); rows at or behind the capacity are counted and stored nowhere; cursor += B on the
    device (cursor > capacity afterwards: the split overflowed).  The accumulators get the bits eval_accumulate gives them.  Returns None."""
    lg, lab, a, cap, B, NL = _eval_collect_args("eval_accumulate_at", logits, labels, acc, cursor, logits_out, labels_out, pred_out)
    check(_lib.load().fmmt_eval_accumulate_at(dtype_code(lg.dtype), B, NL, _p(lg), lg.stride(0), _p(lab), a, a + 8, a + 16, _p(cursor), _p(logits_out),
                                              _p(labels_out), _p(pred_out), int(cap), _st()), f"fmmt_eval_accumulate_at(B={B},NL={NL},capacity={cap})")


def eval_accumulate_rows(logits, labels, acc, cursor, n_rows, logits_out, labels_out, pred_out=None):
    """fmmt_eval_accumulate_rows: eval_accumulate_at for a batch PADDED to (B, NL), the number of rows that exist in a device word -- n_rows: int32
    CUDA tensor of one word, b = its value clamped to [0, B].  Rows i >= b are neither stored nor counted, whatever their label; cursor += b on the
    device.  With n_rows == B: the bits of eval_accumulate_at.  A captured graph re-reads the word on every replay.  Returns None."""
    lg, lab, a, cap, B, NL = _eval_collect_args("eval_accumulate_rows", logits, labels, acc, cursor, logits_out, labels_out, pred_out)
    if not torch.is_tensor(n_rows) or n_rows.dtype != torch.int32 or n_rows.numel() != 1 or n_rows.device != lg.device:
        raise _lib.FmmtError("eval_accumulate_rows: n_rows must be an int32 tensor of one word on the logits' device")
    check(_lib.load().fmmt_eval_accumulate_rows(dtype_code(lg.dtype), B, NL, _p(lg), lg.stride(0), _p(lab), a, a + 8, a + 16, _p(cursor), _p(n_rows),
                                                _p(logits_out), _p(labels_out), _p(pred_out), int(cap), _st()),
          f"fmmt_eval_accumulate_rows(B={B},NL={NL},capacity={cap})")


def eval_merge(words, results, truths, words_out, results_out, truths_out):
    """fmmt_eval_merge: W gathered shards of an evaluation split -> the split, one launch.  words (W, 2 + NL * NL + 1) int64 (per rank: loss-sum bits,
    count, confusion, cursor -- MeldMetrics.words), results (W, cap, NL) fp32, truths (W, cap) int64; words_out (2 + NL * NL + 1,), results_out
    (out_cap, NL), truths_out (out_cap,) receive the merged split in MeldMetrics's layout: rank r's first min(cursor_r, cap) rows behind those of the
    ranks in front of it, rows behind the total untouched, the loss sums added in rank order, cursor_out > out_cap when a rank or the outputs
    overflowed (include/fmmt_eval_shard.h).  All contiguous, on one device; 1 <= W <= 64.  Returns None."""
    _need_cuda(words, "eval_merge")
    dev = words.device
    if results.dim() != 3 or results.dtype != torch.float32:
        raise _lib.FmmtError("eval_merge: results (W, cap, NL) fp32")
    W, cap, NL = results.shape
    nw = 2 + NL * NL + 1
    if results_out.dim() != 2 or results_out.dtype != torch.float32 or results_out.shape[1] != NL:
        raise _lib.FmmtError(f"eval_merge: results_out (out_cap, {NL}) fp32")
    out_cap = results_out.shape[0]
    for name, t, dt, shape in (("words", words, torch.int64, (W, nw)), ("results", results, torch.float32, (W, cap, NL)), ("truths", truths, torch.int64, (W, cap)),
                               ("words_out", words_out, torch.int64, (nw,)), ("results_out", results_out, torch.float32, (out_cap, NL)),
                               ("truths_out", truths_out, torch.int64, (out_cap,))):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise _lib.FmmtError(f"eval_merge: {name} must be a contiguous {dt} {shape} tensor on the device of `words`")
    if not 1 <= W <= 64 or not 1 <= NL <= 8:
        raise _lib.FmmtError("eval_merge: 1 <= W <= 64 ranks, 1 <= NL <= 8 classes")
    # an empty buffer has no address: the kernel touches neither at cap == 0 / out_cap == 0, the entry point wants non-NULL pointers
    check(_lib.load().fmmt_eval_merge(W, NL, int(cap), int(out_cap), _p(words), _p(results) or _p(words), _p(truths) or _p(words), _p(words_out),
                                      _p(results_out) or _p(words_out), _p(truths_out) or _p(words_out), _st()),
          f"fmmt_eval_merge(W={W},NL={NL},cap={cap},out_cap={out_cap})")


# ------------------------------------------------------------------------------------------------
# additive-attention pooling -> dropout -> classifier -> cross-entropy (csrc/pool_head.hip)
# ------------------------------------------------------------------------------------------------
def _pool_head_args(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels):
    _need_cuda(h, "pool_head_loss")
    if h.dim() != 3 or ph.shape != h.shape or ph.dtype != h.dtype:
        raise _lib.FmmtError(f"pool_head_loss: h and ph must be (B, L, H) tensors of one dtype, got {tuple(h.shape)} {h.dtype} / {tuple(ph.shape)} {ph.dtype}")
    B, L, H = h.shape
    if cls_w.dim() != 2 or cls_w.shape[1] != H:
        raise _lib.FmmtError(f"pool_head_loss: the classifier weight must be (NL, {H}), got {tuple(cls_w.shape)}")
    NL = cls_w.shape[0]
    if qq.numel() != H or value_w.numel() != H or value_b.numel() != 1 or tuple(mask.shape) != (B, L) or cls_b.shape != (NL,) or tuple(labels.shape) != (B,):
        raise _lib.FmmtError(f"pool_head_loss: qq / value_w ({H},), value_b (1,), mask ({B}, {L}), cls_b ({NL},), labels ({B},) expected")
    # contiguous fp32 tensors (the modules' parameters, the mask, a qq already cast by the caller) pass through as views: no launch
    f32 = [_c16(t.detach().reshape(-1).float()) for t in (qq, value_w, value_b, mask, cls_w, cls_b)]
    lab = labels.detach().to(device=h.device, dtype=torch.int64).contiguous()
    return (B, L, H, NL), _c16(h.detach()), _c16(ph.detach()), f32, lab


def pool_head_fwd_raw(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p=0.0, seed=0, valid_mean=False):
    """fmmt_pool_head_fwd on tensors (no autograd).  h, ph (B, L, H) bf16 / fp32; the rest as the modules hold them (any shape with the right element
    count, read as fp32); seed: python int or a 1-element int64 CUDA tensor.  Returns (loss (), logits (B, NL), alpha (B, L), pooled (B, H), keep (B, H)),
    all fp32.  valid_mean: fmmt_pool_head_fwd_rows -- the mean over the rows whose label lies in [0, NL) -- and a sixth result, n_rows (1,) int32, the
    device word pool_head_bwd_raw takes."""
    (B, L, H, NL), h2, ph2, (q, vw, vb, mk, cw, cb), lab = _pool_head_args(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels)
    dev = h2.device
    lib = _lib.load()
    logits = torch.empty((B, NL), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, L), dtype=torch.float32, device=dev)
    pooled, keep = torch.empty((B, H), dtype=torch.float32, device=dev), torch.empty((B, H), dtype=torch.float32, device=dev)
    nbytes = lib.fmmt_pool_head_bwd_workspace(B, L, H)
    ws = _ws(nbytes, dev)
    seed_i, seed_t = _seed_args(seed)
    if valid_mean:
        n_rows = torch.empty((1,), dtype=torch.int32, device=dev)
        check(lib.fmmt_pool_head_fwd_rows(dtype_code(h2.dtype), B, L, H, NL, _p(h2), _p(ph2), _p(q), _p(vw), _p(vb), _p(mk), _p(cw), _p(cb), _p(lab), float(p),
                                          seed_i, _p(seed_t), _p(logits), _p(loss), _p(alpha), _p(pooled), _p(keep), _p(n_rows), _p(ws), nbytes, _st()),
              f"fmmt_pool_head_fwd_rows(B={B},L={L},H={H},NL={NL})")
        return loss, logits, alpha, pooled, keep, n_rows
    check(lib.fmmt_pool_head_fwd(dtype_code(h2.dtype), B, L, H, NL, _p(h2), _p(ph2), _p(q), _p(vw), _p(vb), _p(mk), _p(cw), _p(cb), _p(lab), float(p), seed_i,
                                 _p(seed_t), _p(logits), _p(loss), _p(alpha), _p(pooled), _p(keep), _p(ws), nbytes, _st()),
          f"fmmt_pool_head_fwd(B={B},L={L},H={H},NL={NL})")
    return loss, logits, alpha, pooled, keep


def pool_head_bwd_raw(dloss, h, ph, qq, value_w, cls_w, labels, logits, alpha, pooled, keep, n_rows=None):
    """fmmt_pool_head_bwd on tensors: (dh_pool, dph) in h's dtype, (dqq (H,), dv (H,), dvb (1,), dW (NL, H), db (NL,)) fp32.  n_rows (the int32 device
    word of pool_head_fwd_raw(..., valid_mean=True)): fmmt_pool_head_bwd_rows, which reads it on the device."""
    B, L, H = h.shape
    NL = cls_w.shape[0]
    dev = h.device
    lib = _lib.load()
    h2, ph2 = _c16(h.detach()), _c16(ph.detach())
    q, vw, cw = (_c16(t.detach().reshape(-1).float()) for t in (qq, value_w, cls_w))
    dl = dloss.detach().reshape(-1).float().contiguous()
    dh, dph = torch.empty_like(h2), torch.empty_like(h2)
    dqq, dv = torch.empty((H,), dtype=torch.float32, device=dev), torch.empty((H,), dtype=torch.float32, device=dev)
    dvb = torch.empty((1,), dtype=torch.float32, device=dev)
    dW, db = torch.empty((NL, H), dtype=torch.float32, device=dev), torch.empty((NL,), dtype=torch.float32, device=dev)
    nbytes = lib.fmmt_pool_head_bwd_workspace(B, L, H)
    ws = _ws(nbytes, dev)
    if n_rows is not None:
        if n_rows.dtype != torch.int32 or n_rows.device != dev or n_rows.numel() < 1:
            raise _lib.FmmtError(f"pool_head_loss: n_rows must be the int32 word of the forward on {dev}")
        check(lib.fmmt_pool_head_bwd_rows(dtype_code(h2.dtype), B, L, H, NL, _p(dl), _p(h2), _p(ph2), _p(q), _p(vw), _p(cw), _p(labels), _p(logits), _p(alpha),
                                          _p(pooled), _p(keep), _p(n_rows), _p(dh), _p(dph), _p(dqq), _p(dv), _p(dvb), _p(dW), _p(db), _p(ws), nbytes, _st()),
              f"fmmt_pool_head_bwd_rows(B={B},L={L},H={H},NL={NL})")
        return dh, dph, dqq, dv, dvb, dW, db
    check(lib.fmmt_pool_head_bwd(dtype_code(h2.dtype), B, L, H, NL, _p(dl), _p(h2), _p(ph2), _p(q), _p(vw), _p(cw), _p(labels), _p(logits), _p(alpha), _p(pooled),
                                 _p(keep), _p(dh), _p(dph), _p(dqq), _p(dv), _p(dvb), _p(dW), _p(db), _p(ws), nbytes, _st()),
          f"fmmt_pool_head_bwd(B={B},L={L},H={H},NL={NL})")
    return dh, dph, dqq, dv, dvb, dW, db


def _criterion_args(who, criterion, NL, dev):
    """(class weights or None, eps) of a criterion -- anything with `.weight` (None, or the fp32 (NL,) tensor on `dev` the launches address) and
    `.label_smoothing`, train_step.Criterion being the one the steps hold"""
    w, eps = criterion.weight, float(criterion.label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise _lib.FmmtError(f"{who}: label_smoothing must lie in [0, 1), got {eps}")
    if w is not None and (not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) != (NL,) or not w.is_contiguous() or w.device != dev):
        raise _lib.FmmtError(f"{who}: the class weights must be a contiguous fp32 ({NL},) tensor on {dev}")
    return w, eps


def pool_head_fwd_crit_raw(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p, seed, weight, eps):
    """fmmt_pool_head_fwd_crit on tensors (no autograd): pool_head_fwd_raw(..., valid_mean=True) with the class-weighted, label-smoothed loss of
    include/fmmt_loss.h -- weight: None or fp32 (NL,) on the device, eps: float.  The sixth result is den (1,) fp32, the device word
    pool_head_bwd_crit_raw takes."""
    (B, L, H, NL), h2, ph2, (q, vw, vb, mk, cw, cb), lab = _pool_head_args(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels)
    dev = h2.device
    lib = _lib.load()
    logits = torch.empty((B, NL), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    alpha = torch.empty((B, L), dtype=torch.float32, device=dev)
    pooled, keep = torch.empty((B, H), dtype=torch.float32, device=dev), torch.empty((B, H), dtype=torch.float32, device=dev)
    den = torch.empty((1,), dtype=torch.float32, device=dev)
    nbytes = lib.fmmt_pool_head_bwd_workspace(B, L, H)
    ws = _ws(nbytes, dev)
    seed_i, seed_t = _seed_args(seed)
    check(lib.fmmt_pool_head_fwd_crit(dtype_code(h2.dtype), B, L, H, NL, _p(h2), _p(ph2), _p(q), _p(vw), _p(vb), _p(mk), _p(cw), _p(cb), _p(lab), float(p),
                                      seed_i, _p(seed_t), _p(logits), _p(loss), _p(alpha), _p(pooled), _p(keep), _p(weight), float(eps), _p(den), _p(ws), nbytes,
                                      _st()), f"fmmt_pool_head_fwd_crit(B={B},L={L},H={H},NL={NL})")
    return loss, logits, alpha, pooled, keep, den


def pool_head_bwd_crit_raw(dloss, h, ph, qq, value_w, cls_w, labels, logits, alpha, pooled, keep, weight, eps, den):
    """fmmt_pool_head_bwd_crit on tensors: pool_head_bwd_raw's results under the criterion of the forward; den: the fp32 word it wrote"""
    B, L, H = h.shape
    NL = cls_w.shape[0]
    dev = h.device
    lib = _lib.load()
    h2, ph2 = _c16(h.detach()), _c16(ph.detach())
    q, vw, cw = (_c16(t.detach().reshape(-1).float()) for t in (qq, value_w, cls_w))
    dl = dloss.detach().reshape(-1).float().contiguous()
    if den.dtype != torch.float32 or den.device != dev or den.numel() < 1:
        raise _lib.FmmtError(f"pool_head_loss: den must be the fp32 word of the forward on {dev}")
    dh, dph = torch.empty_like(h2), torch.empty_like(h2)
    dqq, dv = torch.empty((H,), dtype=torch.float32, device=dev), torch.empty((H,), dtype=torch.float32, device=dev)
    dvb = torch.empty((1,), dtype=torch.float32, device=dev)
    dW, db = torch.empty((NL, H), dtype=torch.float32, device=dev), torch.empty((NL,), dtype=torch.float32, device=dev)
    nbytes = lib.fmmt_pool_head_bwd_workspace(B, L, H)
    ws = _ws(nbytes, dev)
    check(lib.fmmt_pool_head_bwd_crit(dtype_code(h2.dtype), B, L, H, NL, _p(dl), _p(h2), _p(ph2), _p(q), _p(vw), _p(cw), _p(labels), _p(logits), _p(alpha),
                                      _p(pooled), _p(keep), _p(weight), float(eps), _p(den), _p(dh), _p(dph), _p(dqq), _p(dv), _p(dvb), _p(dW), _p(db), _p(ws),
                                      nbytes, _st()), f"fmmt_pool_head_bwd_crit(B={B},L={L},H={H},NL={NL})")
    return dh, dph, dqq, dv, dvb, dW, db


class PoolHeadLossFn(Function):
    """(loss, logits) of the V-only classifier's tail behind ph = P h + b_P and qq = Q query_vector + b_Q (modules/Transformer.py:24-45, src/models.py:219-221,
    train.py:258): two launches forward, two backward (csrc/pool_head.hip).  The gradient flows from the loss; the logits are returned for the caller's
    bookkeeping and are not differentiable.  Saved: alpha, the pooled vector, the keep mask (the dropout is not replayed: B x H values).
    valid_mean: the fmmt_pool_head_*_rows pair (mean over the labelled rows); the row count stays a device word in the context.
    criterion ((class weights or None, eps), of _criterion_args): the fmmt_pool_head_*_crit pair -- the weighted mean over the labelled rows, its
    divisor a float device word in the context; valid_mean is then implied."""

    @staticmethod
    def forward(ctx, h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p, seed, valid_mean=False, criterion=None):
        _need_cuda(h, "pool_head_loss")
        lab = labels.detach().to(device=h.device, dtype=torch.int64).contiguous()      # once: the raw call below finds it as it needs it
        ctx.crit = criterion
        if criterion is not None:
            loss, logits, alpha, pooled, keep, ctx.n_rows = pool_head_fwd_crit_raw(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, lab, p, seed, *criterion)
        elif valid_mean:
            loss, logits, alpha, pooled, keep, ctx.n_rows = pool_head_fwd_raw(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, lab, p, seed, True)
        else:
            loss, logits, alpha, pooled, keep = pool_head_fwd_raw(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, lab, p, seed)
            ctx.n_rows = None
        ctx.save_for_backward(h, ph, qq, value_w, cls_w, lab, logits, alpha, pooled, keep)
        ctx.shapes = (qq.shape, value_w.shape, value_b.shape, cls_w.shape, cls_b.shape)
        ctx.dtypes = (qq.dtype, value_w.dtype, value_b.dtype, cls_w.dtype, cls_b.dtype)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        h, ph, qq, value_w, cls_w, lab, logits, alpha, pooled, keep = ctx.saved_tensors
        if ctx.crit is not None:
            dh, dph, dqq, dv, dvb, dW, db = pool_head_bwd_crit_raw(dloss, h, ph, qq, value_w, cls_w, lab, logits, alpha, pooled, keep, *ctx.crit, ctx.n_rows)
        else:
            dh, dph, dqq, dv, dvb, dW, db = pool_head_bwd_raw(dloss, h, ph, qq, value_w, cls_w, lab, logits, alpha, pooled, keep, ctx.n_rows)
        sh, dt = ctx.shapes, ctx.dtypes
        outs = [g.reshape(s).to(d) for g, s, d in zip((dqq, dv, dvb, dW, db), sh, dt)]
        return dh.reshape(h.shape), dph.reshape(h.shape), outs[0], outs[1], outs[2], None, outs[3], outs[4], None, None, None, None, None


def pool_head_loss(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p=0.0, seed=0, valid_mean=False, criterion=None):
    """-> (loss, logits): mean cross-entropy of classifier(dropout(additive-attention pooling of h)) and the logits (see PoolHeadLossFn).  valid_mean:
    the mean runs over the rows whose label lies in [0, NL) (F.cross_entropy's ignore_index rule for a padded batch) instead of over all B rows.
    criterion (None: the launches above; else an object with `.weight` and `.label_smoothing`, train_step.Criterion): the class-weighted,
    label-smoothed mean of include/fmmt_loss.h over the labelled rows (fmmt_pool_head_fwd_crit / _bwd_crit)."""
    if criterion is None:
        return PoolHeadLossFn.apply(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p, seed, bool(valid_mean))
    crit = _criterion_args("pool_head_loss", criterion, cls_w.shape[0], h.device)
    return PoolHeadLossFn.apply(h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p, seed, True, crit)


# ------------------------------------------------------------------------------------------------
# class-weighted, label-smoothed cross-entropy of (B, NL) logits (csrc/ce_loss.hip, include/fmmt_loss.h)
# ------------------------------------------------------------------------------------------------
def _ce_args(logits, labels, weight):
    _need_cuda(logits, "ce_loss")
    if logits.dim() != 2 or tuple(labels.shape) != (logits.shape[0],):
        raise _lib.FmmtError(f"ce_loss: logits (B, NL) and labels (B,) expected, got {tuple(logits.shape)} / {tuple(labels.shape)}")
    B, NL = logits.shape
    if not 1 <= NL <= _lib.CE_MAXNL or not 1 <= B <= _lib.CE_MAXB:
        raise _lib.FmmtError(f"ce_loss: 1 <= NL <= {_lib.CE_MAXNL} classes and 1 <= B <= {_lib.CE_MAXB} rows, got B={B}, NL={NL}")
    lg = logits.detach()
    if lg.stride(1) != 1 or lg.stride(0) < NL:
        lg = lg.contiguous()
    dev = lg.device
    if weight is not None and (not torch.is_tensor(weight) or weight.dtype != torch.float32 or tuple(weight.shape) != (NL,) or not weight.is_contiguous()
                               or weight.device != dev):
        raise _lib.FmmtError(f"ce_loss: the class weights must be a contiguous fp32 ({NL},) tensor on {dev}")
    lab = labels.detach().to(device=dev, dtype=torch.int64).contiguous()
    return B, NL, lg, lab


def ce_fwd_raw(logits, labels, weight=None, label_smoothing=0.0):
    """fmmt_ce_fwd on tensors (no autograd): logits (B, NL) bf16 / fp32 (rows may be a strided view, stride(0) >= NL), labels (B,) (a label outside
    [0, NL) is ignored), weight None or fp32 (NL,) on the device.  Returns (loss (), den (1,)), fp32 device words; one launch, no host read."""
    B, NL, lg, lab = _ce_args(logits, labels, weight)
    loss = torch.empty((), dtype=torch.float32, device=lg.device)
    den = torch.empty((1,), dtype=torch.float32, device=lg.device)
    check(_lib.load().fmmt_ce_fwd(dtype_code(lg.dtype), B, NL, _p(lg), lg.stride(0), _p(lab), _p(weight), float(label_smoothing), _p(loss), _p(den), _st()),
          f"fmmt_ce_fwd(B={B},NL={NL})")
    return loss, den


def ce_bwd_raw(dloss, logits, labels, weight, label_smoothing, den):
    """fmmt_ce_bwd on tensors: d(logits) (B, NL), contiguous, in the logits' dtype; dloss and den (the word ce_fwd_raw wrote) are read on the device"""
    B, NL, lg, lab = _ce_args(logits, labels, weight)
    dev = lg.device
    if den.dtype != torch.float32 or den.device != dev or den.numel() < 1:
        raise _lib.FmmtError(f"ce_loss: den must be the fp32 word of the forward on {dev}")
    dl = dloss.detach().reshape(-1).float().contiguous()
    out = torch.empty((B, NL), dtype=lg.dtype, device=dev)
    check(_lib.load().fmmt_ce_bwd(dtype_code(lg.dtype), B, NL, _p(lg), lg.stride(0), _p(lab), _p(weight), float(label_smoothing), _p(dl), _p(den), _p(out), NL,
                                  _st()), f"fmmt_ce_bwd(B={B},NL={NL})")
    return out


class CeLossFn(Function):
    """torch.nn.CrossEntropyLoss(weight, label_smoothing, reduction='mean') of (B, NL) logits (train.py:26,135 with the criterion a run chose), one
    launch forward and one backward (csrc/ce_loss.hip); den == 0 gives loss 0 and a zero gradient (include/fmmt_loss.h).  The weights are read on
    the device at launch time: a captured graph follows a weight tensor changed in place."""

    @staticmethod
    def forward(ctx, logits, labels, weight, label_smoothing):
        loss, den = ce_fwd_raw(logits, labels, weight, label_smoothing)
        ctx.save_for_backward(logits, labels, den)
        ctx.weight, ctx.eps = weight, float(label_smoothing)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, labels, den = ctx.saved_tensors
        return ce_bwd_raw(dloss, logits, labels, ctx.weight, ctx.eps, den), None, None, None


def ce_loss(logits, labels, weight=None, label_smoothing=0.0):
    """-> loss (): the class-weighted, label-smoothed mean cross-entropy of (B, NL) bf16 / fp32 logits (see CeLossFn)"""
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise _lib.FmmtError(f"ce_loss: label_smoothing must lie in [0, 1), got {label_smoothing}")
    return CeLossFn.apply(logits, labels, weight, float(label_smoothing))
