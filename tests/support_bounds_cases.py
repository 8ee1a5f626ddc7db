"""The case table of tests/test_gpu_kernel_bounds.py: one row per call of a non-GEMM entry point whose operands are handed over as views between
guard rows (tests/support_bounds.py).  Pure Python: reading the table needs neither torch nor the library (tests/test_kernel_bounds_cases_cpu.py
checks it on a machine without a GPU).

A row names the entry point, the element type, the shape, which optional operands and outputs are present, and the ROW UNIT of the kernel it reaches
-- the number of rows (tokens, windows, queries) one workgroup or one tile handles at a time -- named after the constant, or the expression, in the
source it was read from.  Every family whose kernels work in such units has three classes of M against its unit:
  below   M < unit                      one partial unit and nothing else
  ragged  M > unit and M % unit != 0    a partial unit behind whole ones: where a missing `row < M` guard reads, sums or stores rows >= M
  exact   M % unit == 0                 the guard-free instantiation where there is one (FULL, M % 256 == 0)
The families of the text encoder's tails and the patch embedding grid-stride single rows or are given one geometry by the model: one ragged case each.
"""
from collections import namedtuple
from itertools import product

GUARD_ROWS = 512                     # tests/support_strided.py GUARD (the CPU test holds the two together)

Case = namedtuple("Case", "id family entry dt shape opts unit unit_name M")

# family -> the classes of M it must show
FAMILIES = {
    "mha": {"below", "ragged", "exact"},
    "wattn": {"below", "ragged", "exact"},
    "wblock": {"below", "ragged", "exact"},
    "mlp": {"below", "ragged", "exact"},
    "lin_ln_bwd": {"below", "ragged", "exact"},
    "layernorm": {"below", "ragged", "exact"},
    "tails": {"ragged"},
    "patch": {"ragged"},
}


def m_class(M, unit):
    if M < unit:
        return "below"
    return "exact" if M % unit == 0 else "ragged"


# ---------------------------------------------------------------------------------------------------------------- multi-head attention
# attn.hip FMMT_MHA_DISPATCH: grid ((L + 63) / 64, B * heads), one query (key) row per lane; mha_mfma.hip: 64-query / 64-key tiles.
MHA_UNIT, MHA_UNIT_NAME = 64, "(L + 63) / 64 in FMMT_MHA_DISPATCH (attn.hip); the 64-row tiles of mha_mfma.hip"
MHA_GEOM = [(128, 2), (64, 2)]                                     # (E, heads): head_dim 64 (bf16: the MFMA kernels) and 32 (VALU only)
MHA_SHAPES = [(70, 33, 3), (33, 70, 2), (1, 65, 2), (64, 64, 1)]   # (Lq, Lk, B)


def mha_pitches(E, separate=False):
    """the five row pitches of a row, pairwise distinct and multiples of 8 elements: k / v (dk / dv) are column slices of one buffer of 2E columns,
    or -- separate -- buffers of their own of E columns"""
    kv = E if separate else 2 * E
    return {"ldq": E + 8, "ldkv": kv + 16, "ldo": E + 24, "lddq": E + 32, "lddkv": kv + 40}


def _mha_rows():
    rows = []
    for (E, nh), (Lq, Lk, B), bm, kb, p, dt in product(MHA_GEOM, MHA_SHAPES, (0, 1), (0, 1), (0.0, 0.1), ("bf16", "f32")):
        shape = dict(Lq=Lq, Lk=Lk, B=B, E=E, heads=nh, p=p, **mha_pitches(E))
        opts = dict(batch_major=bool(bm), key_bias=bool(kb), separate=False)
        tag = f"E{E}-{Lq}x{Lk}x{B}-{'bm' if bm else 'tm'}-{'kb' if kb else 'nokb'}-p{p}-{dt}"
        rows.append(Case(f"mha_fwd-{tag}", "mha", "fmmt_mha_fwd", dt, shape, opts, MHA_UNIT, MHA_UNIT_NAME, Lq))
        rows.append(Case(f"mha_bwd-{tag}", "mha", "fmmt_mha_bwd", dt, shape, opts, MHA_UNIT, MHA_UNIT_NAME, Lq))
        if not bm and kb:                                          # (fmmt_mha_avg_weights has no batch-major form)
            rows.append(Case(f"mha_avg-{tag}", "mha", "fmmt_mha_avg_weights", dt, shape, opts, 1, "one workgroup per (query, batch): dim3(Lq, B)", Lq))
    for (E, nh), dt in product(MHA_GEOM, ("bf16", "f32")):         # k, v, dk, dv in buffers of their own
        shape = dict(Lq=70, Lk=33, B=3, E=E, heads=nh, p=0.1, **mha_pitches(E, separate=True))
        opts = dict(batch_major=False, key_bias=True, separate=True)
        for e in ("fwd", "bwd"):
            rows.append(Case(f"mha_{e}-E{E}-70x33x3-tm-kb-p0.1-{dt}-separate", "mha", f"fmmt_mha_{e}", dt, shape, opts, MHA_UNIT, MHA_UNIT_NAME, 70))
    for p in (0.0, 0.1):                                           # ragged mode: packed rows, more rows than the sequences fill
        shape = dict(T=70, B=3, E=128, heads=2, lens=(70, 33, 1), rows=112, p=p, **mha_pitches(128))
        for e in ("fwd", "bwd"):
            rows.append(Case(f"mha_{e}_ragged-T70-p{p}", "mha", f"fmmt_mha_{e}_ragged", "bf16", shape, dict(separate=False), MHA_UNIT, MHA_UNIT_NAME, 70))
    return rows


# ---------------------------------------------------------------------------------------------------------------- window attention
# (n_img, H, C, heads, shift); M = windows = n_img * (H / 7)^2.  The last row is not in the issue's list: five windows, the one count that is
# ragged against the 4 windows an iteration of the fp32 VALU kernels and of the bf16 forward takes.
WATTN_SHAPES = [(1, 7, 96, 3, 0), (3, 7, 96, 3, 0), (1, 14, 96, 3, 3), (1, 14, 192, 6, 3), (3, 7, 768, 24, 0), (5, 7, 96, 3, 0)]


def wattn_unit(dt, bwd, generic):
    """windows per workgroup iteration: `wpi` of wa_groups_per_head (attn.hip) -- 2 for the bf16 MFMA backward (two waves per window), 4 otherwise --;
    the generic backward (wattn_bwd_ref.hip: fp32 with no mask or the standard mask) takes one window per pair of waves"""
    if bwd and generic:
        return 1, "fmmt_wattn_bwd_groups(B_, heads, 1) (attn.hip): one window per iteration"
    return (2 if (dt == "bf16" and bwd) else 4), "wpi in wa_groups_per_head (attn.hip)"


def _wattn_rows():
    rows = []
    for (n, H, C, nh, shift), dt in product(WATTN_SHAPES, ("bf16", "f32")):
        masks = [("nomask", False, False)] if not shift else [("std", True, True), ("tensor", True, False)]     # (tag, mask tensor passed, mask_is_shift)
        for tag, has_mask, mis in masks:
            M = n * (H // 7) ** 2
            shape = dict(n_img=n, H=H, C=C, heads=nh, shift=shift)
            opts = dict(mask=has_mask, mask_is_shift=mis)
            cid = f"n{n}-H{H}-C{C}-s{shift}-{tag}-{dt}"
            u, un = wattn_unit(dt, False, False)
            rows.append(Case(f"wattn_fwd-{cid}", "wattn", "fmmt_window_attn_fwd", dt, shape, opts, u, un, M))
            u, un = wattn_unit(dt, True, dt == "f32" and (not has_mask or mis))
            rows.append(Case(f"wattn_bwd-{cid}", "wattn", "fmmt_window_attn_bwd", dt, shape, opts, u, un, M))
    return rows


# ---------------------------------------------------------------------------------------------------------------- fused block half
# (n_img, H, shift); the last three are not in the issue's list: 8 windows (exact against the forward's 8 waves per workgroup), 12 (ragged against 8)
# and 5 (ragged against the 4 windows per iteration of the recompute backward)
WBLOCK_SHAPES = [(1, 7, 0), (3, 7, 0), (1, 14, 3), (2, 14, 0), (3, 14, 3), (5, 7, 0)]


def _wblock_rows():
    rows = []
    for (n, H, shift), rs, saved in product(WBLOCK_SHAPES, (True, False), (True, False)):
        if rs != saved:                                            # two combinations: everything optional present, everything optional NULL
            continue
        M = n * (H // 7) ** 2
        shape = dict(n_img=n, H=H, C=96, heads=3, shift=shift)
        opts = dict(rowscale=rs, xn=saved, attn_out=saved, stats=saved)
        tag = f"n{n}-H{H}-s{shift}-{'rs-saved' if rs else 'nors-nosave'}"
        rows.append(Case(f"wblock_fwd-{tag}-bf16", "wblock", "fmmt_window_block_fwd", "bf16", shape, opts, 8, "NW = 8 in wb_launch<96, 8> (wblock.hip): one wave per window", M))
    for (n, H, shift), C, rs in product(WBLOCK_SHAPES, (96, 192), (True, False)):
        M = n * (H // 7) ** 2
        shape = dict(n_img=n, H=H, C=C, heads=C // 32, shift=shift)
        rows.append(Case(f"wblock_attn_bwd-n{n}-H{H}-C{C}-s{shift}-{'rs' if rs else 'nors'}-bf16", "wblock", "fmmt_window_block_attn_bwd", "bf16", shape,
                         dict(rowscale=rs), 4, "fmmt_wattn_bwd_groups(B_, heads, 4) in wba_run (attn.hip)", M))
    return rows


# ---------------------------------------------------------------------------------------------------------------- fused Mlp
MLP_M = {96: (40, 296, 256), 192: (40, 168, 296, 256)}


def mlp_unit(entry, C, dt):
    """tokens per tile: 256 in both forward kernels (a.tiles = (M + 255) / 256 in fmmt_mlp_fwd; FULL = M % 256 == 0) and in the generic restatements
    (mlp_ref.hip, fp32); TT = C == 96 ? 256 : 128 in launch_mlp_bwd (mlp_fused.hip) for the bf16 backward"""
    if "bwd" in entry and dt == "bf16" and C == 192:
        return 128, "TT = C == 96 ? 256 : 128 in launch_mlp_bwd (mlp_fused.hip)"
    return 256, "a.tiles = (M + 255) / 256; FULL = M % 256 == 0 in launch_mlp (mlp_fused.hip)"


def _mlp_rows():
    rows = []
    entries = ("fmmt_mlp_fwd", "fmmt_mlp_ln_fwd", "fmmt_mlp_bwd_input", "fmmt_mlp_ln_bwd_input")
    for entry, C in product(entries, (96, 192)):
        for M, dg, full in product(MLP_M[C], (False, True), (True, False)):
            # full: rowscale (rows_per_scale 49, one zero) and every optional operand / output present; not full: all of them NULL
            u, un = mlp_unit(entry, C, "bf16")
            shape = dict(M=M, C=C, rows_per_scale=49)
            opts = dict(dg=dg, rowscale=full, res=full, h_pre=full, h_act=full, xn=full, stats=full)
            rows.append(Case(f"{entry[5:]}-M{M}-C{C}-{'dg' if dg else 'pre'}-{'full' if full else 'bare'}-bf16", "mlp", entry, "bf16", shape, opts, u, un, M))
        u, un = mlp_unit(entry, C, "f32")                          # one fp32 case each: the generic restatement, ragged
        rows.append(Case(f"{entry[5:]}-M296-C{C}-pre-full-f32", "mlp", entry, "f32", dict(M=296, C=C, rows_per_scale=49),
                         dict(dg=False, rowscale=True, res=True, h_pre=True, h_act=True, xn=True, stats=True), u, un, 296))
    return rows


# ---------------------------------------------------------------------------------------------------------------- Linear + LayerNorm backward
def _lin_ln_rows():
    rows = []
    for M, dres, dt in product((40, 296, 256), (True, False), ("bf16", "f32")):
        rows.append(Case(f"linear_ln_bwd-M{M}-{'dres' if dres else 'nodres'}-{dt}", "lin_ln_bwd", "fmmt_linear_ln_bwd", dt, dict(M=M, C=96, K=288),
                         dict(dres=dres), 256, "a.tiles = (M + 255) / 256 in fmmt_linear_ln_bwd (lin_lnbwd.hip)", M))
    return rows


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_rows_per_pass(C, dt):
    """ROWS = 256 / G of ln_fwd_kernel / ln_bwd_kernel with pick_shape's G (layernorm.hip): 16-lane groups up to 48 16-byte chunks per row, else a wave"""
    chunks = C // (8 if dt == "bf16" else 4)
    return 16 if chunks <= 48 else 4


def _ln_rows():
    rows = []
    un = "ROWS = 256 / G in ln_fwd_kernel / ln_bwd_kernel, G from pick_shape (layernorm.hip)"
    for (M, C), dt in product([(1, 96), (77, 192), (33, 768), (20, 1536)], ("bf16", "f32")):
        u = ln_rows_per_pass(C, dt)
        rows.append(Case(f"layernorm_fwd-{M}x{C}-{dt}", "layernorm", "fmmt_layernorm_fwd", dt, dict(M=M, C=C, merge_hw=0), dict(stats=True), u, un, M))
        for add in (True, False):
            rows.append(Case(f"layernorm_bwd-{M}x{C}-{'add' if add else 'noadd'}-{dt}", "layernorm", "fmmt_layernorm_bwd", dt, dict(M=M, C=C, merge_hw=0),
                             dict(add=add), u, un, M))
    for (n, Cq), dt in product([(1, 96), (3, 384)], ("bf16", "f32")):          # PatchMerging form, merge_hw = 14: M = n * 49 rows of C = 4 Cq
        M, C = n * 49, 4 * Cq
        u = ln_rows_per_pass(C, dt)
        rows.append(Case(f"layernorm_fwd-merge14-n{n}-Cq{Cq}-{dt}", "layernorm", "fmmt_layernorm_fwd", dt, dict(M=M, C=C, merge_hw=14, n=n), dict(stats=True), u, un, M))
        for add in (True, False):
            rows.append(Case(f"layernorm_bwd-merge14-n{n}-Cq{Cq}-{'add' if add else 'noadd'}-{dt}", "layernorm", "fmmt_layernorm_bwd", dt,
                             dict(M=M, C=C, merge_hw=14, n=n), dict(add=add), u, un, M))
    return rows


# ---------------------------------------------------------------------------------------------------------------- text / fusion tails
def _tail_rows():
    rows = []
    fwd_u, fwd_n = 4, "row = blockIdx.x * 4 + wave in the forward kernel (plm_fused.hip): 4 rows per workgroup"
    bwd_u, bwd_n = 8, "PF_BW = 8 (plm_fused.hip): rows in flight per workgroup of the backward"
    for (M, C) in [(37, 768), (5, 1024)]:
        rows.append(Case(f"layernorm_bwd_bf16-{M}x{C}", "tails", "fmmt_layernorm_bwd_bf16", "bf16", dict(M=M, C=C), {}, 4,
                         "row = blockIdx.x * 4 + wave in the bf16 LayerNorm backward (misc.hip): 4 rows per workgroup", M))
        for p in (0.0, 0.1):
            for pd in ("bf16", "f32"):                              # the affine parameters' type
                sh = dict(M=M, C=C, p=p, param_dt=pd)
                rows.append(Case(f"dropadd_ln_fwd-{M}x{C}-p{p}-param{pd}", "tails", "fmmt_dropadd_ln_fwd", "bf16", sh, {}, fwd_u, fwd_n, M))
                rows.append(Case(f"dropadd_ln_bwd-{M}x{C}-p{p}-param{pd}", "tails", "fmmt_dropadd_ln_bwd", "bf16", sh, dict(dbias=True), bwd_u, bwd_n, M))
            sh = dict(M=M, C=C, p=p, param_dt="bf16")
            rows.append(Case(f"plm_dropadd_ln_fwd-{M}x{C}-p{p}", "tails", "fmmt_plm_dropadd_ln_fwd", "bf16", sh, {}, fwd_u, fwd_n, M))
            rows.append(Case(f"plm_dropadd_ln_bwd-{M}x{C}-p{p}", "tails", "fmmt_plm_dropadd_ln_bwd", "bf16", sh, dict(dbias=p == 0.0), bwd_u, bwd_n, M))
    rows.append(Case("plm_gelu_bwd_colsum-37x3072", "tails", "fmmt_plm_gelu_bwd_colsum", "bf16", dict(M=37, H=3072), {}, 4,
                     "GB_PH = 4 (plm_fused.hip): row phases per workgroup", 37))
    return rows


# ---------------------------------------------------------------------------------------------------------------- patch embedding
def _patch_rows():
    un = "tiles = (M + 255) / 256 in fmmt_patch_embed_ln_fwd (patch_ln.hip)"
    return [Case(f"patch_embed_ln_fwd-n1-{dt}", "patch", "fmmt_patch_embed_ln_fwd", dt, dict(M=3136, C=96, K=48), dict(x_pre=True, stats=True), 256, un, 3136)
            for dt in ("bf16", "f32")]


CASES = _mha_rows() + _wattn_rows() + _wblock_rows() + _mlp_rows() + _lin_ln_rows() + _ln_rows() + _tail_rows() + _patch_rows()


def rowscale_len(c):
    """entries of the rowscale vector of a case that has one: one per image (block half), one per rows_per_scale rows (Mlp)"""
    if c.family == "wblock":
        return c.shape["n_img"]
    rps = c.shape["rows_per_scale"]
    return (c.shape["M"] + rps - 1) // rps


def of(entry):
    return [c for c in CASES if c.entry == entry]


def largest_overread_rows():
    """the most rows behind M any kernel of the table may touch when its last unit is partial, in rows of the operand it reads:
    a whole unit of tokens (256-row tiles), 4 windows x 49 tokens, and the 63 keys x B of the last time-major attention tile"""
    worst = 0
    for c in CASES:
        if c.family in ("wattn", "wblock"):
            worst = max(worst, c.unit * 49)
        elif c.family == "mha":
            worst = max(worst, (c.unit - 1) * c.shape["B"])
        else:
            worst = max(worst, c.unit)
    return worst
