// Which kernel a Linear call takes, and with what geometry: the whole decision of gemm.hip as integer arithmetic on shapes.
// Plain C++17: no HIP header, no operand pointer, no launch -- it compiles with any host compiler (tests/gemm_plan_sweep.cpp runs it under sanitizers).
// The entry points and the route queries of gemm.hip call the same two functions, check_query() and plan_query(); the route of the plan indexes
// gemm.hip's launch table and nothing in between changes it.
#pragma once
#include <stddef.h>
#include "../../include/fmmt.h"

namespace {

// A call as the entry points see it, pointers reduced to presence.  Weight gradient: ldy is dy's pitch (dy is [M][N]), ldx is x's.
enum { GEMM_FWD = FMMT_ROUTE_MODE_FWD, GEMM_SEG3_N = FMMT_ROUTE_MODE_SEG3_N, GEMM_SEG3_K = FMMT_ROUTE_MODE_SEG3_K, GEMM_SPLITK = FMMT_ROUTE_MODE_SPLITK,
       GEMM_WGRAD, GEMM_WGRAD_PARTIALS };
struct GemmQuery {
    int mode, dtype, M, N, K;
    int ldx, ldw, ldy, ldaux, ldres;
    bool bias, y_pre, aux, res, rowscale;                   // seg3: bias = any of the three
    int epi, rows_per_scale, x_epi;
};

// What the launch site needs and the kernel does not compute itself.
struct GemmPlan {
    int route;                                              // enum fmmt_route, or a negative FMMT_E*
    int tiles_m, tiles_n, bn;                               // NT: LinArgs::tiles_*; bn = channels per tile (96 / 128 share a route)
    int ksplit, splits, grid;                               // NT: K range per blockIdx.y and their number; TN: token splits; grid: gridDim.x
    int tiles_k, chunk, npad, tn, tk;                       // TN: TnArgs fields; tn x tk != 0: linear_tn_dma_kernel's tile, tn = the layout word of the workspace header
    bool direct;                                            // TN: one split written to dw / db themselves: no header, no finish pass
    int smax, rows;                                         // workspace carving (TN): [header | bias partials smax x rows | weight partials smax x rows x K]
    size_t ws_bytes;                                        // workspace size (TN, split-K)
};

// ---- predicates that several plans share ----
// kernels that form per-lane unsigned 32-bit byte offsets of 2-byte elements: rows x ld elements have to stay below 2^31
inline bool fits32(int rows, int ld) { return (unsigned long long)rows * ld < (1ull << 31); }
// direct global->LDS DMA moves 16-byte pieces of bf16 rows: both operands' pitches in whole pieces
inline bool dma_pitches(const GemmQuery& a) { return a.ldx % 8 == 0 && a.ldw % 8 == 0; }
inline bool nearly_full(long long tiles) { return tiles * 100 >= (tiles + 255) / 256 * 256 * 85; }    // rounds of 256 persistent workgroups at least 85 % full
constexpr int SMALL_TILES = 256;                           // fewer 64 x 128 tiles than this: the quarter-tile kernels (dispatch_nt) and the only shapes of fmmt_linear_fwd_seg3
inline bool few_tiles(int M, int N) { return ((M + 63) / 64) * ((N + 127) / 128) < SMALL_TILES; }
constexpr int SMALL_R4K = 2048;                            // four-buffer ring from this K
// a matrix operand's rows: `width` elements, 16-byte aligned, inside the pitch
inline bool rows_ok(int width, int ld, int vec) { return width % vec == 0 && ld % vec == 0 && ld >= width; }

// Shape and pitch validation of an entry point: 0 or FMMT_EINVAL.  (Pointer alignment is the entry point's: FMMT_EALIGN, checked after this.)
// Every epilogue moves 16-byte vectors at row * ld + column (nt_epilogue / _slab / _wslab, the p256 slab stores, the buffer stores of gemm_ph.h /
// gemm_ph3.h; DESIGN.md "Leading dimensions of the GEMMs"): N and every ld of a present M x N operand keep each row 16-byte aligned.
inline int check_query(const GemmQuery& q) {
    if (q.M <= 0 || q.N <= 0 || q.K <= 0 || (q.dtype != FMMT_BF16 && q.dtype != FMMT_F32) || q.mode < GEMM_FWD || q.mode > GEMM_WGRAD_PARTIALS) return FMMT_EINVAL;
    const int vec = q.dtype == FMMT_BF16 ? 8 : 4;
    const bool wgrad = q.mode == GEMM_WGRAD || q.mode == GEMM_WGRAD_PARTIALS, seg3 = q.mode == GEMM_SEG3_N || q.mode == GEMM_SEG3_K;
    // x [M][K], y / dy [M][N]; the weight's rows are K wide (a third of it for weights segmented along K)
    if (!rows_ok(q.K, q.ldx, vec) || !rows_ok(q.N, q.ldy, vec)) return FMMT_EINVAL;
    if (!wgrad && !rows_ok(q.mode == GEMM_SEG3_K ? q.K / 3 : q.K, q.ldw, vec)) return FMMT_EINVAL;
    if (q.mode != GEMM_SPLITK && !seg3 && q.rowscale && q.rows_per_scale <= 0) return FMMT_EINVAL;
    if (q.mode == GEMM_FWD) {
        if (q.epi < 0 || q.epi > FMMT_EPI_MUL_AUX) return FMMT_EINVAL;
        if ((q.epi == FMMT_EPI_GELU_BWD || q.epi == FMMT_EPI_MUL_AUX) && !q.aux) return FMMT_EINVAL;
        if (q.aux && !rows_ok(q.N, q.ldaux, vec)) return FMMT_EINVAL;
        if (q.res && !rows_ok(q.N, q.ldres, vec)) return FMMT_EINVAL;
    }
    if (seg3) {
        // bf16, the direct-to-LDS quarter-tile kernels only (the shapes dispatch_nt sends there: tokens <= 4096, few tiles)
        const int seg = q.mode == GEMM_SEG3_N ? q.N / 3 : q.K / 3;
        if (q.dtype != FMMT_BF16 || (q.mode == GEMM_SEG3_N ? q.N : q.K) % 3 || seg % 64 || q.N % 64 || q.K % 64 || q.K < 128 || q.M > 4096) return FMMT_EINVAL;
        if (q.mode == GEMM_SEG3_K && q.bias) return FMMT_EINVAL;
    }
    return 0;
}

inline GemmPlan refuse(int rc) { GemmPlan pl{}; pl.route = rc; return pl; }

// geometry of one output tile per workgroup (bm x bn), or of 256 persistent workgroups walking such tiles
inline GemmPlan nt_tiles(int route, const GemmQuery& a, int bm, int bn, int ksplit = 0, bool persistent = false) {
    GemmPlan pl{};
    pl.route = route, pl.bn = bn, pl.ksplit = ksplit;
    pl.tiles_m = (a.M + bm - 1) / bm, pl.tiles_n = (a.N + bn - 1) / bn;
    pl.splits = ksplit ? (a.K + ksplit - 1) / ksplit : 1;
    pl.grid = persistent ? 256 : pl.tiles_m * pl.tiles_n;
    return pl;
}

// Tile choice for the persistent kernel: the widest channel tile that divides N, unless a narrower one fills the last
// round of 256 workgroups better (31360 tokens x 768 channels: 369 tiles of 256 x 256 = 2 rounds at 72 %, 492 tiles of
// 256 x 192 = 2 rounds at 96 %).  Returns the route (tile width and loop form), 0 if the shape is not for this kernel.
inline int p256_plan(const GemmQuery& a, int ksplit, int* bn) {
    constexpr int P256_MINM = 16384;                       // fewest tokens for this kernel
    // (K % 64 != 0 -- Swin stage 0: K = 96 -- stays on the deep / single-step kernels)
    if (ksplit || a.M < P256_MINM || a.M % 16 || a.K % 64 || a.K < 96 || !dma_pitches(a)) return 0;
    if (!fits32(a.M, a.ldx) || !fits32(a.N, a.ldw)) return 0;   // 32-bit byte offsets of the DMA pieces
    // One workgroup per CU has nothing to hide an epilogue's own M x N loads behind (residual, GELU' operand, DropPath
    // scale: the in-order vmcnt also makes them wait for the DMA stages in flight).  Measured on MI355X
    // (profiles/r02_gemm_shapes.txt): plain / bias / GELU + pre-activation launches gain 5-50 % over the two-workgroup
    // 256 x 128 kernels (125440 x 1536 x 384 GELU: 0.439 -> 0.295 ms).
    // Launches with a residual and / or DropPath scale come here too, on the 192- / 128-wide tiles, with the operand prefetched
    // into registers one K step before the epilogue (HASOP): measured, same call, 321 -> 262 us (501760 x 192 x 768), 210 -> 201
    // (125440 x 384 x 1536).  GELU' launches (an aux operand) do not: 338 -> 391 / 530 -> 614 us -- that epilogue is ~11 k VALU
    // cycles per wave tile against 4.6 k MFMA cycles of a K = 384 tile, and one workgroup per CU has no second workgroup whose K
    // loop could run under it.
    // (round 4: re-measured with gelu' from an LDS table in this kernel's unused epilogue scratch instead of the polynomial: 125440 x 1536 x 384
    //  328 -> 364 us, 501760 x 768 x 192 522 -> 561, 31360 x 3072 x 768 267 -> 253 -- still a loss where it matters.
    //  And once more with the polynomial GELU' that replaced the tables: 314 -> 340, 491 -> 529, 258 -> 241 us.)
    const bool has_op = a.res || a.aux || a.rowscale;
    if (has_op && (a.aux || a.ldres % 8 || a.ldaux % 8)) return 0;
    const int tm = (a.M + 255) / 256;
    int best_i = -1;
    double best_cost = 0;
    const int cand[3] = {256, 192, 128};
    const int routes[3][3] = {{FMMT_ROUTE_P256_256, FMMT_ROUTE_P256_256_PIPE, 0},                       // plain loop, pipelined loop, operand prefetch
                              {FMMT_ROUTE_P256_192, FMMT_ROUTE_P256_192_PIPE, FMMT_ROUTE_P256_192_OP},
                              {FMMT_ROUTE_P256_128, FMMT_ROUTE_P256_128_PIPE, FMMT_ROUTE_P256_128_OP}};
    const double pen[3] = {1.0, 1.04, 1.10};
    for (int i = 0; i < 3; ++i) {
        const int w = cand[i];
        if (a.N % w) continue;
        if (has_op && w == 256) continue;
        const int tiles = tm * (a.N / w);
        if (tiles < 256) continue;
        const double cost = (double)((tiles + 255) / 256) * w * pen[i];
        if (best_i < 0 || cost < best_cost) {
            best_i = i;
            best_cost = cost;
        }
    }
    if (best_i < 0) return 0;
    *bn = cand[best_i];
    // launches with an M x N epilogue operand or a DropPath scale: operand prefetched into registers (48 / 32 of them:
    // no room beside the 128 accumulators of the 256-wide tile).  (Operand-free launches that store directly, K > 1536, were tried
    // on this instantiation as well: against the pipelined loop below it loses, 135 -> 127 us, same call.)
    if (has_op) return routes[best_i][2];
    // Pipelined fragment reads + DMA pieces in groups (PIPE), for K >= 384.  Same-call A/B against the plain loop, us per
    // launch: 31360 x 2304 x 768 124 -> 115, 31360 x 3072 x 768 150 -> 141, 31360 x 768 x 768 44.4 -> 41.2, 125440 x 1536 x 384
    // (256-wide tile, one group) 190 -> 178, 125440 x 384 x 384 52.7 -> 50.2, 125440 x 1152 x 384 / 384 x 1536 / 384 x 1152 +-1 %;
    // K = 192 (three K steps per tile: the late pieces are waited for) 210 -> 220, stays on the plain loop.
    return routes[best_i][a.K >= 384 ? 1 : 0];
}

// The 64- / 128-row kernels with one output tile per workgroup: the K loop's form.
inline GemmPlan dispatch_nt_bk(const GemmQuery& a, int ksplit, int bm, int bn) {
    const bool m64 = bm == 64;
    if (a.dtype != FMMT_BF16) return nt_tiles(m64 ? FMMT_ROUTE_NT64_F32 : FMMT_ROUTE_NT128_F32, a, bm, bn, ksplit);   // fp32 parity path
    // Swin stage 0: one K step.  (64- and 256-row tiles measured: no gain / -35 %.)  These launches are HBM streams
    // (40-70 FLOP/B); epilogue-shaped stores alone reach 5.5 TB/s on this part (profiles/r01_hbm_calibration.txt), what
    // holds a single-step workgroup at ~3 TB/s is its load -> LDS -> MFMA -> store chain with nothing to overlap, so
    // occupancy is what counts (NtWaves in gemm.hip); the fc1 + GELU + pre-activation launch is the only one still on it.
    if (!ksplit && a.K == 96) return nt_tiles(m64 ? FMMT_ROUTE_NT64_K96 : FMMT_ROUTE_NT128_K96, a, bm, bn);
    if (!ksplit && a.K <= 64) return nt_tiles(m64 ? FMMT_ROUTE_NT64_K64 : FMMT_ROUTE_NT128_K64, a, bm, bn);     // PatchEmbed (K = 48)
    // measured on MI355X (tools/probes/gemm_bench.py, sum over the bench shapes): BK=64 5.33 ms vs BK=32 5.88 ms
    // direct global->LDS DMA staging: measured +7 % over register staging summed over the bench shapes, up to
    // +25 % on the K >= 768 ones (971 TF/s on 31360x768x3072)
    if (a.K % 64 == 0 && !ksplit && dma_pitches(a)) {
        // four-buffer ring for few-token problems with a long K loop and at most one workgroup per CU (fc2 of the
        // encoder FFNs, 512-1328 tokens x 768 x 3072: 32 -> 25 us); with more tiles than CUs the 96 KB ring costs
        // co-residency (1328 x 3072 x 768: 15 -> 21 us), and at K = 768 it is a wash.
        if (m64) {
            const int tiles = ((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn);
            if (a.K >= 2048 && tiles <= 256) return nt_tiles(FMMT_ROUTE_NT64_DMA_R4, a, bm, bn);      // a rule of its own: tiles of THIS kernel, <=; not few_tiles()
        }
        return nt_tiles(m64 ? FMMT_ROUTE_NT64_DMA : FMMT_ROUTE_NT128_DMA, a, bm, bn);
    }
    if (a.K % 64 == 0 && (!ksplit || ksplit % 64 == 0)) return nt_tiles(m64 ? FMMT_ROUTE_NT64_BK64 : FMMT_ROUTE_NT128_BK64, a, bm, bn, ksplit);
    return nt_tiles(m64 ? FMMT_ROUTE_NT64_BK32 : FMMT_ROUTE_NT128_BK32, a, bm, bn, ksplit);
}

// The phase-structured kernels (gemm_ph.h: 256 x 256 tiles, four phases; gemm_ph3.h: 192 x 256 tiles, three phases, all epilogues but GELU').
// Returns the route -- 0 (none), FMMT_ROUTE_PH (gemm_ph.h, plain / bias), _PH3_* (gemm_ph3.h, 192 x 256 tiles) or _PH3W_* (gemm_ph3.h, 384 x 128 tiles) -- and the tile's
// token rows in *bm; the route's suffix is gemm_ph3.h's EPI template value: 2 plain / bias, 3 GELU + pre-activation, 5 residual / row scale, 6 product with the stored
// GELU derivative (+ row scale).
// Measured against the kernels below and each other (tools/probes/nt_ph_probe.hip, same call, us per launch, production -> ph / ph3):
//   plain / bias     31360 x 768 x 3072 136 -> 139 / 110 (369 tiles of 256 x 256 = 1.44 rounds of 256 workgroups, 492 of 192 x 256 = 1.92), x 768 x 768 42 -> 44 / 35,
//                    x 2304 x 768 113 -> 101 / 100, x 3072 x 768 143 -> 129 / 132, 125440 x 1536 x 384 190 -> 154 / 167, 7840 x 1536 x 6144 168 -> 134 / 106,
//                    7840 x 6144 x 1536 186 -> 116 / 123, 7840 x 1536 x 1536 38.5 (128-row kernels) -> 38 / 31: the tile whose rounds waste less wins;
//   res + row scale  31360 x 768 x 3072 156 -> 117, x 768 x 768 56 -> 42, x 3072 x 768 235 -> 161, 125440 x 1536 x 384 318 -> 242, 7840 x 1536 x 6144 169 -> 110 (ph3 only);
//   GELU + pre       wins from K = 1536 (7840 x 6144 x 1536 211 -> 184, 31360 x 768 x 3072 159 -> 141), loses below (31360 x 3072 x 768 195 -> 254: the polynomial runs
//                    behind the MFMAs of a phase, on the workgroup's critical path, and a short K loop has few phases to amortise it);
//   GELU'            loses everywhere (262 -> 828): stays on the persistent kernel.
inline int ph_plan(const GemmQuery& a, int ksplit, int* bm) {
    const bool mul_aux = a.epi == FMMT_EPI_MUL_AUX && a.aux && !a.res && !a.y_pre && !a.bias;
    if (ksplit || (a.aux && !mul_aux)) return 0;
    const bool gelu_pre = a.epi == FMMT_EPI_GELU && a.y_pre, has_op = a.res || a.rowscale;
    if (!gelu_pre && !mul_aux && (a.epi != 0 || a.y_pre)) return 0;
    if (gelu_pre && (has_op || a.K < 1536)) return 0;
    if (mul_aux && (a.ldaux % 8 || !fits32(a.M, a.ldaux))) return 0;
    if (a.M < 4096 || a.M % 8 || a.N % 128 || a.K % 64 || a.K < 192 || !dma_pitches(a) || a.ldy % 8) return 0;
    if (a.res && a.ldres % 8) return 0;
    if (a.rowscale && a.rows_per_scale <= 0) return 0;
    if (!fits32(a.M, a.ldx) || !fits32(a.N, a.ldw) || !fits32(a.M, a.ldy) || (a.res && !fits32(a.M, a.ldres))) return 0;
    if (a.N % 256) {
        // channel counts that are multiples of 128 only (Swin stage 2: 384, 1152): gemm_ph3.h's 384-token x 128-channel layout (_PH3W_*).  Measured at 125440 tokens
        // (production -> ph3): x 1152 x 384 134 -> 129, x 384 x 384 45.5 -> 43.6, with residual + row scale 240 -> 204 / 79 -> 58, row scale alone 59 -> 54.5;
        // at K = 1152 / 1536 it loses (164 -> 166, with residual 181 -> 196: three channel tiles per token panel, 96 FLOP per staged byte): K <= 512 only.
        if (gelu_pre || a.K > 512) return 0;
        const long long t384 = (long long)((a.M + 383) / 384) * (a.N / 128);
        if (t384 < 256 || !nearly_full(t384)) return 0;
        *bm = 384;
        return mul_aux ? FMMT_ROUTE_PH3W_MUL_AUX : has_op ? FMMT_ROUTE_PH3W_OP : FMMT_ROUTE_PH3W_PLAIN;
    }
    const long long t256 = (long long)((a.M + 255) / 256) * (a.N / 256), t192 = (long long)((a.M + 191) / 192) * (a.N / 256);
    const long long r256 = (t256 + 255) / 256, r192 = (t192 + 255) / 256;
    const long long min_tiles = a.M < 16384 ? 150 : 256;        // 16384+ tokens: the persistent 256-row kernel's ground, taken only with (nearly) full rounds
    const bool ok256 = t256 >= min_tiles && (a.M < 16384 || nearly_full(t256));
    const bool ok192 = t192 >= min_tiles && (a.M < 16384 || nearly_full(t192));
    *bm = 192;
    if (gelu_pre || has_op || mul_aux) return !ok192 ? 0 : gelu_pre ? FMMT_ROUTE_PH3_GELU_PRE : mul_aux ? FMMT_ROUTE_PH3_MUL_AUX : FMMT_ROUTE_PH3_OP;
    // plain / bias: rows of MFMA work per workgroup over the launch; the 192-row tile is charged 3 % (shorter phases per byte staged)
    const long long c256 = r256 * 256 * 100, c192 = r192 * 192 * 103;
    if (ok192 && (!ok256 || c192 < c256)) return FMMT_ROUTE_PH3_PLAIN;
    *bm = 256;
    return ok256 ? FMMT_ROUTE_PH : 0;
}

// fmmt_linear_fwd and the contraction of fmmt_linear_fwd_splitk (ksplit != 0: fp32 partials instead of the epilogue)
inline GemmPlan dispatch_nt(const GemmQuery& a, int ksplit) {
    const bool bf = a.dtype == FMMT_BF16;
    // BN = 96 when it tiles N exactly and 128 would not (C = 96, 288, 192, 576 ...)
    const bool n96 = (a.N % 96 == 0) && (a.N % 128 != 0);
    // few-token problems (cross-modal encoder: 152..1280 rows; embedding head: 640 rows) use 64-row tiles so
    // that twice as many workgroups share the work; the multi-million-token Swin GEMMs use 128-row tiles
    // (few rows but tens of thousands of output channels -- the input gradient of the 37632 -> 512 embedding head: there are
    //  workgroups enough, 128-row tiles read each weight slab half as often)
    if (a.M <= 4096 && (a.N < 16384 || a.M < 256)) {
        // Fewer 64 x 128 tiles than half the CUs (the fusion stack: 152-1328 tokens x 768 channels = 18-126 tiles): such a
        // launch is a chain of K / 64 steps whose cost is the step's DMA issue (six 1-KB pieces per wave) plus a barrier, on a
        // mostly idle GPU.  Quarter tiles (32 x 64) put four times the workgroups on the chip, each with half the pieces per
        // wave and step.  Measured per launch inside a graph (tools/probes/few_probe.py, same call): 152-640 x 768 x 768 8.5 -> 5.5 us
        // (hipBLASLt 7.5-8.1), 1328 x 768 x 768 9.2 -> 6.7, 664 x 1536 x 768 9.0 -> 6.5, 512 x 3072 x 768 12.9 -> 9.8,
        // 512 x 768 x 3072 24.4 -> 16, 1328 x 768 x 3072 25.5 -> 19.5; with 256+ tiles of 64 x 128 the quarter tiles lose
        // (1328 x 3072 x 768: 14 -> 22 us), and the four-buffer ring does nothing for K = 768.  (64 x 64 tiles: 6.4 us on the first group.)
        if (bf && few_tiles(a.M, a.N) && a.N % 64 == 0 && a.K % 64 == 0 && a.K >= 128 && !ksplit && dma_pitches(a))
            return nt_tiles(a.K >= SMALL_R4K ? FMMT_ROUTE_NT_QUARTER_R4 : FMMT_ROUTE_NT_QUARTER, a, 32, 64);
        return dispatch_nt_bk(a, ksplit, 64, n96 ? 96 : 128);
    }
    if (bf) {
        int bm = 0, bn = 0;
        if (const int ph = ph_plan(a, ksplit, &bm)) return nt_tiles(ph, a, bm, bm == 384 ? 128 : 256, 0, true);
        if (const int p256 = p256_plan(a, ksplit, &bn)) return nt_tiles(p256, a, 256, bn, 0, true);
        // measured (tools/probes/gemm_bench.py): +8 % on the 125440-token stage-2 shapes (K = 384: 496 -> 540 TF/s),
        // -4 % on the 31360-token stage-3 shapes (tile quantisation at one workgroup per CU) -> only for M >= 65536
        constexpr int DEEP_MINM = 65536, DEEP_MINK = 96;
        // K = 96 (stage 0, three K steps): -5..7 % with the deep kernel except for the GELU + pre-activation launch
        // (two output streams; measured +2 %), which keeps the single-step kernel
        const bool big = a.M >= DEEP_MINM && !ksplit && a.K % 32 == 0 && a.K >= DEEP_MINK && dma_pitches(a) &&
                         !(a.K == 96 && a.epi == FMMT_EPI_GELU);
        if (big && n96)
            return nt_tiles(a.K == 192 ? FMMT_ROUTE_DEEP32_K192_N96 : a.K == 96 ? FMMT_ROUTE_DEEP32_K96_N96 : FMMT_ROUTE_DEEP32_N96, a, 256, 96);
        if (big && a.N % 128 == 0) {
            // measured (tools/probes/gemm_bench.py, 125440 tokens): the K-step-32 kernel with two workgroups per CU wins
            // where the epilogue is a large share of a tile's life -- GELU / GELU' launches (0.388 -> 0.340 ms) and
            // K = 384 (384x384: 0.069 -> 0.057 ms); the K-step-64 kernel keeps a 2-4 % edge on plain K >= 1152.
            if (a.epi != 0 || a.K <= 512 || a.K % 64 != 0)
                return nt_tiles(a.K == 192 ? FMMT_ROUTE_DEEP32_K192_N128 : a.K == 96 ? FMMT_ROUTE_DEEP32_K96_N128 : FMMT_ROUTE_DEEP32_N128, a, 256, 128);
            return nt_tiles(FMMT_ROUTE_DEEP, a, 256, 128);
        }
    }
    // (256-row tiles with 4 waves measured: -30 % on the stage-2/3 shapes -- one workgroup per CU)
    return dispatch_nt_bk(a, ksplit, 128, n96 ? 96 : 128);
}

// split-K plan for skinny problems (the 37632 -> 512 head): few output tiles, very long K
inline int splitk_plan(int M, int N, int K, int* ksplit) {
    const int bm = M <= 4096 ? 64 : 128;
    const int tiles = ((M + bm - 1) / bm) * ((N + 127) / 128);
    if (tiles >= 128 || K < 4096) { *ksplit = 0; return 1; }
    int splits = 512 / tiles;
    if (splits > 32) splits = 32;
    int ks = (K + splits - 1) / splits;
    ks = (ks + 63) / 64 * 64;
    *ksplit = ks;
    return (K + ks - 1) / ks;
}

// ---- TN (weight gradient): the geometry fields of a GemmPlan; tn != 0: linear_tn_dma_kernel<tn>; npad: rows of a split's partials (0 = N) ----
inline GemmPlan tn_tiles(int tiles_n, int tiles_k, int splits, int chunk, int tn = 0, int tk = 0, int npad = 0) {
    GemmPlan pl{};
    pl.tiles_n = tiles_n, pl.tiles_k = tiles_k, pl.splits = splits, pl.chunk = chunk, pl.tn = tn, pl.tk = tk, pl.npad = npad, pl.grid = tiles_n * tiles_k * splits;
    return pl;
}

// (An XCD-local decomposition -- tile shapes 192 x 96 / 96 x 192 / 128 x 128 chosen so that all tiles of a token split fill
//  whole XCDs, every dy / x slab fetched into exactly one L2 -- was written, tested and measured: the stage-2/3 launches of the
//  step took 7.16 ms against 6.57 ms with this split-major order (same call).  The second fetch of a slab is served by the
//  256 MB Infinity Cache; what the XCD-local form paid was 6-25 % idle workgroup slots and 244-252 registers.  Not kept.)
inline GemmPlan tn_plan(int M, int N, int K) {
    const int tiles_n = (N + 127) / 128, tiles_k = (K + 127) / 128;
    const int tiles = tiles_n * tiles_k;
    // one round of co-resident workgroups: 2 per CU for the 64-token-step kernels (64-78 KB LDS), 3 per CU for
    // the 32-token-step kernel; more would run as a second, partly empty round
    // (leaving head-room for the concurrent text-encoder stream -- 448/672, 384/576 -- measured: no gain)
    const int target = (M <= 262144) ? 512 : 768;
    int splits = target / tiles;
    // few-token problems (fusion stack: 152-664 rows): one pass over the tokens per output tile, written straight to
    // dW / db by fmmt_linear_wgrad -- a second launch to add two or three partials costs as much as the contraction
    if (M <= 768) splits = 1;
    const int max_by_rows = (M + 255) / 256;
    if (splits > max_by_rows) splits = max_by_rows;
    if (splits < 1) splits = 1;
    // keep the partial buffer under 512 MiB
    while (splits > 1 && (size_t)splits * N * K * 4 > ((size_t)512 << 20)) --splits;
    int chunk = (M + splits - 1) / splits;
    chunk = (chunk + 63) / 64 * 64;
    return tn_tiles(tiles_n, tiles_k, (M + chunk - 1) / chunk, chunk);
}

// DMA-staged plan (linear_tn_dma_kernel): tile TNn x 128 with TNn = 256 / 192, one workgroup per CU, splits = 256 / tiles
inline GemmPlan tn_plan_dma(int M, int N, int K) {
    // History: the first version of this kernel (256 / 192 x 128 tiles,
    // the builtin ds_read_tr) measured 3-9 % SLOWER than the register-staged kernel with 68 % of its wave cycles parked in
    // waits -- hipcc had put s_waitcnt vmcnt(0) in front of every stage's first fragment read, so the ring never had a second
    // stage in flight.  With the reads in inline asm, 128 FLOP per staged byte and four 32-token stages: 860-1105 TF/s against
    // 550-630.
    // Fewest tokens for this kernel, exclusive.  8192 since the 320-frame legs (configs[4]: 15680 stage-3 tokens)
    // measured 56.2 -> 55.7 ms per step with it, three alternating pairs in one call; 16384 before.
    constexpr int TN_DMA_MINM = 8192;
    if (M <= TN_DMA_MINM || M % 64) return GemmPlan{};
    int tn = 0, tk = 0;
    if (N % 256 == 0 && K % 256 == 0) tn = 256, tk = 256;
    else if (N % 192 == 0 && K % 384 == 0) tn = 192, tk = 384;
    // round 6: the transposed tile for K = 192 (Swin stage 1's fc1 weight gradient, 768 x 192: it fell to the 128 x 128 register-staged kernel at 3.3 TB/s
    // where its mirror image 192 x 768 runs at 4.7 on <192,384>); one k-tile only (the bias blocks' positions assume it), unscaled launches only
    // N = 576 (stage 1's qkv weight gradient) is 192 short of two tiles: the last tile's upper half re-reads valid columns and its products go to partial rows
    // the finish pass drops (npad)
    else if ((N % 384 == 0 || (N % 384 == 192 && N >= 576)) && K == 192) tn = 384, tk = 192;
    // (two or three tiles used to be refused -- > 64 splits, "the partial sums outweigh the operands" --; re-measured in round 4, same call:
    //  501760 x 192 x 768 with the DropPath scale 324 -> 233 us, 125440 x 384 x 384 70 -> 64 us with the finish pass, no shape slower.  One tile stays out.)
    const int npad = tn ? (N + tn - 1) / tn * tn : 0;
    if (tn && (npad / tn) * (K / tk) < 2) tn = 0;
    if (!tn) return GemmPlan{};
    const int tiles = (npad / tn) * (K / tk);
    if (tiles > 128) return GemmPlan{};
    int splits = 256 / tiles;
    while (splits > 1 && (size_t)splits * npad * K * 4 > ((size_t)512 << 20)) --splits;
    int chunk = (M + splits - 1) / splits;
    chunk = (chunk + 63) / 64 * 64;
    splits = (M + chunk - 1) / chunk;
    if (chunk < 512) return GemmPlan{};
    return tn_tiles(npad / tn, K / tk, splits, chunk, tn, tk, npad == N ? 0 : npad);
}

// eligibility of linear_tn_few_kernel: bf16, 129..2048 tokens, whole 64 x 64 tiles, at least 8 of them, 16-byte rows
inline bool tn_few_ok(int M, int N, int K, int dtype) {
    // (at most 1024 tiles: the embedding head's 512 x 37632 gradient -- 4704 tiles of 640 tokens -- took 767 us here against 292 us
    //  with the 128 x 128-tile kernel, whose workgroups reuse each staged token slab four times as often)
    return dtype == FMMT_BF16 && M > 128 && M <= 2048 && N % 64 == 0 && K % 64 == 0 && (N / 64) * (K / 64) >= 8 && (N / 64) * (K / 64) <= 1024;
}

// The weight gradient of one call, computed once: the plan its contraction takes and the carving of its workspace, [256-byte header | bias partials
// smax x rows | weight partials smax x rows x K].  The carving is a function of (dtype, M, N, K) alone (fmmt_linear_wgrad_workspace and _finish read it from
// a query that holds nothing else): smax and rows are the largest split and row counts of the plans such a launch MAY take, may[] below.  Which of them it
// takes also depends on its operands (DropPath scale ...), so the contraction kernel records the split count it wrote in the header and the finish pass reads it from there.
constexpr size_t TN_HDR = 256;
inline GemmPlan launch_tn_plan(const GemmQuery& q) {
    const int M = q.M, N = q.N, K = q.K;
    // linear_tn_few_kernel: the eight waves split the tokens, one split.  (A plan without splits: not for this shape.)
    const GemmPlan few = tn_few_ok(M, N, K, q.dtype) ? tn_tiles(N / 64, K / 64, 1, (M + 7) / 8) : GemmPlan{};
    const GemmPlan reg = tn_plan(M, N, K);
    const GemmPlan dma = q.dtype == FMMT_BF16 ? tn_plan_dma(M, N, K) : GemmPlan{};
    const GemmPlan* const may[3] = {&few, &reg, &dma};
    int smax = 1, rows = N;
    for (const GemmPlan* c : may) {
        if (c->splits > smax) smax = c->splits;
        if (c->npad > rows) rows = c->npad;
    }
    const size_t ws_bytes = TN_HDR + (size_t)smax * ((size_t)rows * K + rows) * sizeof(float);
    const bool dma_rows = q.ldy % 8 == 0 && q.ldx % 8 == 0;       // 16-byte pieces of dy and x rows
    const bool use_few = few.splits && !q.rowscale && !q.x_epi && dma_rows;
    // single split: the "partials" ARE the result -- fmmt_linear_wgrad lets the contraction kernel write dw / db directly
    const bool direct = q.mode == GEMM_WGRAD && (use_few || smax == 1);
    GemmPlan pl = reg;
    if (q.x_epi != 0 && q.x_epi != FMMT_EPI_GELU) {
        pl.route = FMMT_EINVAL;
    } else if (use_few) {
        pl = few;                                               // one split: part_w / part_b may be dw / db themselves
        pl.route = FMMT_ROUTE_TN_FEW;
    } else if (dma.tn && !direct && !q.x_epi && dma_rows &&
               // scaled launches: the split's slice of the scale vector has to fit the 4 KB behind the ring
               (!q.rowscale || (q.rows_per_scale >= 32 && dma.tk != 192 && dma.chunk / q.rows_per_scale + 2 <= 1024))) {
        pl = dma;
        pl.route = q.rowscale ? (dma.tk == 256 ? FMMT_ROUTE_TN_DMA_256_SCALED : FMMT_ROUTE_TN_DMA_192_SCALED)
                              : dma.tk == 192 ? FMMT_ROUTE_TN_DMA_384 : dma.tk == 256 ? FMMT_ROUTE_TN_DMA_256 : FMMT_ROUTE_TN_DMA_192;
    } else if (q.dtype != FMMT_BF16) {
        pl.route = FMMT_ROUTE_TN_F32;
    } else if (M <= 4096) {
        pl.route = FMMT_ROUTE_TN_REG32_FEW;                     // few-token problems: 32-token steps, one in flight
    } else {
        // measured (tools/probes/gemm_bench.py): 64-token steps win for the compute-heavy stage-2/3 shapes (+15-25 %),
        // 32-token steps (3 workgroups per CU) win for the HBM-bound multi-million-token stage-0/1 shapes.
        // Two token steps in flight (register sets R0/R1): measured +3..5 % on the stage-2/3 shapes, +3..11 % on the stage-0/1
        // ones, at unchanged occupancy (200 / 160 registers)
        pl.route = M <= 262144 ? FMMT_ROUTE_TN_REG64 : FMMT_ROUTE_TN_REG32;
    }
    pl.direct = direct, pl.smax = smax, pl.rows = rows, pl.ws_bytes = ws_bytes;
    return pl;
}

// The plan of a query that check_query() passed.
inline GemmPlan plan_query(const GemmQuery& q) {
    if (q.mode == GEMM_WGRAD || q.mode == GEMM_WGRAD_PARTIALS) return launch_tn_plan(q);
    if (q.mode == GEMM_SEG3_N || q.mode == GEMM_SEG3_K) {
        if (!few_tiles(q.M, q.N)) return refuse(FMMT_EINVAL);      // dispatch_nt's few-tile rule: larger problems do not come here
        return nt_tiles(q.K >= SMALL_R4K ? FMMT_ROUTE_NT_SEG3_R4 : FMMT_ROUTE_NT_SEG3, q, 32, 64);
    }
    if (q.mode == GEMM_FWD) return dispatch_nt(q, 0);
    // split-K: the contraction runs as a plain product into fp32 partials [split][M][N]; bias and the output's pitch are the finish kernel's (with a
    // ksplit dispatch_nt reads no epilogue field).  The workspace size is a function of (M, N, K) alone: fmmt_linear_splitk_workspace reads it from here.
    int ks;
    const int splits = splitk_plan(q.M, q.N, q.K, &ks);
    if (!ks) return refuse(FMMT_EINVAL);                        // not a split-K shape: use fmmt_linear_fwd
    GemmPlan pl = dispatch_nt(q, ks);
    pl.ws_bytes = (size_t)splits * q.M * q.N * sizeof(float);
    return pl;
}

// what the route queries answer: the route, or the FMMT_E* of the refusal
inline int route_of(const GemmQuery& q) {
    const int rc = check_query(q);
    return rc ? rc : plan_query(q).route;
}

}  // namespace
