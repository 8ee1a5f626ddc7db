/* libfmmt_hip -- which kernel family a GEMM launch takes, asked on the host (included by fmmt.h).
 *
 * fmmt_linear_fwd, fmmt_linear_fwd_seg3, fmmt_linear_fwd_splitk and fmmt_linear_wgrad / _partials choose among some fifty kernel
 * instantiations by shape, leading dimensions, epilogue and which optional operands are present.  That choice is host arithmetic on
 * the shape alone (csrc/gemm_plan.h: check_query() validates a call, plan_query() returns its plan), and the plan's route is the index an
 * entry point takes into its table of launchers -- one entry per value below, nothing between planner and table changes a route.  The two
 * queries below call the SAME two functions on the same query and return the plan's FMMT_ROUTE_* value, or the negative FMMT_E* the entry
 * point would return.  No launch, no HIP call, no device.  Pointer arguments are replaced by presence flags (0 / non-zero); pointers count
 * as 16-byte aligned and workspaces as large enough.
 *
 * Tests use them to prove that every kernel family is exercised with leading dimensions different from the row width
 * (tests/support_gemm_cases.py); callers may use them to see where a shape lands.
 */
#ifndef FMMT_ROUTE_H
#define FMMT_ROUTE_H

#ifdef __cplusplus
extern "C" {
#endif

enum fmmt_route {
    /* NT (forward / input gradient), bf16, tokens <= 4096 */
    FMMT_ROUTE_NT_QUARTER = 1,        /* 32 x 64 quarter tiles, direct-to-LDS, two buffers */
    FMMT_ROUTE_NT_QUARTER_R4 = 2,     /* the same with a four-buffer ring (K >= 2048) */
    FMMT_ROUTE_NT_SEG3 = 3,           /* fmmt_linear_fwd_seg3: quarter tiles over three weights */
    FMMT_ROUTE_NT_SEG3_R4 = 4,
    FMMT_ROUTE_NT64_K96 = 5,          /* 64-row tiles, one K step of 96 */
    FMMT_ROUTE_NT64_K64 = 6,          /* 64-row tiles, one K step (K <= 64) */
    FMMT_ROUTE_NT64_DMA = 7,          /* 64-row tiles, BK = 64, direct-to-LDS, two buffers */
    FMMT_ROUTE_NT64_DMA_R4 = 8,       /* the same with a four-buffer ring */
    FMMT_ROUTE_NT64_BK64 = 9,         /* 64-row tiles, BK = 64, register-staged (split-K slices) */
    FMMT_ROUTE_NT64_BK32 = 10,        /* 64-row tiles, BK = 32, register-staged (K % 64 != 0) */
    FMMT_ROUTE_NT64_F32 = 11,         /* fp32 parity kernel, 64-row tiles */
    /* NT, tokens > 4096 */
    FMMT_ROUTE_NT128_K96 = 12,
    FMMT_ROUTE_NT128_K64 = 13,
    FMMT_ROUTE_NT128_DMA = 14,
    FMMT_ROUTE_NT128_BK64 = 15,
    FMMT_ROUTE_NT128_BK32 = 16,
    FMMT_ROUTE_NT128_F32 = 17,
    FMMT_ROUTE_PH = 18,               /* gemm_ph.h: 256 x 256 tiles, four phases, plain / bias */
    FMMT_ROUTE_PH3_PLAIN = 19,        /* gemm_ph3.h, 192 x 256 tiles: plain / bias */
    FMMT_ROUTE_PH3_GELU_PRE = 20,     /*   GELU + pre-activation */
    FMMT_ROUTE_PH3_OP = 21,           /*   residual and / or row scale */
    FMMT_ROUTE_PH3_MUL_AUX = 22,      /*   product with the stored GELU derivative */
    FMMT_ROUTE_PH3W_PLAIN = 23,       /* gemm_ph3.h, 384 x 128 tiles */
    FMMT_ROUTE_PH3W_OP = 24,
    FMMT_ROUTE_PH3W_MUL_AUX = 25,
    FMMT_ROUTE_P256_256 = 26,         /* persistent 256-row kernel, 256 channels wide */
    FMMT_ROUTE_P256_256_PIPE = 27,    /*   pipelined fragment reads (K >= 384) */
    FMMT_ROUTE_P256_192 = 28,
    FMMT_ROUTE_P256_192_PIPE = 29,
    FMMT_ROUTE_P256_192_OP = 30,      /*   residual / row scale prefetched into registers */
    FMMT_ROUTE_P256_128 = 31,
    FMMT_ROUTE_P256_128_PIPE = 32,
    FMMT_ROUTE_P256_128_OP = 33,
    FMMT_ROUTE_DEEP32_K96_N96 = 34,   /* 256-row deep kernels, K step 32: <3, 96> */
    FMMT_ROUTE_DEEP32_K192_N96 = 35,  /*   <6, 96> */
    FMMT_ROUTE_DEEP32_N96 = 36,       /*   <0, 96> */
    FMMT_ROUTE_DEEP32_K96_N128 = 37,
    FMMT_ROUTE_DEEP32_K192_N128 = 38,
    FMMT_ROUTE_DEEP32_N128 = 39,
    FMMT_ROUTE_DEEP = 40,             /* 256-row deep kernel, K step 64 */
    /* TN (weight gradient): the contraction kernel */
    FMMT_ROUTE_TN_FEW = 41,           /* linear_tn_few_kernel: one launch, writes dw / db */
    FMMT_ROUTE_TN_REG32_FEW = 42,     /* register-staged, 32-token steps, tokens <= 4096 */
    FMMT_ROUTE_TN_REG64 = 43,         /* register-staged, 64-token steps */
    FMMT_ROUTE_TN_REG32 = 44,         /* register-staged, 32-token steps, tokens > 262144 */
    FMMT_ROUTE_TN_F32 = 45,           /* fp32 parity kernel */
    FMMT_ROUTE_TN_DMA_256 = 46,       /* DMA-staged, 256 x 256 tiles */
    FMMT_ROUTE_TN_DMA_192 = 47,       /* DMA-staged, 192 x 384 tiles */
    FMMT_ROUTE_TN_DMA_384 = 48,       /* DMA-staged, 384 x 192 tiles (padded partials when N % 384 == 192) */
    FMMT_ROUTE_TN_DMA_256_SCALED = 49,
    FMMT_ROUTE_TN_DMA_192_SCALED = 50,
    FMMT_ROUTE_COUNT = 51
};

/* mode of fmmt_linear_fwd_route */
#define FMMT_ROUTE_MODE_FWD 0      /* fmmt_linear_fwd */
#define FMMT_ROUTE_MODE_SEG3_N 1   /* fmmt_linear_fwd_seg3, seg_mode 1 (has_bias: bias0 / 1 / 2 present) */
#define FMMT_ROUTE_MODE_SEG3_K 2   /* fmmt_linear_fwd_seg3, seg_mode 2 */
#define FMMT_ROUTE_MODE_SPLITK 3   /* fmmt_linear_fwd_splitk: the route of its contraction launch */

int fmmt_linear_fwd_route(int dtype, int M, int N, int K, int ldx, int ldw, int ldy, int has_bias, int has_y_pre, int epi,
                          int has_aux, int ldaux, int has_res, int ldres, int has_rowscale, int rows_per_scale, int mode);

/* mode 0: fmmt_linear_wgrad, 1: fmmt_linear_wgrad_partials */
int fmmt_linear_wgrad_route(int dtype, int M, int N, int K, int lddy, int ldx, int has_rowscale, int rows_per_scale, int x_epi, int mode);

#ifdef __cplusplus
}
#endif
#endif
