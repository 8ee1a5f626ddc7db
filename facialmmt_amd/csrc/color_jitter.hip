// The MELD training ColorJitter (utils/dataset.py:35-39,62-63: torchvision ColorJitter(.5, .5, .5, .5) on the resized uint8 face) inside the uint8
// pre-step: bicubic resize -> the frame's brightness / contrast / saturation / hue operations in the frame's order, on bytes, each rounding to uint8 as
// Pillow does -> ToTensor / Normalize table -> 4x4 patch gather (-> PatchEmbed's projection + LayerNorm).  include/fmmt_jitter.h states the arithmetic;
// tests/support_color_jitter.py restates it in numpy and is held to Pillow bit for bit.
//
// The resize is preproc.hip's (same tables, same integer sums), except that a band's four resized rows land in LDS as BYTES (4 x 224 x 3): the jitter needs
// a pixel's three channels together, where the resize gives a thread one (x, channel) column.  A thread then owns pixels tid, tid + 256, ... of the band.
// Contrast blends with the mean luma of the WHOLE frame as it is when contrast is applied, so there are two launches on the same grid:
//   jitter_stats_kernel  resize, the operations in front of contrast, the band's integer sum of L -> partial[n][56]     (frames without contrast: exit)
//   jitter_main_kernel   resize, sum the frame's 56 integers, every operation, table, gather (, projection + LayerNorm)
// Integer sums: exact and order-free, no atomics, nothing to zero.
//
// Rounding.  The library is built with -ffp-contract=fast, and Pillow rounds every product before the sum that follows it: the products and sums of the blend
// and of the HSV conversions are single instructions behind inline asm, which the compiler can neither fuse nor re-associate.
#include "jitter_core.h"

namespace {

// block = (patch row p, image n); 256 threads: preproc.hip's kernel with the jitter between the resize's bytes and the table
template <typename T, bool PIL, bool FUSE>
__global__ __launch_bounds__(256) void jitter_main_kernel(const uint8_t* __restrict__ img, int S, const int32_t* __restrict__ tab,
                                                          const float* __restrict__ lut, const int32_t* __restrict__ jit,
                                                          const int32_t* __restrict__ partial, T* __restrict__ cols, PeTail<T> tail) {
    __shared__ __attribute__((aligned(16))) uint8_t src[RMAX * SMAX * 3];
    __shared__ __attribute__((aligned(16))) uint8_t rb[4 * ROWB];
    __shared__ __attribute__((aligned(16))) T colsl[64 * CPITCH];
    __shared__ float slut[256];
    const int p = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    slut[tid] = lut[tid];
    const JitRec j = load_rec(jit, n);
    float m = 0.f;
    if (has_contrast(j)) {                                   // uniform addresses: scalar loads; Pillow's int(mean + 0.5) in integers
        int total = 0;
        for (int q = 0; q < GRID; ++q) total += partial[(size_t)n * GRID + q];
        m = (float)((2 * total + NPIX) / (2 * NPIX));
    }
    if constexpr (FUSE) {
        for (int e = tid; e < 8 * KPATCH; e += 256) colsl[(GRID + e / KPATCH) * CPITCH + e % KPATCH] = from_f32<T>(0.f);   // rows 56-63 of the last wave's tile
    }
    resize_band<PIL>(img, S, tab, p, n, tid, src, rb);       // (its barriers cover slut and the tile's zero rows)
    for (int q = tid; q < 4 * OUT; q += 256) {
        const int dy = q / OUT, x = q - dy * OUT;
        int r = rb[q * 3], g = rb[q * 3 + 1], b = rb[q * 3 + 2];
        jitter_px<false>(r, g, b, j, m);
        T* o = colsl + (x >> 2) * CPITCH + dy * 4 + (x & 3);
        o[0] = from_f32<T>(slut[r]);
        o[16] = from_f32<T>(slut[g]);
        o[32] = from_f32<T>(slut[b]);
    }
    __syncthreads();
    if (!FUSE || cols) {                                     // the patch matrix of the band: 56 rows of 48 values, whole 16-byte chunks
        constexpr int CH = 16 / (int)sizeof(T), CPR = KPATCH / CH;
        T* out = cols + ((size_t)n * GRID + p) * GRID * KPATCH;
        for (int q = tid; q < GRID * CPR; q += 256) {
            const int patch = q / CPR, ch = q - patch * CPR;
            *reinterpret_cast<uint4*>(out + patch * KPATCH + ch * CH) = *reinterpret_cast<const uint4*>(colsl + patch * CPITCH + ch * CH);
        }
    }
    if constexpr (FUSE) {
        using E = ElemTrait<T>;
        const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
        const int patch = wave * 16 + li;
        const typename E::frag c0 = E::ld(colsl + patch * CPITCH + lg * 8);
        const typename E::frag c1 = lg < 2 ? E::ld(colsl + patch * CPITCH + 32 + lg * 8) : E::zero();
        patch_ln_tile_lean<T>(tail.w, tail.bias, tail.gamma, tail.beta, c0, c1, tail.eps, ((size_t)n * GRID + p) * GRID + patch, patch < GRID, li, lg,
                              tail.x_pre, tail.y, tail.mean, tail.rstd);
    }
}

template <typename T, bool FUSE>
int launch(int mode, int n_img, int in_size, const uint8_t* img, const int32_t* tab, const float* lut, const int32_t* jit, int32_t* partial, T* cols,
           const PeTail<T>& tail, hipStream_t st) {
    dim3 grid(GRID, n_img);
    if (mode == FMMT_RESIZE_PIL) {
        hipLaunchKernelGGL((jitter_stats_kernel<true>), grid, dim3(256), 0, st, img, in_size, tab, jit, partial);
        hipLaunchKernelGGL((jitter_main_kernel<T, true, FUSE>), grid, dim3(256), 0, st, img, in_size, tab, lut, jit, partial, cols, tail);
    } else {
        hipLaunchKernelGGL((jitter_stats_kernel<false>), grid, dim3(256), 0, st, img, in_size, tab, jit, partial);
        hipLaunchKernelGGL((jitter_main_kernel<T, false, FUSE>), grid, dim3(256), 0, st, img, in_size, tab, lut, jit, partial, cols, tail);
    }
    FMMT_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int fmmt_jitter_table_check(const int32_t* table, int n_img) {
    if (!table || n_img <= 0) return FMMT_EINVAL;
    for (int i = 0; i < n_img; ++i) {
        int seen = 0;
        for (int k = 0; k < 4; ++k) {
            const int op = table[(size_t)i * FMMT_JITTER_WORDS + 4 + k];
            if (op < 0 || op > FMMT_JITTER_NONE) return FMMT_EINVAL;
            if (op != FMMT_JITTER_NONE && (seen & (1 << op))) return FMMT_EINVAL;
            seen |= 1 << op;
        }
        if (table[(size_t)i * FMMT_JITTER_WORDS + 3] < 0 || table[(size_t)i * FMMT_JITTER_WORDS + 3] > 255) return FMMT_EINVAL;
    }
    return 0;
}

extern "C" int fmmt_patch_embed_u8_jitter(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev, const float* lut_dev,
                                          const int32_t* jitter_dev, int32_t* partial, void* cols, void* stream) {
    if ((dtype != FMMT_BF16 && dtype != FMMT_F32) || (mode != FMMT_RESIZE_PIL && mode != FMMT_RESIZE_CV2)) return FMMT_EINVAL;
    if (n_img <= 0 || n_img > 65535 || in_size < 4 || in_size > SMAX || !img_u8 || !table_dev || !lut_dev || !cols || !jitter_dev || !partial) return FMMT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(table_dev) | reinterpret_cast<uintptr_t>(cols)) & 15) return FMMT_EALIGN;
    if ((reinterpret_cast<uintptr_t>(jitter_dev) | reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(lut_dev)) & 3) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t* img = reinterpret_cast<const uint8_t*>(img_u8);
    if (dtype == FMMT_BF16) return launch<bf16, false>(mode, n_img, in_size, img, table_dev, lut_dev, jitter_dev, partial, (bf16*)cols, PeTail<bf16>{}, st);
    return launch<float, false>(mode, n_img, in_size, img, table_dev, lut_dev, jitter_dev, partial, (float*)cols, PeTail<float>{}, st);
}

extern "C" int fmmt_patch_embed_u8_jitter_ln_fwd(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev,
                                                 const float* lut_dev, const int32_t* jitter_dev, int32_t* partial, const void* w, const float* bias,
                                                 const float* ln_gamma, const float* ln_beta, float eps, void* cols, void* x_pre, void* y, float* mean,
                                                 float* rstd, void* stream) {
    if ((dtype != FMMT_BF16 && dtype != FMMT_F32) || (mode != FMMT_RESIZE_PIL && mode != FMMT_RESIZE_CV2)) return FMMT_EINVAL;
    if (n_img <= 0 || n_img > 65535 || in_size < 4 || in_size > SMAX || !img_u8 || !table_dev || !lut_dev || !jitter_dev || !partial) return FMMT_EINVAL;
    if (!w || !ln_gamma || !ln_beta || !y || (mean == nullptr) != (rstd == nullptr)) return FMMT_EINVAL;
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!al16(w) || !al16(y) || (x_pre && !al16(x_pre)) || (cols && !al16(cols)) || !al16(table_dev) || (bias && !al16(bias)) || !al16(ln_gamma) || !al16(ln_beta))
        return FMMT_EALIGN;
    if ((reinterpret_cast<uintptr_t>(jitter_dev) | reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(lut_dev)) & 3) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t* img = reinterpret_cast<const uint8_t*>(img_u8);
    if (dtype == FMMT_BF16) {
        const PeTail<bf16> t{(const bf16*)w, bias, ln_gamma, ln_beta, eps, (bf16*)x_pre, (bf16*)y, mean, rstd};
        return launch<bf16, true>(mode, n_img, in_size, img, table_dev, lut_dev, jitter_dev, partial, (bf16*)cols, t, st);
    }
    const PeTail<float> t{(const float*)w, bias, ln_gamma, ln_beta, eps, (float*)x_pre, (float*)y, mean, rstd};
    return launch<float, true>(mode, n_img, in_size, img, table_dev, lut_dev, jitter_dev, partial, (float*)cols, t, st);
}
