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
#include "fmmt_common.h"
#include "../../include/fmmt.h"
#include "patch_ln_core.h"
#include <math.h>

namespace {

constexpr int OUT = 224, GRID = 56, KPATCH = 48;
constexpr int RMAX = 8;              // source rows a band of 4 output rows may touch (fmmt_resize_band_rows)
constexpr int SMAX = 224;            // largest source edge (up-scaling only)
constexpr int CPITCH = 56;           // LDS pitch of a patch row, as in preproc.hip
constexpr int ROWB = OUT * 3;        // bytes of a resized row
constexpr int NPIX = OUT * OUT;

template <typename T>
struct PeTail {                      // the projection + LayerNorm behind the gather (FUSE)
    const T* w;
    const float* bias;
    const float* gamma;
    const float* beta;
    float eps;
    T* x_pre;
    T* y;
    float* mean;
    float* rstd;
};

struct JitRec {                      // one record of the table, in scalar registers (the address is workgroup-uniform)
    float fb, fc, fs;
    int shift;
    int op[4];
};
__device__ __forceinline__ JitRec load_rec(const int32_t* __restrict__ jit, int n) {
    const int32_t* r = jit + (size_t)n * FMMT_JITTER_WORDS;
    JitRec j;
    j.fb = __int_as_float(r[0]);
    j.fc = __int_as_float(r[1]);
    j.fs = __int_as_float(r[2]);
    j.shift = r[3] & 255;
#pragma unroll
    for (int k = 0; k < 4; ++k) j.op[k] = r[4 + k];
    return j;
}
__device__ __forceinline__ bool has_contrast(const JitRec& j) {
    return j.op[0] == FMMT_JITTER_CONTRAST || j.op[1] == FMMT_JITTER_CONTRAST || j.op[2] == FMMT_JITTER_CONTRAST || j.op[3] == FMMT_JITTER_CONTRAST;
}

// one rounding per operation, whatever the contraction mode
__device__ __forceinline__ float mul_f(float a, float b) { float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float add_f(float a, float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float sub_f(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double mul_d(double a, double b) { double r; asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double add_d(double a, double b) { double r; asm("v_add_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double sub_d(double a, double b) { return add_d(a, -b); }

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate, image, f): d + f * (x - d) in float32, clipped, truncated
__device__ __forceinline__ int blend(float d, float f, int x) {
    const float t = add_f(d, mul_f(f, sub_f((float)x, d)));
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ int round8(double x) { return clip8((int)round(x)); }          // C round: half away from zero

// Pillow's rgb2hsv, H += shift (mod 256), hsv2rgb (src/libImaging/Convert.c): float / double mixed exactly as there
__device__ __forceinline__ void hue_px(int& r, int& g, int& b, int shift) {
    const int mx = max(max(r, g), b), mn = min(min(r, g), b);
    int H = 0, S = 0;
    const int V = mx;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = __fdiv_rn(cr, (float)mx);
        const float rc = __fdiv_rn((float)(mx - r), cr), gc = __fdiv_rn((float)(mx - g), cr), bc = __fdiv_rn((float)(mx - b), cr);
        float h;
        if (r == mx) h = sub_f(bc, gc);
        else if (g == mx) h = (float)sub_d(add_d(2.0, (double)rc), (double)bc);
        else h = (float)sub_d(add_d(4.0, (double)gc), (double)rc);
        const double hd = add_d(__ddiv_rn((double)h, 6.0), 1.0);                          // in [5/6, 2): fmod(hd, 1.0) = hd - floor(hd), exact
        h = (float)sub_d(hd, floor(hd));
        H = clip8((int)mul_d((double)h, 255.0));
        S = clip8((int)mul_d((double)s, 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double fh = __ddiv_rn(mul_d((double)H, 6.0), 255.0);
    const double fi = floor(fh);                                                          // 0 .. 6 (H = 255: exactly 6, sector 0)
    const float f = (float)sub_d(fh, fi);
    const float fs = (float)__ddiv_rn((double)S, 255.0);
    const double v = (double)V, dfs = (double)fs, df = (double)f;
    const int p = round8(mul_d(v, sub_d(1.0, dfs)));
    const int q = round8(mul_d(v, sub_d(1.0, mul_d(dfs, df))));
    const int t = round8(mul_d(v, sub_d(1.0, mul_d(dfs, sub_d(1.0, df)))));
    int i = (int)fi;
    i = i >= 6 ? i - 6 : i;
    switch (i) {
        case 0: r = V; g = t; b = p; break;
        case 1: r = q; g = V; b = p; break;
        case 2: r = p; g = V; b = t; break;
        case 3: r = p; g = q; b = V; break;
        case 4: r = t; g = p; b = V; break;
        default: r = V; g = p; b = q; break;
    }
}

// a pixel through its frame's operations.  STATS: stop in front of contrast (the statistic is taken there).  `m`: the frame's mean luma, used by the
// FIRST contrast of a record; a second one, like any unknown code, is "none" (fmmt_jitter_table_check refuses both on the host).
template <bool STATS>
__device__ __forceinline__ void jitter_px(int& r, int& g, int& b, const JitRec& j, float m) {
    bool seen = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = j.op[k];                                                           // workgroup-uniform: scalar branches
        if (op == FMMT_JITTER_BRIGHTNESS) {
            r = blend(0.f, j.fb, r);
            g = blend(0.f, j.fb, g);
            b = blend(0.f, j.fb, b);
        } else if (op == FMMT_JITTER_CONTRAST) {
            if constexpr (STATS) return;
            if (!seen) {
                r = blend(m, j.fc, r);
                g = blend(m, j.fc, g);
                b = blend(m, j.fc, b);
            }
            seen = true;
        } else if (op == FMMT_JITTER_SATURATION) {
            const float d = (float)luma(r, g, b);
            r = blend(d, j.fs, r);
            g = blend(d, j.fs, g);
            b = blend(d, j.fs, b);
        } else if (op == FMMT_JITTER_HUE) {
            hue_px(r, g, b, j.shift);
        }
    }
}

// preproc.hip's steps 1-3 for band p of image n, the four resized rows written as bytes: rb[dy * ROWB + x * 3 + c].  Ends with a barrier.
template <bool PIL>
__device__ __forceinline__ void resize_band(const uint8_t* __restrict__ img, int S, const int32_t* __restrict__ tab, int p, int n, int tid, uint8_t* src,
                                            uint8_t* rb) {
    int tyi[4][4], tyw[4][4];
    int ymin = S, ymax = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tyi[j][k] = tab[(4 * p + j) * 8 + k];
            tyw[j][k] = tab[(4 * p + j) * 8 + 4 + k];
            ymin = min(ymin, tyi[j][k]);
            ymax = max(ymax, tyi[j][k]);
        }
    ymin = min(max(ymin, 0), S - 1);                         // a table that is not fmmt_resize_table's cannot send the staging out of the image
    const int nr = min(ymax - ymin + 1, min(RMAX, S - ymin));
    int W[4][RMAX];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            int w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) w += (tyi[j][k] - ymin == r) ? tyw[j][k] : 0;
            W[j][r] = w;
        }
    const int rowb = S * 3;
    const uint8_t* base = img + ((size_t)n * S + ymin) * rowb;
    const int nbytes = nr * rowb;
    const int mis = (int)((uintptr_t)base & 3);
    const int head = mis ? min(4 - mis, nbytes) : 0;
    if (tid < head) src[tid] = base[tid];
    const int words = (nbytes - head) >> 2;
    const uint32_t* b4 = reinterpret_cast<const uint32_t*>(base + head);
    for (int i = tid; i < words; i += 256) {
        const uint32_t v = b4[i];
        const int o = head + 4 * i;
        src[o] = (uint8_t)v;
        src[o + 1] = (uint8_t)(v >> 8);
        src[o + 2] = (uint8_t)(v >> 16);
        src[o + 3] = (uint8_t)(v >> 24);
    }
    for (int i = head + 4 * words + tid; i < nbytes; i += 256) src[i] = base[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int rem = tid + 256 * i;                       // output column: x = rem / 3, channel c = rem % 3
        if (rem >= ROWB) break;
        const int x = rem / 3, c = rem - 3 * x;
        const int4 ti = *reinterpret_cast<const int4*>(tab + x * 8), tw = *reinterpret_cast<const int4*>(tab + x * 8 + 4);
        const int lim = S - 1;
        const int o0 = min(max(ti.x, 0), lim) * 3 + c, o1 = min(max(ti.y, 0), lim) * 3 + c, o2 = min(max(ti.z, 0), lim) * 3 + c, o3 = min(max(ti.w, 0), lim) * 3 + c;
        int h[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            if (r < nr) {                                    // uniform
                const uint8_t* s = src + r * rowb;
                int32_t acc = PIL ? (1 << 21) : 0;
                acc += (int32_t)s[o0] * tw.x + (int32_t)s[o1] * tw.y + (int32_t)s[o2] * tw.z + (int32_t)s[o3] * tw.w;
                h[r] = PIL ? min(max(acc >> 22, 0), 255) : acc;
            } else {
                h[r] = 0;
            }
        }
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            int32_t acc = 1 << 21;
#pragma unroll
            for (int r = 0; r < RMAX; ++r) acc += h[r] * W[dy][r];
            rb[dy * ROWB + rem] = (uint8_t)min(max(acc >> 22, 0), 255);
        }
    }
    __syncthreads();
}

// block = (patch row p, image n); 256 threads: the band's sum of L in front of the frame's contrast -> partial[n * 56 + p]
template <bool PIL>
__global__ __launch_bounds__(256) void jitter_stats_kernel(const uint8_t* __restrict__ img, int S, const int32_t* __restrict__ tab,
                                                           const int32_t* __restrict__ jit, int32_t* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) uint8_t src[RMAX * SMAX * 3];
    __shared__ __attribute__((aligned(16))) uint8_t rb[4 * ROWB];
    __shared__ int wsum[4];
    const int p = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const JitRec j = load_rec(jit, n);
    if (!has_contrast(j)) return;                            // uniform: nobody reads this frame's partials
    resize_band<PIL>(img, S, tab, p, n, tid, src, rb);
    int sum = 0;
    for (int q = tid; q < 4 * OUT; q += 256) {
        int r = rb[q * 3], g = rb[q * 3 + 1], b = rb[q * 3 + 2];
        jitter_px<true>(r, g, b, j, 0.f);
        sum += luma(r, g, b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) partial[(size_t)n * GRID + p] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

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
