// What the two on-device augmentations of the uint8 pre-step share (color_jitter.hip: the MELD ColorJitter; aff_augment.hip: the Aff-Wild2 chain): the
// jitter record, the exactly rounded arithmetic of the four Pillow operations, the band resize and the contrast statistic.  Everything is in an
// anonymous namespace: each of the two translation units gets its own copy.
#pragma once
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
// WORDS: the record's pitch in the table (the jitter record is its first 8 words).  GRAY_WORD >= 0: bit 0 of that word puts Grayscale(3) in front of
// the frame's operations (aff_augment.hip's record).
template <bool PIL, int WORDS = FMMT_JITTER_WORDS, int GRAY_WORD = -1>
__global__ __launch_bounds__(256) void jitter_stats_kernel(const uint8_t* __restrict__ img, int S, const int32_t* __restrict__ tab,
                                                           const int32_t* __restrict__ jit, int32_t* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) uint8_t src[RMAX * SMAX * 3];
    __shared__ __attribute__((aligned(16))) uint8_t rb[4 * ROWB];
    __shared__ int wsum[4];
    const int p = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const JitRec j = load_rec(jit + (size_t)n * (WORDS - FMMT_JITTER_WORDS), n);
    if (!has_contrast(j)) return;                            // uniform: nobody reads this frame's partials
    bool gray = false;
    if constexpr (GRAY_WORD >= 0) gray = jit[(size_t)n * WORDS + GRAY_WORD] & 1;
    resize_band<PIL>(img, S, tab, p, n, tid, src, rb);
    int sum = 0;
    for (int q = tid; q < 4 * OUT; q += 256) {
        int r = rb[q * 3], g = rb[q * 3 + 1], b = rb[q * 3 + 2];
        if (gray) r = g = b = luma(r, g, b);
        jitter_px<true>(r, g, b, j, 0.f);
        sum += luma(r, g, b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) partial[(size_t)n * GRID + p] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

}  // namespace
