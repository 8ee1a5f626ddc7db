// BatchNorm1d over (n, C) rows, the bodies of the kernels of misc.hip (fmmt_batchnorm1d_fwd / _bwd) and of ragged.hip (the same with the row
// count read from the device, fmmt_batchnorm1d_fwd_n / _bwd_n): ONE statement of the arithmetic, so that a masked call over all its rows gives the
// bits of the unmasked one.
//
// A workgroup of 1024 threads = 64 columns x 16 row groups; every column sum is sixteen per-group partial sums (rows g, g + 16, ...) added in
// group order through LDS -- fixed order, two passes (mean, then centred squares).
// (One thread per column walking all n rows serially, the round-1 form, took 295 us forward and 250 us backward for the 640 x 512 head
//  of the bench step: three dependent passes of 640 loads.)
//
// MASKED: `n` rows of the `n_cap` the buffers hold are real (the caller read n from the device, once per workgroup, clamped to [0, n_cap]).
// Statistics, the running-statistics update and every column sum run over those n rows; rows [n, n_cap) of y / dx are written as zeros and
// their x / dy are never read.  n == 0: zeros everywhere, running statistics untouched.  n == 1: mean = x, variance 0, running variance
// updated with 0, dx = 0 -- what the reference's duplicate-the-sample rule gives (Swin_Transformer.forward, ref :535-538) -- by the arithmetic below;
// its one output row is written in the centred form (see there).
#pragma once
#include "fmmt_common.h"

namespace {

constexpr int BN_COLS = 64, BN_GROUPS = 16;

__device__ __forceinline__ float bn_colsum(float v, float (*red)[BN_COLS], int tc, int tg) {
    __syncthreads();                                        // the previous use of `red` is over
    red[tg][tc] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < BN_GROUPS; ++g) s += red[g][tc];
    return s;
}

// the row count of a masked launch: one read per workgroup, handed to every thread through LDS
__device__ __forceinline__ int bn_rows(const int* __restrict__ n_valid, int n_cap) {
    __shared__ int n_sh;
    if (threadIdx.x == 0) n_sh = min(max(*n_valid, 0), n_cap);
    __syncthreads();
    return n_sh;
}

template <typename T, bool MASKED>
__device__ __forceinline__ void bn1d_fwd_body(int n, int n_cap, int C, const T* __restrict__ x, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float* running_mean, float* running_var, float momentum, float eps,
                                              int training, T* __restrict__ y, float* save_mean, float* save_invstd) {
    __shared__ float red[BN_GROUPS][BN_COLS];
    const int tc = threadIdx.x % BN_COLS, tg = threadIdx.x / BN_COLS;
    const int c = blockIdx.x * BN_COLS + tc;
    const bool ok = c < C;
    if constexpr (MASKED) {
        if (n == 0) {                                       // uniform over the workgroup: nothing to normalise, nothing to track
            if (!ok) return;
            if (tg == 0) {
                if (save_mean) save_mean[c] = 0.f;
                if (save_invstd) save_invstd[c] = 0.f;
            }
            for (int r = tg; r < n_cap; r += BN_GROUPS) y[(size_t)r * C + c] = from_f32<T>(0.f);
            return;
        }
    }
    float mean, invstd;
    if (training) {
        float s = 0.f;
        if (ok)
            for (int r = tg; r < n; r += BN_GROUPS) s += to_f32(x[(size_t)r * C + c]);
        mean = bn_colsum(s, red, tc, tg) / n;
        float q = 0.f;
        if (ok)
            for (int r = tg; r < n; r += BN_GROUPS) {
                const float d = to_f32(x[(size_t)r * C + c]) - mean;
                q += d * d;
            }
        q = bn_colsum(q, red, tc, tg);
        const float var = q / n;
        invstd = rsqrtf(var + eps);
        if (ok && tg == 0) {
            running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * (n > 1 ? q / (n - 1) : var);
        }
    } else {
        mean = ok ? running_mean[c] : 0.f;
        invstd = ok ? rsqrtf(running_var[c] + eps) : 0.f;
    }
    if (!ok) return;
    if (tg == 0) {
        if (save_mean) save_mean[c] = mean;
        if (save_invstd) save_invstd[c] = invstd;
    }
    const float g = gamma[c] * invstd, b = beta[c] - mean * g;
    bool centred = false;
    if constexpr (MASKED) centred = training && n == 1;
    if (centred) {
        // One real row: variance 0, invstd = 1 / sqrt(eps) ~ 316, and the folded offset b = beta - mean g is rounded at the magnitude of mean g (measured:
        // y off beta by 1.5e-5 where |beta| <= 0.1).  The reference's duplicate-the-sample rule normalises the centred value, (x - mean) invstd gamma + beta
        // = beta exactly; so does this row.  (Only here: everywhere else the folded form keeps the bits of the unmasked kernel.)
        if (tg == 0) y[c] = from_f32<T>((to_f32(x[c]) - mean) * g + beta[c]);
    } else {
        for (int r = tg; r < n; r += BN_GROUPS) y[(size_t)r * C + c] = from_f32<T>(to_f32(x[(size_t)r * C + c]) * g + b);
    }
    if constexpr (MASKED) {
        const int pad0 = n + (tg - n % BN_GROUPS + BN_GROUPS) % BN_GROUPS;       // first row >= n of this thread's group
        for (int r = pad0; r < n_cap; r += BN_GROUPS) y[(size_t)r * C + c] = from_f32<T>(0.f);
    }
}

template <typename T, bool MASKED>
__device__ __forceinline__ void bn1d_bwd_body(int n, int n_cap, int C, const T* __restrict__ dy, const T* __restrict__ x,
                                              const float* __restrict__ gamma, const float* __restrict__ save_mean,
                                              const float* __restrict__ save_invstd, int training, T* __restrict__ dx, float* dgamma, float* dbeta) {
    __shared__ float red[BN_GROUPS][BN_COLS];
    const int tc = threadIdx.x % BN_COLS, tg = threadIdx.x / BN_COLS;
    const int c = blockIdx.x * BN_COLS + tc;
    const bool ok = c < C;
    if constexpr (MASKED) {
        if (n == 0) {
            if (!ok) return;
            if (tg == 0) {
                if (dgamma) dgamma[c] = 0.f;
                if (dbeta) dbeta[c] = 0.f;
            }
            for (int r = tg; r < n_cap; r += BN_GROUPS) dx[(size_t)r * C + c] = from_f32<T>(0.f);
            return;
        }
    }
    const float mean = ok ? save_mean[c] : 0.f, invstd = ok ? save_invstd[c] : 0.f;
    float sb = 0.f, sg = 0.f;
    if (ok)
        for (int r = tg; r < n; r += BN_GROUPS) {
            const float g = to_f32(dy[(size_t)r * C + c]);
            sb += g;
            sg += g * (to_f32(x[(size_t)r * C + c]) - mean) * invstd;
        }
    sb = bn_colsum(sb, red, tc, tg);
    sg = bn_colsum(sg, red, tc, tg);
    if (!ok) return;
    if (tg == 0) {
        if (dgamma) dgamma[c] = sg;
        if (dbeta) dbeta[c] = sb;
    }
    const float k = gamma[c] * invstd;
    if (training) {
        const float inv_n = 1.f / n;
        for (int r = tg; r < n; r += BN_GROUPS) {
            const float xh = (to_f32(x[(size_t)r * C + c]) - mean) * invstd;
            dx[(size_t)r * C + c] = from_f32<T>(k * (to_f32(dy[(size_t)r * C + c]) - sb * inv_n - xh * sg * inv_n));
        }
    } else {
        for (int r = tg; r < n; r += BN_GROUPS) dx[(size_t)r * C + c] = from_f32<T>(k * to_f32(dy[(size_t)r * C + c]));
    }
    if constexpr (MASKED) {
        const int pad0 = n + (tg - n % BN_GROUPS + BN_GROUPS) % BN_GROUPS;
        for (int r = pad0; r < n_cap; r += BN_GROUPS) dx[(size_t)r * C + c] = from_f32<T>(0.f);
    }
}

}  // namespace
