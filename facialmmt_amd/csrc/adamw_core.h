// Clip + AdamW + bf16 twins over a descriptor table: the body of adamw_batch_kernel (misc.hip, fmmt_adamw_batch), of adamw_batch_guarded_kernel
// (guard.hip, fmmt_adamw_batch_guarded) and of the two kernels of adamw_groups.hip (fmmt_adamw_groups, fmmt_adamw_groups_guarded) -- ONE statement
// of the arithmetic, so that the guarded update on a finite norm gives the bits of the plain one and the grouped update the bits of one plain
// launch per group.  The kernels differ only in where `t`, the hyper-parameters and the decision to run at all come from; the formulas and the
// descriptor record are described above adamw_batch_kernel and in include/fmmt.h.
#pragma once
#include "fmmt_common.h"

namespace {

struct AdamDesc {
    float* p; const void* g; float* m; float* v; bf16* low;     // low may be null
    long long n;
    int blk_begin, g_bf16;                                      // g_bf16: the gradient is bf16 (the twin's own .grad), else fp32
};

// what one record is stepped with: launch arguments in the one-group kernels, groups[group_of[record]] in the grouped ones -- block-uniform either way
struct AdamHyper {
    float lr, beta1, beta2, eps, wd;
};

// NaN and +-inf have every exponent bit set: a test on the bits, which no floating-point compiler option can fold away (the guarded kernels'
// decision, and fmmt_guard_commit's behind them)
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// the record block `blockIdx.x` belongs to: the last one whose blk_begin is not behind it
__device__ __forceinline__ int adamw_find_record(const AdamDesc* __restrict__ desc, int n_desc) {
    int lo = 0, hi = n_desc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].blk_begin <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One block = 4096 elements of one record.  STEP_IS_BEFORE: *step_p is the update count BEFORE this update (the guarded kernel, whose step word
// another kernel advances behind it), t = *step_p + 1; else *step_p is t itself.  coef = min(1, max_norm / (total_norm + 1e-6)) is
// torch.nn.utils.clip_grad_norm_'s.
template <bool STEP_IS_BEFORE>
__device__ __forceinline__ void adamw_batch_body(const AdamDesc d, const AdamHyper h, const float* __restrict__ step_p,
                                                 const float* __restrict__ norm_p, float max_norm, int hf) {
    const float lr = h.lr, beta1 = h.beta1, beta2 = h.beta2, eps = h.eps, wd = h.wd;
    const float t = STEP_IS_BEFORE ? *step_p + 1.0f : *step_p;
    const float coef = norm_p ? fminf(1.0f, max_norm / (*norm_p + 1e-6f)) : 1.0f;
    const float bc1 = 1.0f - powf(beta1, t), bc2s = sqrtf(1.0f - powf(beta2, t));
    const float step_size = hf ? lr * bc2s / bc1 : lr / bc1, decay = hf ? 1.0f : 1.0f - lr * wd;
    const float den_div = hf ? 1.0f : bc2s, post = hf ? -lr * wd : 0.0f;
    const long long base = (long long)((int)blockIdx.x - d.blk_begin) * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long o = base + (long long)(i * 256 + threadIdx.x) * 4;
        if (o >= d.n) break;
        const float* gf = reinterpret_cast<const float*>(d.g);
        const bf16* gb = reinterpret_cast<const bf16*>(d.g);
        const bool g_ok = d.g_bf16 ? (reinterpret_cast<uintptr_t>(gb + o) & 7) == 0 : (reinterpret_cast<uintptr_t>(gf + o) & 15) == 0;
        if (o + 4 <= d.n && g_ok && ((reinterpret_cast<uintptr_t>(d.p + o) | reinterpret_cast<uintptr_t>(d.m + o) |
                                       reinterpret_cast<uintptr_t>(d.v + o)) & 15) == 0) {
            f32x4 p = *reinterpret_cast<const f32x4*>(d.p + o), g;
            if (d.g_bf16) {
                const bf16x4 t = *reinterpret_cast<const bf16x4*>(gb + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = (float)t[e];
            } else {
                g = *reinterpret_cast<const f32x4*>(gf + o);
            }
            f32x4 m = *reinterpret_cast<const f32x4*>(d.m + o), v = *reinterpret_cast<const f32x4*>(d.v + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ge = g[e] * coef;
                p[e] *= decay;
                m[e] = beta1 * m[e] + (1.0f - beta1) * ge;
                v[e] = beta2 * v[e] + (1.0f - beta2) * ge * ge;
                p[e] -= step_size * (m[e] / (sqrtf(v[e]) / den_div + eps));
                p[e] = fmaf(p[e], post, p[e]);
            }
            *reinterpret_cast<f32x4*>(d.p + o) = p;
            *reinterpret_cast<f32x4*>(d.m + o) = m;
            *reinterpret_cast<f32x4*>(d.v + o) = v;
            if (d.low) {
                if ((reinterpret_cast<uintptr_t>(d.low + o) & 7) == 0) {
                    bf16x4 l;
#pragma unroll
                    for (int e = 0; e < 4; ++e) l[e] = (bf16)p[e];
                    *reinterpret_cast<bf16x4*>(d.low + o) = l;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) d.low[o + e] = (bf16)p[e];
                }
            }
        } else {
            for (long long j = o; j < d.n && j < o + 4; ++j) {
                const float ge = (d.g_bf16 ? (float)gb[j] : gf[j]) * coef;
                float p = d.p[j] * decay;
                const float m = beta1 * d.m[j] + (1.0f - beta1) * ge;
                const float v = beta2 * d.v[j] + (1.0f - beta2) * ge * ge;
                p -= step_size * (m / (sqrtf(v) / den_div + eps));
                p = fmaf(p, post, p);
                d.p[j] = p;
                d.m[j] = m;
                d.v[j] = v;
                if (d.low) d.low[j] = (bf16)p;
            }
        }
    }
}

}  // namespace
