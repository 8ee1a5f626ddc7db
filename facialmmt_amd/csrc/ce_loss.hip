// The training loss of the (B, NL) logits of the target and auxiliary steps (train.py:26,135: criterion(logits, labels)) as the value a run chooses:
// torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps, reduction='mean'), one launch per direction (include/fmmt_loss.h states the formulas).
//
//   forward : ONE workgroup of 1024 threads.  Leaf `tid` walks its rows tid, tid + 1024, ... in that order (a row is NL <= 8 values: max, sum of
//             exp, log -- all in registers) and adds the row's numerator and its weight; the 1024 (num, den) pairs meet in LDS in the fixed 10-level
//             tree of eval_accumulate_body (eval.hip).  No atomics: two runs give the same bits.  loss = num / den, 0 when den == 0.
//   backward: a thread per row recomputes the row's softmax and writes dloss / den * (p * sum_c t_c - t); dloss and den are device words.
// The problem is launch count, not bytes (B = 4..150 rows of 7 values): torch's cross_entropy is a chain of 2-4 us launches in each direction.
// FMMT_BF16: logits / dlogits bf16, all arithmetic fp32;  FMMT_F32: the same template, nothing rounded.
#include "fmmt_common.h"
#include "../../include/fmmt.h"

namespace {

constexpr int CE_THREADS = 1024, CE_BWD_THREADS = 256, CE_MAXNL = 8, CE_MAXB = 65536;

// what both directions need of one row: the values, their maximum, sum_c exp(x_c - max); the class weights (1 without a table) and their sum
template <typename T>
__device__ __forceinline__ void ce_row(const T* __restrict__ row, int NL, float (&v)[CE_MAXNL], float& m, float& z) {
    m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CE_MAXNL; ++c) {
        v[c] = c < NL ? (float)row[c] : -INFINITY;
        m = fmaxf(m, v[c]);
    }
    z = 0.f;
#pragma unroll
    for (int c = 0; c < CE_MAXNL; ++c) z += c < NL ? expf(v[c] - m) : 0.f;
}

__device__ __forceinline__ float ce_weights(const float* __restrict__ class_w, int NL, float (&w)[CE_MAXNL]) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CE_MAXNL; ++c) {
        w[c] = c < NL ? (class_w != nullptr ? class_w[c] : 1.f) : 0.f;
        sum += w[c];
    }
    return sum;
}

template <typename T>
__global__ __launch_bounds__(CE_THREADS) void ce_fwd_kernel(int B, int NL, const T* __restrict__ logits, int ld, const long long* __restrict__ labels,
                                                            const float* __restrict__ class_w, float eps, float* __restrict__ loss,
                                                            float* __restrict__ den) {
    __shared__ float rn[CE_THREADS], rd[CE_THREADS];
    const int tid = threadIdx.x;
    float w[CE_MAXNL];
    ce_weights(class_w, NL, w);
    const float k2 = eps / (float)NL;
    float num = 0.f, dn = 0.f;
    for (int i = tid; i < B; i += CE_THREADS) {             // the leaf's rows in their order
        const long long label = labels[i];
        if (label < 0 || label >= NL) continue;             // ignored: adds nothing (torch's ignore_index; a padded row's -100)
        float v[CE_MAXNL], m, z;
        ce_row<T>(logits + (size_t)i * ld, NL, v, m, z);
        const float lse = m + logf(z);
        float vy = 0.f, wy = 0.f;
#pragma unroll
        for (int c = 0; c < CE_MAXNL; ++c) {
            vy = c == (int)label ? v[c] : vy;
            wy = c == (int)label ? w[c] : wy;
        }
        float rl = (1.0f - eps) * wy * (lse - vy);
        if (eps > 0.f) {                                    // the smoothing term: every class's -log p, weighted; stays when w[y] == 0
            float t2 = 0.f;
#pragma unroll
            for (int c = 0; c < CE_MAXNL; ++c) t2 += c < NL ? w[c] * (lse - v[c]) : 0.f;
            rl = fmaf(k2, t2, rl);
        }
        num += rl;
        dn += wy;
    }
    rn[tid] = num;
    rd[tid] = dn;
    __syncthreads();
    for (int s = CE_THREADS / 2; s > 0; s >>= 1) {          // the same 1024-leaf tree for every B: a fixed summation order
        if (tid < s) {
            rn[tid] += rn[tid + s];
            rd[tid] += rd[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {                                         // ordinary vector stores
        den[0] = rd[0];
        loss[0] = rd[0] > 0.f ? rn[0] / rd[0] : 0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(CE_BWD_THREADS) void ce_bwd_kernel(int B, int NL, const T* __restrict__ logits, int ld, const long long* __restrict__ labels,
                                                                const float* __restrict__ class_w, float eps, const float* __restrict__ dloss,
                                                                const float* __restrict__ den, T* __restrict__ dlogits, int ld_d) {
    const int i = blockIdx.x * CE_BWD_THREADS + threadIdx.x;
    if (i >= B) return;
    T* out = dlogits + (size_t)i * ld_d;
    const long long label = labels[i];
    const float dn = den[0];
    const float g = dn > 0.f ? dloss[0] / dn : 0.f;
    if (label < 0 || label >= NL || !(dn > 0.f)) {
#pragma unroll
        for (int c = 0; c < CE_MAXNL; ++c)
            if (c < NL) out[c] = (T)0.f;
        return;
    }
    float w[CE_MAXNL], v[CE_MAXNL], m, z;
    const float wsum = ce_weights(class_w, NL, w);
    ce_row<T>(logits + (size_t)i * ld, NL, v, m, z);
    float wy = 0.f;
#pragma unroll
    for (int c = 0; c < CE_MAXNL; ++c) wy = c == (int)label ? w[c] : wy;
    const float k1 = (1.0f - eps) * wy, k2 = eps / (float)NL;
    const float tsum = fmaf(k2, wsum, k1);
#pragma unroll
    for (int c = 0; c < CE_MAXNL; ++c) {
        if (c < NL) {
            const float t = fmaf(k2, w[c], c == (int)label ? k1 : 0.f);
            out[c] = (T)(g * (expf(v[c] - m) / z * tsum - t));
        }
    }
}

}  // namespace

extern "C" int fmmt_ce_fwd(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, const float* class_w, float smoothing,
                           float* loss, float* den, void* stream) {
    if (dtype != FMMT_BF16 && dtype != FMMT_F32) return FMMT_EINVAL;
    if (B < 1 || B > CE_MAXB || NL < 1 || NL > CE_MAXNL || ld < NL) return FMMT_EINVAL;
    if (!(smoothing >= 0.f) || !(smoothing < 1.f)) return FMMT_EINVAL;
    if (!logits || !labels || !loss || !den) return FMMT_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(ce_fwd_kernel<bf16>, dim3(1), dim3(CE_THREADS), 0, st, B, NL, (const bf16*)logits, ld, (const long long*)labels, class_w, smoothing,
                           loss, den);
    else
        hipLaunchKernelGGL(ce_fwd_kernel<float>, dim3(1), dim3(CE_THREADS), 0, st, B, NL, (const float*)logits, ld, (const long long*)labels, class_w, smoothing,
                           loss, den);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_ce_bwd(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, const float* class_w, float smoothing,
                           const float* dloss, const float* den, void* dlogits, int ld_d, void* stream) {
    if (dtype != FMMT_BF16 && dtype != FMMT_F32) return FMMT_EINVAL;
    if (B < 1 || B > CE_MAXB || NL < 1 || NL > CE_MAXNL || ld < NL || ld_d < NL) return FMMT_EINVAL;
    if (!(smoothing >= 0.f) || !(smoothing < 1.f)) return FMMT_EINVAL;
    if (!logits || !labels || !dloss || !den || !dlogits) return FMMT_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((B + CE_BWD_THREADS - 1) / CE_BWD_THREADS);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(ce_bwd_kernel<bf16>, grid, dim3(CE_BWD_THREADS), 0, st, B, NL, (const bf16*)logits, ld, (const long long*)labels, class_w, smoothing,
                           dloss, den, (bf16*)dlogits, ld_d);
    else
        hipLaunchKernelGGL(ce_bwd_kernel<float>, grid, dim3(CE_BWD_THREADS), 0, st, B, NL, (const float*)logits, ld, (const long long*)labels, class_w, smoothing,
                           dloss, den, (float*)dlogits, ld_d);
    FMMT_CHECK_LAUNCH();
    return 0;
}
