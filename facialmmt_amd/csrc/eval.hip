// The two pieces of device work only EVALUATION has (train.py:154-243, utils/eval_metrics.py:16-28), one launch each.
//
// fmmt_emotion_head_fwd: the target-task head of SwinForAffwildClassification at inference (src/models.py:28-32) with the importance score of
//   train.py:186-188:  feats [N][K] -> Linear(K,64) + bias -> ReLU -> Linear(64,NL) + bias -> (+ gumbel) / tau -> softmax -> preds, sum_c preds^2.
//   The work is 2 * N * K * 64 FLOP (21 MFLOP at N = 640, K = 512): the kernel is about latency.  Layout:
//     * a workgroup owns 16 rows (N = 640: 40 workgroups) and has 8 waves: wave w forms the 16 x 16 tile of hidden units [16 (w & 3), +16) over the
//       K half (w >> 2) with exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), so the K loop is K / 32 steps long instead of K / 16;
//     * W1 (64 x K fp32, 128 KB at K = 512) is NOT staged in LDS: it is read once per workgroup straight into the MFMA B operand, 16 bytes per lane
//       -- 40 workgroups re-read the same 128 KB, which the 4 MB L2 serves -- and the weights stay the module's fp32 parameters, no shadow copy;
//     * the lane's four consecutive k of a 16-byte load feed four successive MFMAs (A and B use the same k permutation, so the sum is the same);
//     * the two K halves meet in LDS (8 KB), then 8 lanes per row finish the row: bias + ReLU + the 64 x NL product, the NL-way softmax and the
//       squared sum through three xor shuffles.
// fmmt_eval_accumulate: per-row fp32 log-sum-exp cross entropy and argmax, added into accumulators that stay on the device for the whole split
//   (loss sum as a double, row count and the NL x NL confusion matrix as int64).  ONE workgroup; the row losses are summed by a fixed 1024-leaf tree
//   in LDS, whatever B is, so the sum is deterministic; the counts go through integer LDS atomics (order-free) and leave with ordinary stores.
// fmmt_eval_accumulate_at (include/fmmt_eval_collect.h): the same update, the rows of the batch also kept -- logits, label, argmax -- at a row index
//   read from a device word that the kernel then advances, so that a captured graph collects a whole split; same body, same accumulator bits.
// fmmt_eval_accumulate_rows (include/fmmt_eval_shard.h): that update with the number of rows that exist in a second device word -- a short batch
//   padded to the captured B stores and counts its real rows only and advances the cursor by them; the same body once more.
#include "fmmt_common.h"
#include "../../include/fmmt.h"

namespace {

constexpr int EH_ROWS = 16, EH_HID = 64, EH_THREADS = 512, EH_MAXNL = 8;
constexpr int EA_THREADS = 1024;

template <typename T> __device__ __forceinline__ f32x4 eh_load4(const T* p);
template <> __device__ __forceinline__ f32x4 eh_load4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <> __device__ __forceinline__ f32x4 eh_load4<bf16>(const bf16* p) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    f32x4 r = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    return r;
}

template <typename T>
__global__ __launch_bounds__(EH_THREADS) void emotion_head_kernel(int N, int K, int NL, const T* __restrict__ feats, int ld, const float* __restrict__ w1,
                                                                  const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                                  const float* __restrict__ gumbel, float tau, float* __restrict__ preds,
                                                                  float* __restrict__ importance) {
    __shared__ float hpart[2][EH_ROWS][EH_HID + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = wave & 3, kh = wave >> 2;
    const int li = lane & 15, lg = lane >> 4;
    const int row0 = blockIdx.x * EH_ROWS;
    const int row = min(row0 + li, N - 1);                   // rows behind the end re-read the last row; their stores are masked below
    const T* a_ptr = feats + (size_t)row * ld + lg * 4;
    const float* b_ptr = w1 + (size_t)(tile * 16 + li) * K + lg * 4;
    const int kbeg = kh * (K >> 1), kend = kbeg + (K >> 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = kbeg; k < kend; k += 32) {                  // K % 64 == 0: a K half is whole 32-deep steps; both loads of a step are in flight together
        const f32x4 a0 = eh_load4<T>(a_ptr + k), a1 = eh_load4<T>(a_ptr + k + 16);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(b_ptr + k), b1v = *reinterpret_cast<const f32x4*>(b_ptr + k + 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b0[e], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b1v[e], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) hpart[kh][lg * 4 + r][tile * 16 + li] = acc[r];      // D[i = lg * 4 + r][j = li]
    __syncthreads();
    if (tid < EH_ROWS * EH_MAXNL) {                          // two whole waves: the shuffles below run with every lane active
        const int r = tid >> 3, c = tid & 7, grow = row0 + r;
        const bool live = c < NL;
        float s = -INFINITY;
        if (live) {
            s = 0.f;                                        // the bias is added to the finished sum: 64 roundings at a +-1e4 bias's magnitude would cost 1e-3 of a probability
            const float* wc = w2 + c * EH_HID;
            for (int j = 0; j < EH_HID; ++j) {
                const float pre = hpart[0][r][j] + hpart[1][r][j] + b1[j];
                const float h = pre < 0.f ? 0.f : pre;               // torch.relu: a NaN feature stays NaN (fmaxf would return the 0)
                s = fmaf(h, wc[j], s);
            }
            s += b2[c];
            if (gumbel != nullptr && grow < N) s += gumbel[(size_t)grow * NL + c];
            s = s / tau;
        }
        float m = s;
        m = fmaxf(m, __shfl_xor(m, 1));
        m = fmaxf(m, __shfl_xor(m, 2));
        m = fmaxf(m, __shfl_xor(m, 4));
        const float e = live ? expf(s - m) : 0.f;
        float z = e;
        z += __shfl_xor(z, 1);
        z += __shfl_xor(z, 2);
        z += __shfl_xor(z, 4);
        const float p = e / z;
        float q = p * p;
        q += __shfl_xor(q, 1);
        q += __shfl_xor(q, 2);
        q += __shfl_xor(q, 4);
        if (grow < N) {
            if (live) preds[(size_t)grow * NL + c] = p;
            if (c == 0 && importance != nullptr) importance[grow] = q;
        }
    }
}

// The body both metric-update kernels share -- ONE statement of the row loss, the argmax, the 1024-leaf loss tree and the LDS confusion counts, so
// the two entry points leave the same bits in the accumulators.  Row `tid` of the batch is kept at row `base + tid` of logits_out / labels_out /
// pred_out when that row exists (0 <= base + tid < cap; each pointer may be NULL); `pred` is indexed by the batch row.  Every thread of the
// workgroup passes the barriers below, whatever B is.
template <typename T>
__device__ __forceinline__ void eval_accumulate_body(int B, int NL, const T* __restrict__ logits, int ld, const long long* __restrict__ labels,
                                                     double* __restrict__ loss_sum, long long* __restrict__ count, long long* __restrict__ confusion,
                                                     int* __restrict__ pred, float* __restrict__ logits_out, long long* __restrict__ labels_out,
                                                     int* __restrict__ pred_out, long long base, long long cap) {
    __shared__ double red[EA_THREADS];
    __shared__ int conf[EH_MAXNL * EH_MAXNL];
    __shared__ int cnt;
    const int tid = threadIdx.x;
    if (tid < EH_MAXNL * EH_MAXNL) conf[tid] = 0;
    if (tid == 0) cnt = 0;
    __syncthreads();
    double loss = 0.0;
    if (tid < B) {
        float v[EH_MAXNL];
        float m = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int c = 0; c < EH_MAXNL; ++c) {
            v[c] = c < NL ? (float)logits[(size_t)tid * ld + c] : -INFINITY;
            if (v[c] > m) { m = v[c]; arg = c; }             // strict: the first maximum wins (numpy.argmax)
        }
        float z = 0.f;
#pragma unroll
        for (int c = 0; c < EH_MAXNL; ++c) z += c < NL ? expf(v[c] - m) : 0.f;
        const float lse = m + logf(z);
        const long long label = labels[tid];
        if (pred != nullptr) pred[tid] = arg;
        const long long dst = base + tid;
        if (dst >= 0 && dst < cap) {                         // a row behind the capacity is counted below and kept nowhere
            if (logits_out != nullptr) {
                float* o = logits_out + (size_t)dst * NL;
#pragma unroll
                for (int c = 0; c < EH_MAXNL; ++c)
                    if (c < NL) o[c] = v[c];
            }
            if (labels_out != nullptr) labels_out[dst] = label;
            if (pred_out != nullptr) pred_out[dst] = arg;
        }
        if (label >= 0 && label < NL) {                      // negative: ignored (torch's ignore_index, padded rows); >= NL can address nothing here
            float vl = 0.f;
#pragma unroll
            for (int c = 0; c < EH_MAXNL; ++c) vl = c == (int)label ? v[c] : vl;
            loss = (double)(lse - vl);
            atomicAdd(&conf[(int)label * NL + arg], 1);
            atomicAdd(&cnt, 1);
        }
    }
    red[tid] = loss;
    __syncthreads();
    for (int s = EA_THREADS / 2; s > 0; s >>= 1) {          // the same 1024-leaf tree for every B: a fixed summation order
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid < NL * NL) confusion[tid] += conf[tid];          // one workgroup, launches ordered by the stream: plain read-modify-write
    if (tid == 0) {
        *loss_sum += red[0];
        *count += cnt;
    }
}

template <typename T>
__global__ __launch_bounds__(EA_THREADS) void eval_accumulate_kernel(int B, int NL, const T* __restrict__ logits, int ld, const long long* __restrict__ labels,
                                                                     double* __restrict__ loss_sum, long long* __restrict__ count,
                                                                     long long* __restrict__ confusion, int* __restrict__ pred,
                                                                     float* __restrict__ logits_out, long long out_offset) {
    // the host has checked out_offset + B <= capacity: every row has a place
    eval_accumulate_body<T>(B, NL, logits, ld, labels, loss_sum, count, confusion, pred, logits_out, nullptr, nullptr, out_offset, out_offset + B);
}

// The same update with the destination row held in a DEVICE word: a captured graph freezes its launch arguments, a word in memory it re-reads on
// every replay.  All 1024 threads read *cursor, then a barrier, and only behind the whole body thread 0 advances it: without the barrier a late
// wave of a B = 1024 batch could read the advanced value and keep its rows B too far.
template <typename T>
__global__ __launch_bounds__(EA_THREADS) void eval_accumulate_at_kernel(int B, int NL, const T* __restrict__ logits, int ld, const long long* __restrict__ labels,
                                                                        double* __restrict__ loss_sum, long long* __restrict__ count,
                                                                        long long* __restrict__ confusion, long long* cursor,
                                                                        float* __restrict__ logits_out, long long* __restrict__ labels_out,
                                                                        int* __restrict__ pred_out, long long out_capacity) {
    const long long base = *cursor;
    __syncthreads();                                         // every thread holds the old cursor before anything below may write the new one
    eval_accumulate_body<T>(B, NL, logits, ld, labels, loss_sum, count, confusion, nullptr, logits_out, labels_out, pred_out, base, out_capacity);
    if (threadIdx.x == 0) *cursor = base + B;                // also when rows were dropped: cursor > out_capacity reports the overflow
}

// The collecting update with the batch's REAL row count in a device word as well: a short batch padded to the captured B.  The body is instantiated
// with b = clamp(*n_rows, 0, B) in the place of B, so a row at or behind b is not read, stored or counted whatever its label says, and b == B is
// eval_accumulate_at_kernel instruction for instruction behind the two loads.  Both words are read by every thread in front of the barrier.
template <typename T>
__global__ __launch_bounds__(EA_THREADS) void eval_accumulate_rows_kernel(int B, int NL, const T* __restrict__ logits, int ld, const long long* __restrict__ labels,
                                                                          double* __restrict__ loss_sum, long long* __restrict__ count,
                                                                          long long* __restrict__ confusion, long long* cursor, const int* __restrict__ n_rows,
                                                                          float* __restrict__ logits_out, long long* __restrict__ labels_out,
                                                                          int* __restrict__ pred_out, long long out_capacity) {
    const long long base = *cursor;
    const int b = min(max(*n_rows, 0), B);
    __syncthreads();                                         // every thread holds the old cursor before anything below may write the new one
    eval_accumulate_body<T>(b, NL, logits, ld, labels, loss_sum, count, confusion, nullptr, logits_out, labels_out, pred_out, base, out_capacity);
    if (threadIdx.x == 0) *cursor = base + b;
}

}  // namespace

extern "C" int fmmt_emotion_head_fwd(int dtype, int N, int K, int H, int NL, const void* feats, int ld, const float* w1, const float* b1, const float* w2,
                                     const float* b2, const float* gumbel, float tau, float* preds, float* importance, void* stream) {
    if (dtype != FMMT_BF16 && dtype != FMMT_F32) return FMMT_EINVAL;
    if (N <= 0 || K <= 0 || K % 64 || H != EH_HID || NL <= 0 || NL > EH_MAXNL || ld < K || !(tau > 0.f)) return FMMT_EINVAL;
    if (!feats || !w1 || !b1 || !w2 || !b2 || !preds) return FMMT_EINVAL;
    if (((uintptr_t)feats | (uintptr_t)w1) & 15 || ld % 4) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((N + EH_ROWS - 1) / EH_ROWS);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(emotion_head_kernel<bf16>, grid, dim3(EH_THREADS), 0, st, N, K, NL, (const bf16*)feats, ld, w1, b1, w2, b2, gumbel, tau, preds, importance);
    else
        hipLaunchKernelGGL(emotion_head_kernel<float>, grid, dim3(EH_THREADS), 0, st, N, K, NL, (const float*)feats, ld, w1, b1, w2, b2, gumbel, tau, preds, importance);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_eval_accumulate(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, double* loss_sum, int64_t* count,
                                    int64_t* confusion, int32_t* pred, float* logits_out, int64_t out_offset, int64_t out_capacity, void* stream) {
    if (dtype != FMMT_BF16 && dtype != FMMT_F32) return FMMT_EINVAL;
    if (B <= 0 || B > EA_THREADS || NL <= 0 || NL > EH_MAXNL || ld < NL) return FMMT_EINVAL;
    if (!logits || !labels || !loss_sum || !count || !confusion) return FMMT_EINVAL;
    if (logits_out && (out_offset < 0 || out_capacity < 0 || out_offset > out_capacity - B)) return FMMT_EINVAL;
    if (((uintptr_t)loss_sum | (uintptr_t)count | (uintptr_t)confusion | (uintptr_t)labels) & 7) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(eval_accumulate_kernel<bf16>, dim3(1), dim3(EA_THREADS), 0, st, B, NL, (const bf16*)logits, ld, (const long long*)labels, loss_sum,
                           (long long*)count, (long long*)confusion, pred, logits_out, (long long)out_offset);
    else
        hipLaunchKernelGGL(eval_accumulate_kernel<float>, dim3(1), dim3(EA_THREADS), 0, st, B, NL, (const float*)logits, ld, (const long long*)labels, loss_sum,
                           (long long*)count, (long long*)confusion, pred, logits_out, (long long)out_offset);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_eval_accumulate_at(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, double* loss_sum, int64_t* count,
                                       int64_t* confusion, int64_t* cursor, float* logits_out, int64_t* labels_out, int32_t* pred_out,
                                       int64_t out_capacity, void* stream) {
    if (dtype != FMMT_BF16 && dtype != FMMT_F32) return FMMT_EINVAL;
    if (B <= 0 || B > EA_THREADS || NL <= 0 || NL > EH_MAXNL || ld < NL || out_capacity < 0) return FMMT_EINVAL;
    if (!logits || !labels || !loss_sum || !count || !confusion || !cursor || !logits_out || !labels_out) return FMMT_EINVAL;
    if (((uintptr_t)loss_sum | (uintptr_t)count | (uintptr_t)confusion | (uintptr_t)labels | (uintptr_t)cursor | (uintptr_t)labels_out) & 7) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(eval_accumulate_at_kernel<bf16>, dim3(1), dim3(EA_THREADS), 0, st, B, NL, (const bf16*)logits, ld, (const long long*)labels, loss_sum,
                           (long long*)count, (long long*)confusion, (long long*)cursor, logits_out, (long long*)labels_out, pred_out, (long long)out_capacity);
    else
        hipLaunchKernelGGL(eval_accumulate_at_kernel<float>, dim3(1), dim3(EA_THREADS), 0, st, B, NL, (const float*)logits, ld, (const long long*)labels, loss_sum,
                           (long long*)count, (long long*)confusion, (long long*)cursor, logits_out, (long long*)labels_out, pred_out, (long long)out_capacity);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_eval_accumulate_rows(int dtype, int B, int NL, const void* logits, int ld, const int64_t* labels, double* loss_sum, int64_t* count,
                                         int64_t* confusion, int64_t* cursor, const int32_t* n_rows, float* logits_out, int64_t* labels_out,
                                         int32_t* pred_out, int64_t out_capacity, void* stream) {
    if (dtype != FMMT_BF16 && dtype != FMMT_F32) return FMMT_EINVAL;
    if (B <= 0 || B > EA_THREADS || NL <= 0 || NL > EH_MAXNL || ld < NL || out_capacity < 0) return FMMT_EINVAL;
    if (!logits || !labels || !loss_sum || !count || !confusion || !cursor || !n_rows || !logits_out || !labels_out) return FMMT_EINVAL;
    if (((uintptr_t)loss_sum | (uintptr_t)count | (uintptr_t)confusion | (uintptr_t)labels | (uintptr_t)cursor | (uintptr_t)labels_out) & 7) return FMMT_EALIGN;
    if ((uintptr_t)n_rows & 3) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(eval_accumulate_rows_kernel<bf16>, dim3(1), dim3(EA_THREADS), 0, st, B, NL, (const bf16*)logits, ld, (const long long*)labels, loss_sum,
                           (long long*)count, (long long*)confusion, (long long*)cursor, (const int*)n_rows, logits_out, (long long*)labels_out, pred_out,
                           (long long)out_capacity);
    else
        hipLaunchKernelGGL(eval_accumulate_rows_kernel<float>, dim3(1), dim3(EA_THREADS), 0, st, B, NL, (const float*)logits, ld, (const long long*)labels, loss_sum,
                           (long long*)count, (long long*)confusion, (long long*)cursor, (const int*)n_rows, logits_out, (long long*)labels_out, pred_out,
                           (long long)out_capacity);
    FMMT_CHECK_LAUNCH();
    return 0;
}
