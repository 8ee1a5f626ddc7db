// Ragged MELD batches behind ONE captured shape (include/fmmt_ragged.h, DESIGN.md "Ragged frame counts").
//
// The loader hands a target-task step (B, Lv, ...) zero-padded face frames and the real count per utterance (utils/dataset.py:275-292); the
// reference concatenates the real ones on the host (train.py:60-71), so the frame tensor's first dimension changes with every batch.  Here the
// batch is packed ON THE DEVICE into a buffer of a fixed capacity -- real frames in the reference's concatenation order at the front, zeros
// behind -- and a device word n_valid says how many rows are real.  Swin runs on all rows; the one op of it that is not per row, the embedding
// head's BatchNorm1d in training mode, takes its statistics and its column sums over the first n_valid rows only (bn1d_core.h, MASKED) and hands
// padded rows a zero gradient, which is what keeps padding out of every weight gradient above it.
#include "fmmt_common.h"
#include "bn1d_core.h"
#include "../../include/fmmt.h"

namespace {

constexpr int PK_THREADS = 256, PK_VECS = 8;                  // a workgroup moves 256 x 8 x 16 bytes = 32 KB of one destination row
constexpr int PK_MAX_B = 256;

// grid = (chunks of a row, F_cap rows).  Every workgroup rebuilds the utterance boundaries -- the inclusive prefix sum of clamp(num_imgs, 0, Lv),
// at most 256 words -- in LDS and looks up which (utterance, frame) its destination row comes from; rows at or behind the total are zero-filled.
__global__ __launch_bounds__(PK_THREADS) void pack_frames_kernel(int B, int Lv, int F_cap, unsigned vecs_per_row, const u32x4* __restrict__ src,
                                                                 const long long* __restrict__ num_imgs, u32x4* __restrict__ dst,
                                                                 int* __restrict__ counts) {
    __shared__ int cum[PK_MAX_B];                             // inclusive prefix sum of the clamped counts
    __shared__ int src_row;                                   // u * Lv + k of this destination row, -1: padding
    const int tid = threadIdx.x, r = blockIdx.y;
    if (tid < B) {
        const long long n = num_imgs[tid];
        cum[tid] = (int)(n < 0 ? 0 : (n > Lv ? Lv : n));
    }
    __syncthreads();
    if (tid == 0) {                                           // <= 256 words: a serial scan is a few hundred cycles
        int a = 0, row = -1;
        for (int u = 0; u < B; ++u) {
            const int n = cum[u];
            if (row < 0 && r < a + n) row = u * Lv + (r - a);
            a += n;
            cum[u] = a;
        }
        src_row = row;
        if (blockIdx.x == 0 && r == 0) {
            counts[0] = a < F_cap ? a : F_cap;
            counts[1] = a;
        }
    }
    __syncthreads();
    const int row = src_row;
    const unsigned v0 = blockIdx.x * (PK_THREADS * PK_VECS) + tid;
    u32x4* d = dst + (size_t)r * vecs_per_row;
    u32x4 t[PK_VECS];
#pragma unroll
    for (int j = 0; j < PK_VECS; ++j) t[j] = u32x4{0u, 0u, 0u, 0u};
    if (row >= 0) {                                           // all of a thread's loads in flight before its first store
        const u32x4* s = src + (size_t)row * vecs_per_row;
#pragma unroll
        for (int j = 0; j < PK_VECS; ++j) {
            const unsigned v = v0 + j * PK_THREADS;
            if (v < vecs_per_row) t[j] = s[v];
        }
    }
#pragma unroll
    for (int j = 0; j < PK_VECS; ++j) {
        const unsigned v = v0 + j * PK_THREADS;
        if (v < vecs_per_row) d[v] = t[j];
    }
}

// The inverse (include/fmmt_tokens.h): grid = (B * L destination rows, chunks of a row).  Destination row (u, k) takes source row cum_{u-1} + k when
// k < n_u and that row lies below `cap`, zeros otherwise; the workgroup sums the counts in front of its utterance itself (<= 256 words).
__global__ __launch_bounds__(PK_THREADS) void unpack_rows_kernel(int B, int L, int cap, unsigned vecs_per_row, const u32x4* __restrict__ src,
                                                                 const long long* __restrict__ counts, u32x4* __restrict__ dst) {
    __shared__ int cnt[PK_MAX_B];
    __shared__ int src_row;
    const int tid = threadIdx.x, r = blockIdx.x, u = r / L, k = r - u * L;
    if (tid < B) {
        const long long n = counts[tid];
        cnt[tid] = (int)(n < 0 ? 0 : (n > L ? L : n));
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0;
        for (int i = 0; i < u; ++i) a += cnt[i];
        src_row = (k < cnt[u] && a + k < cap) ? a + k : -1;
    }
    __syncthreads();
    const int row = src_row;
    const unsigned v0 = blockIdx.y * (PK_THREADS * PK_VECS) + tid;
    u32x4* d = dst + (size_t)r * vecs_per_row;
    u32x4 t[PK_VECS];
#pragma unroll
    for (int j = 0; j < PK_VECS; ++j) t[j] = u32x4{0u, 0u, 0u, 0u};
    if (row >= 0) {
        const u32x4* s = src + (size_t)row * vecs_per_row;
#pragma unroll
        for (int j = 0; j < PK_VECS; ++j) {
            const unsigned v = v0 + j * PK_THREADS;
            if (v < vecs_per_row) t[j] = s[v];
        }
    }
#pragma unroll
    for (int j = 0; j < PK_VECS; ++j) {
        const unsigned v = v0 + j * PK_THREADS;
        if (v < vecs_per_row) d[v] = t[j];
    }
}

// fmmt_token_layout (include/fmmt_tokens.h): one workgroup.  A wave per mask row finds the row's first zero (the length of its prefix of real tokens) and
// counts its non-zeros; thread 0 scans the <= 256 lengths, cutting them to the capacity; all threads then write the row map.
__global__ __launch_bounds__(256) void token_layout_kernel(int B, int T, int cap, const int* __restrict__ mask, int* __restrict__ seq_len, int* __restrict__ seq_off,
                                                          long long* __restrict__ len64, int* __restrict__ row_map, int* __restrict__ counts) {
    __shared__ int len[PK_MAX_B], off[PK_MAX_B + 1], nz[PK_MAX_B];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = wave; b < B; b += 4) {
        int first = T, n = 0;
        for (int t = lane; t < T; t += 64) {
            const bool real = mask[(size_t)b * T + t] != 0;
            n += real ? 1 : 0;
            if (!real && t < first) first = t;
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            first = min(first, __shfl_xor(first, s, 64));
            n += __shfl_xor(n, s, 64);
        }
        if (lane == 0) { len[b] = first; nz[b] = n; }
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0, all = 0;
        for (int b = 0; b < B; ++b) {
            const int n = min(len[b], cap - a);
            all += nz[b];
            off[b] = a;
            len[b] = n;
            a += n;
        }
        off[B] = a;
        counts[0] = a;
        counts[1] = all;
    }
    __syncthreads();
    if (tid < B) {
        seq_len[tid] = len[tid];
        seq_off[tid] = off[tid];
        len64[tid] = len[tid];
    }
    const int total = off[B];
    for (int r = tid; r < cap; r += 256) {
        int v = B * T + r;
        if (r < total) {
            int b = 0;
            while (b + 1 < B && off[b + 1] <= r) ++b;
            v = b * T + (r - off[b]);
        }
        row_map[r] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(BN_COLS * BN_GROUPS) void bn1d_fwd_n_kernel(int n_cap, int C, const int* __restrict__ n_valid, const T* __restrict__ x,
                                const float* __restrict__ gamma, const float* __restrict__ beta, float* running_mean, float* running_var,
                                float momentum, float eps, int training, T* __restrict__ y, float* save_mean, float* save_invstd) {
    const int n = bn_rows(n_valid, n_cap);
    bn1d_fwd_body<T, true>(n, n_cap, C, x, gamma, beta, running_mean, running_var, momentum, eps, training, y, save_mean, save_invstd);
}

template <typename T>
__global__ __launch_bounds__(BN_COLS * BN_GROUPS) void bn1d_bwd_n_kernel(int n_cap, int C, const int* __restrict__ n_valid, const T* __restrict__ dy,
                                const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ save_mean,
                                const float* __restrict__ save_invstd, int training, T* __restrict__ dx, float* dgamma, float* dbeta) {
    const int n = bn_rows(n_valid, n_cap);
    bn1d_bwd_body<T, true>(n, n_cap, C, dy, x, gamma, save_mean, save_invstd, training, dx, dgamma, dbeta);
}

}  // namespace

extern "C" int fmmt_pack_frames(int B, int Lv, int F_cap, size_t row_bytes, const void* src, const int64_t* num_imgs, void* dst, int32_t* counts,
                                void* stream) {
    if (B <= 0 || B > PK_MAX_B || Lv <= 0 || F_cap <= 0 || F_cap > 65535 || row_bytes == 0 || (long long)B * Lv > 0x7fffffffLL) return FMMT_EINVAL;
    if (!src || !num_imgs || !dst || !counts) return FMMT_EINVAL;
    if (row_bytes % 16 || ((uintptr_t)src | (uintptr_t)dst) % 16) return FMMT_EALIGN;
    const size_t vecs = row_bytes / 16;
    if (vecs > 0x7fffffffu) return FMMT_EINVAL;
    const unsigned per = PK_THREADS * PK_VECS;
    dim3 grid((unsigned)((vecs + per - 1) / per), (unsigned)F_cap);
    hipLaunchKernelGGL(pack_frames_kernel, grid, dim3(PK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), B, Lv, F_cap, (unsigned)vecs,
                       (const u32x4*)src, (const long long*)num_imgs, (u32x4*)dst, counts);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_unpack_rows(int B, int L, int cap, size_t row_bytes, const void* src, const int64_t* counts, void* dst, void* stream) {
    if (B <= 0 || B > PK_MAX_B || L <= 0 || cap <= 0 || row_bytes == 0 || (long long)B * L > 0x7fffffffLL) return FMMT_EINVAL;
    if (!src || !counts || !dst) return FMMT_EINVAL;
    if (row_bytes % 16 || ((uintptr_t)src | (uintptr_t)dst) % 16) return FMMT_EALIGN;
    const size_t vecs = row_bytes / 16;
    if (vecs > 0x7fffffffu) return FMMT_EINVAL;
    const unsigned per = PK_THREADS * PK_VECS;
    const size_t chunks = (vecs + per - 1) / per;
    if (chunks > 65535) return FMMT_EINVAL;
    dim3 grid((unsigned)(B * L), (unsigned)chunks);          // destination rows along x: B * L may pass the 65535 of a grid's y
    hipLaunchKernelGGL(unpack_rows_kernel, grid, dim3(PK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), B, L, cap, (unsigned)vecs, (const u32x4*)src,
                       (const long long*)counts, (u32x4*)dst);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_token_layout(int B, int T, int cap, const int32_t* mask, int32_t* seq_len, int32_t* seq_off, int64_t* len64, int32_t* row_map,
                                 int32_t* counts, void* stream) {
    if (B <= 0 || B > PK_MAX_B || T <= 0 || T > 65535 || cap <= 0 || cap > 65535) return FMMT_EINVAL;
    if (!mask || !seq_len || !seq_off || !len64 || !row_map || !counts) return FMMT_EINVAL;
    hipLaunchKernelGGL(token_layout_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), B, T, cap, (const int*)mask, (int*)seq_len, (int*)seq_off,
                       (long long*)len64, (int*)row_map, (int*)counts);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_batchnorm1d_fwd_n(int dtype, int n_cap, int C, const int32_t* n_valid, const void* x, const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, float momentum, float eps, int training, void* y,
                                      float* save_mean, float* save_invstd, void* stream) {
    if ((dtype != FMMT_BF16 && dtype != FMMT_F32) || n_cap <= 0 || C <= 0 || !n_valid) return FMMT_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((C + BN_COLS - 1) / BN_COLS);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(bn1d_fwd_n_kernel<bf16>, grid, dim3(BN_COLS * BN_GROUPS), 0, st, n_cap, C, n_valid, (const bf16*)x, gamma, beta,
                           running_mean, running_var, momentum, eps, training, (bf16*)y, save_mean, save_invstd);
    else
        hipLaunchKernelGGL(bn1d_fwd_n_kernel<float>, grid, dim3(BN_COLS * BN_GROUPS), 0, st, n_cap, C, n_valid, (const float*)x, gamma, beta,
                           running_mean, running_var, momentum, eps, training, (float*)y, save_mean, save_invstd);
    FMMT_CHECK_LAUNCH();
    return 0;
}

extern "C" int fmmt_batchnorm1d_bwd_n(int dtype, int n_cap, int C, const int32_t* n_valid, const void* dy, const void* x, const float* gamma,
                                      const float* save_mean, const float* save_invstd, int training, void* dx, float* dgamma, float* dbeta,
                                      void* stream) {
    if ((dtype != FMMT_BF16 && dtype != FMMT_F32) || n_cap <= 0 || C <= 0 || !n_valid) return FMMT_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((C + BN_COLS - 1) / BN_COLS);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(bn1d_bwd_n_kernel<bf16>, grid, dim3(BN_COLS * BN_GROUPS), 0, st, n_cap, C, n_valid, (const bf16*)dy, (const bf16*)x, gamma,
                           save_mean, save_invstd, training, (bf16*)dx, dgamma, dbeta);
    else
        hipLaunchKernelGGL(bn1d_bwd_n_kernel<float>, grid, dim3(BN_COLS * BN_GROUPS), 0, st, n_cap, C, n_valid, (const float*)dy, (const float*)x, gamma,
                           save_mean, save_invstd, training, (float*)dx, dgamma, dbeta);
    FMMT_CHECK_LAUNCH();
    return 0;
}
