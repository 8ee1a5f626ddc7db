// The replica digest (include/fmmt_digest.h): two 64-bit integer sums over the BITS of every parameter, first moment and second moment the fused
// optimizer's descriptor table (AdamDesc, adamw_core.h) addresses -- six words a rank can compare with the other ranks' instead of copying
// gigabytes to the host.  For tensor j (descriptor order), element i, e = the element's 32 bits as an unsigned integer:
//     S1 = sum e                                  mod 2^64
//     S2 = sum e * ((i + 1) + (j + 1) * 2^32)     mod 2^64
// Integer sums are associative: the result does not depend on the order of summation, so nothing here has to fix one.
//
// digest_partial_kernel: one workgroup per 4096-element block of the table, exactly fmmt_adamw_batch's block map.  A full block whose three
//   pointers are 16-byte aligned reads 16 bytes per lane and load; the last block of a tensor and a misaligned tensor go element by element.
//   Wave reduction by shuffles, the four waves through LDS, thread 0 stores the block's six words.
// digest_finish_kernel: one workgroup sums the per-block words into out[0..5].
// Every word has one writer; launches on a stream are ordered: ordinary loads and stores, no atomics.
#include "fmmt_common.h"
#include "adamw_core.h"
#include "../../include/fmmt.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += (u64)__shfl_xor((long long)v, s, 64);
    return v;
}

__global__ __launch_bounds__(256) void digest_partial_kernel(const AdamDesc* __restrict__ desc, int n_desc, u64* __restrict__ partial) {
    __shared__ u64 red[4][6];
    int lo = 0, hi = n_desc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].blk_begin <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const AdamDesc d = desc[lo];
    const long long base = (long long)((int)blockIdx.x - d.blk_begin) * 4096;
    const u64 tensor = (u64)(lo + 1) << 32;
    const float* src[3] = {d.p, d.m, d.v};
    u64 s[6] = {0, 0, 0, 0, 0, 0};
    const bool vec = base + 4096 <= d.n && ((reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.m) |
                                               reinterpret_cast<uintptr_t>(d.v)) & 15) == 0;                    // block-uniform
    if (vec) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long o = base + (long long)(i * 256 + threadIdx.x) * 4;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const u32x4 e = *reinterpret_cast<const u32x4*>(src[k] + o);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    s[2 * k] += (u64)e[c];
                    s[2 * k + 1] += (u64)e[c] * ((u64)(o + c + 1) + tensor);
                }
            }
        }
    } else {
        for (long long o = base + threadIdx.x; o < base + 4096 && o < d.n; o += 256) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const u64 e = (u64)__float_as_uint(src[k][o]);
                s[2 * k] += e;
                s[2 * k + 1] += e * ((u64)(o + 1) + tensor);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        s[k] = wave_sum_u64(s[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) partial[(size_t)blockIdx.x * 6 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

__global__ __launch_bounds__(1024) void digest_finish_kernel(const u64* __restrict__ partial, int n_blocks, u64* __restrict__ out) {
    __shared__ u64 red[16][6];
    u64 s[6] = {0, 0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < n_blocks; b += 1024) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += partial[(size_t)b * 6 + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        s[k] = wave_sum_u64(s[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        u64 a = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) a += red[w][threadIdx.x];
        out[threadIdx.x] = a;
    }
}

}  // namespace

extern "C" int fmmt_param_digest(int n_desc, int n_blocks, const void* desc, uint64_t* partial, uint64_t* out, void* stream) {
    if (n_desc < 1 || n_blocks < 1 || !desc || !partial || !out) return FMMT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(out)) & 7) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(digest_partial_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, reinterpret_cast<const AdamDesc*>(desc), n_desc,
                       reinterpret_cast<u64*>(partial));
    FMMT_CHECK_LAUNCH();
    hipLaunchKernelGGL(digest_finish_kernel, dim3(1), dim3(1024), 0, st, reinterpret_cast<const u64*>(partial), n_blocks, reinterpret_cast<u64*>(out));
    FMMT_CHECK_LAUNCH();
    return 0;
}
