// Per-tensor statistics over the fused optimizer's descriptor table (include/fmmt_stats.h): for every record of the AdamDesc table
// (adamw_core.h) the sum of squares, the largest magnitude and the count of NaN / inf elements of ONE field -- the gradient, the parameter, the
// first or the second moment.  fmmt_param_digest's shape (digest.hip) with a reduction per record instead of one over everything: a captured step
// runs it between the clip norm and the update (train.py:135-143), so that a skipped update can name the tensor that caused it before the flat
// gradient buffers are zeroed.
//
// table_stats_partial_kernel: one workgroup per 4096-element block of the table, exactly fmmt_adamw_batch's block map (adamw_find_record) and its
//   alignment rule (adamw_batch_body): a quad of four elements is one 16-byte load (8 bytes for a bf16 gradient) where its address allows it,
//   element by element otherwise and in the last partial quad of a record (a whole block of an aligned fp32 field takes the same loads without the
//   per-quad tests, all four in flight at once).  Each lane folds its up to 16 elements in index order, the wave folds
//   by xor shuffles, the four waves through LDS as (w0 + w1) + (w2 + w3); thread 0 stores the block's triple as one 16-byte word.
// table_stats_finish_kernel: one workgroup per record folds that record's block triples the same way (lane t takes blocks t, t + 256, ...) and
//   stores stats[j].  With a norm word whose exponent bits are all set, every workgroup also copies its record into the snapshot, and workgroup 0
//   counts the bad update and looks for the first offending record by REPEATING the records' reductions in order -- the same function on the
//   same partials, hence the same bits as the workgroup that owns the record -- until one offends: no workgroup reads what another one writes.
// The largest magnitude is folded as an unsigned integer over the bits with the sign cleared: for everything that is not a NaN the order of those
// integers is the order of the magnitudes, a NaN (above 0x7f800000) is left out by one compare, and denormals pass untouched.
// Every word has one writer; every order of summation is fixed by the table alone: ordinary loads and stores, no atomics, two calls the same bits.
#include "fmmt_common.h"
#include "adamw_core.h"
#include "../../include/fmmt.h"

namespace {

struct Tri {
    float sumsq;
    unsigned max_bits;      // bits of the largest |x| that is not a NaN
    int nonfinite;
};

__device__ __forceinline__ void tri_add(Tri& t, float x) {
    const unsigned a = __float_as_uint(x) & 0x7fffffffu;
    t.sumsq += x * x;
    if (a <= 0x7f800000u && a > t.max_bits) t.max_bits = a;
    t.nonfinite += finite_bits(x) ? 0 : 1;
}

__device__ __forceinline__ Tri tri_join(const Tri a, const Tri b) {
    return Tri{a.sumsq + b.sumsq, a.max_bits > b.max_bits ? a.max_bits : b.max_bits, a.nonfinite + b.nonfinite};
}

// the fold of a 256-thread workgroup, returned to every thread; `red` is free again when it returns
__device__ __forceinline__ Tri tri_block(Tri t, Tri (&red)[4]) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        Tri o;
        o.sumsq = __shfl_xor(t.sumsq, s, 64);
        o.max_bits = (unsigned)__shfl_xor((int)t.max_bits, s, 64);
        o.nonfinite = __shfl_xor(t.nonfinite, s, 64);
        t = tri_join(t, o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    t = tri_join(tri_join(red[0], red[1]), tri_join(red[2], red[3]));
    __syncthreads();
    return t;
}

__device__ __forceinline__ u32x4 tri_word(const Tri t) { return u32x4{__float_as_uint(t.sumsq), t.max_bits, (unsigned)t.nonfinite, 0u}; }

template <int WHICH>
__device__ __forceinline__ Tri block_stats(const AdamDesc d) {
    const float* xf = WHICH == FMMT_STATS_G ? reinterpret_cast<const float*>(d.g) : WHICH == FMMT_STATS_P ? d.p : WHICH == FMMT_STATS_M ? d.m : d.v;
    const bf16* xb = reinterpret_cast<const bf16*>(d.g);
    const bool is_bf16 = WHICH == FMMT_STATS_G && d.g_bf16;                                   // block-uniform
    const long long base = (long long)((int)blockIdx.x - d.blk_begin) * 4096;
    Tri t{0.0f, 0u, 0};
    // a whole block of an aligned fp32 field (a quad's offset is a multiple of 16 bytes, so the rule below says the same of each of its quads):
    // the four loads of a lane are issued together, then folded in the order of the general path -- the same bits, more bytes in flight
    if (!is_bf16 && base + 4096 <= d.n && (reinterpret_cast<uintptr_t>(xf) & 15) == 0) {
        f32x4 x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const f32x4*>(xf + base + (long long)(i * 256 + threadIdx.x) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) tri_add(t, x[i][e]);
        }
        return t;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long o = base + (long long)(i * 256 + threadIdx.x) * 4;
        if (o >= d.n) break;
        const bool ok = is_bf16 ? (reinterpret_cast<uintptr_t>(xb + o) & 7) == 0 : (reinterpret_cast<uintptr_t>(xf + o) & 15) == 0;
        if (o + 4 <= d.n && ok) {
            f32x4 x;
            if (is_bf16) {
                const bf16x4 q = *reinterpret_cast<const bf16x4*>(xb + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = (float)q[e];
            } else {
                x = *reinterpret_cast<const f32x4*>(xf + o);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) tri_add(t, x[e]);
        } else {
            for (long long j = o; j < d.n && j < o + 4; ++j) tri_add(t, is_bf16 ? (float)xb[j] : xf[j]);
        }
    }
    return t;
}

template <int WHICH>
__global__ __launch_bounds__(256) void table_stats_partial_kernel(const AdamDesc* __restrict__ desc, int n_desc, u32x4* __restrict__ partial) {
    __shared__ Tri red[4];
    const int r = adamw_find_record(desc, n_desc);
    const Tri t = tri_block(block_stats<WHICH>(desc[r]), red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tri_word(t);
}

// record j's blocks are [desc[j].blk_begin, the next record's blk_begin or n_blocks)
__device__ __forceinline__ Tri record_stats(const AdamDesc* __restrict__ desc, int n_desc, int n_blocks, const u32x4* __restrict__ partial, int j,
                                            Tri (&red)[4]) {
    const int b0 = desc[j].blk_begin, b1 = j + 1 < n_desc ? desc[j + 1].blk_begin : n_blocks;
    Tri t{0.0f, 0u, 0};
    for (int b = b0 + (int)threadIdx.x; b < b1; b += 256) {
        const u32x4 w = partial[b];
        t = tri_join(t, Tri{__uint_as_float(w[0]), w[1], (int)w[2]});
    }
    return tri_block(t, red);
}

__global__ __launch_bounds__(256) void table_stats_finish_kernel(const AdamDesc* __restrict__ desc, int n_desc, int n_blocks,
                                                                 const u32x4* __restrict__ partial, u32x4* __restrict__ stats,
                                                                 const float* __restrict__ norm_p, u32x4* __restrict__ bad_stats,
                                                                 long long* __restrict__ bad_words) {
    __shared__ Tri red[4];
    const int j = (int)blockIdx.x;
    const Tri t = record_stats(desc, n_desc, n_blocks, partial, j, red);
    if (threadIdx.x == 0) stats[j] = tri_word(t);
    if (!norm_p || finite_bits(*norm_p)) return;             // grid-uniform: the common case ends here
    if (threadIdx.x == 0 && bad_stats) bad_stats[j] = tri_word(t);
    if (j != 0 || !bad_words) return;
    int first = -1;
    for (int k = 0; k < n_desc; ++k) {                       // every thread holds the same triple: the exit is block-uniform
        const Tri s = k == 0 ? t : record_stats(desc, n_desc, n_blocks, partial, k, red);
        if (s.nonfinite > 0 || !finite_bits(s.sumsq)) {
            first = k;
            break;
        }
    }
    if (threadIdx.x == 0) {
        bad_words[0] += 1;
        bad_words[1] = first;
    }
}

}  // namespace

extern "C" int fmmt_table_stats(int which, int n_desc, int n_blocks, const void* desc, void* partial, void* stats, const float* norm,
                                void* bad_stats, int64_t* bad_words, void* stream) {
    if (n_desc < 1 || n_blocks < 1 || which < FMMT_STATS_G || which > FMMT_STATS_V || !desc || !partial || !stats) return FMMT_EINVAL;
    if (!norm && (bad_stats || bad_words)) return FMMT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(bad_stats)) & 15) return FMMT_EALIGN;
    if (reinterpret_cast<uintptr_t>(bad_words) & 7) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const AdamDesc* d = reinterpret_cast<const AdamDesc*>(desc);
    u32x4* part = reinterpret_cast<u32x4*>(partial);
    const dim3 grid((unsigned)n_blocks), block(256);
    switch (which) {
        case FMMT_STATS_G: hipLaunchKernelGGL(table_stats_partial_kernel<FMMT_STATS_G>, grid, block, 0, st, d, n_desc, part); break;
        case FMMT_STATS_P: hipLaunchKernelGGL(table_stats_partial_kernel<FMMT_STATS_P>, grid, block, 0, st, d, n_desc, part); break;
        case FMMT_STATS_M: hipLaunchKernelGGL(table_stats_partial_kernel<FMMT_STATS_M>, grid, block, 0, st, d, n_desc, part); break;
        default: hipLaunchKernelGGL(table_stats_partial_kernel<FMMT_STATS_V>, grid, block, 0, st, d, n_desc, part); break;
    }
    FMMT_CHECK_LAUNCH();
    hipLaunchKernelGGL(table_stats_finish_kernel, dim3((unsigned)n_desc), block, 0, st, d, n_desc, n_blocks, part, reinterpret_cast<u32x4*>(stats), norm,
                       reinterpret_cast<u32x4*>(bad_stats), reinterpret_cast<long long*>(bad_words));
    FMMT_CHECK_LAUNCH();
    return 0;
}
