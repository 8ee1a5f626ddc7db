// The merge of an evaluation split that W ranks evaluated in contiguous shards (include/fmmt_eval_shard.h): the gathered per-rank accumulators
// (loss sum as a double, row count, confusion matrix, cursor) and per-rank row buffers of different fill levels become one dense split in rank order,
// which blocked sharding makes dataset order.  ONE launch:
//   * every workgroup reads the W gathered cursors (W <= 64: one wave's worth), clamps them to n_r in [0, cap] and thread 0 forms the exclusive prefix
//     start_r in LDS -- recomputed per workgroup, so that no workgroup waits for another and nothing is atomic;
//   * a grid-stride loop over the W * cap * NL elements of the gathered `results`: element (r, i, c) with i < n_r goes to row start_r + i of the
//     output when that row exists; the thread of column 0 moves the row's label.  Reads and writes are contiguous within a rank's rows; nothing at or
//     behind row n_r of a rank is read and no output row at or behind the total is written;
//   * workgroup 0 writes words_out: thread 0 adds the ranks' loss sums in rank order (the bits are fixed), threads 1 .. NL * NL + 1 the integer
//     words, thread NL * NL + 2 the cursor.  A rank whose cursor is <= 0 is left out of every sum.
// Every word has one writer; ordinary loads and stores.
#include "fmmt_common.h"
#include "../../include/fmmt.h"

namespace {

constexpr int EM_THREADS = 256, EM_MAXW = 64, EM_MAXNL = 8, EM_MAXGRID = 1024;

__global__ __launch_bounds__(EM_THREADS) void eval_merge_kernel(int W, int NL, long long cap, long long out_cap, const long long* __restrict__ words,
                                                                const float* __restrict__ results, const long long* __restrict__ truths,
                                                                long long* __restrict__ words_out, float* __restrict__ results_out,
                                                                long long* __restrict__ truths_out) {
    __shared__ long long n_of[EM_MAXW], start_of[EM_MAXW], seen_of[EM_MAXW];
    __shared__ long long total_rows, seen_rows;
    const int tid = threadIdx.x;
    const int nw = 2 + NL * NL + 1;                          // words per rank, the cursor last
    if (tid < W) {
        const long long c = words[(size_t)tid * nw + nw - 1];
        seen_of[tid] = c > 0 ? c : 0;
        n_of[tid] = c < 0 ? 0 : (c > cap ? cap : c);
    }
    __syncthreads();
    if (tid == 0) {
        long long s = 0, seen = 0;
        for (int r = 0; r < W; ++r) {
            start_of[r] = s;
            s += n_of[r];
            seen += seen_of[r];
        }
        total_rows = s;
        seen_rows = seen;
    }
    __syncthreads();
    const long long per_rank = cap * NL, elems = per_rank * W;
    for (long long e = (long long)blockIdx.x * EM_THREADS + tid; e < elems; e += (long long)gridDim.x * EM_THREADS) {
        const int r = (int)(e / per_rank);
        const long long rem = e - (long long)r * per_rank;
        const long long i = rem / NL;
        const int c = (int)(rem - i * NL);
        if (i >= n_of[r]) continue;
        const long long dst = start_of[r] + i;
        if (dst >= out_cap) continue;
        results_out[dst * NL + c] = results[e];
        if (c == 0) truths_out[dst] = truths[(long long)r * cap + i];
    }
    if (blockIdx.x != 0) return;
    if (tid == 0) {
        double s = 0.0;
        bool first = true;
        for (int r = 0; r < W; ++r) {
            if (seen_of[r] == 0) continue;
            const double l = __longlong_as_double(words[(size_t)r * nw]);
            s = first ? l : s + l;
            first = false;
        }
        words_out[0] = __double_as_longlong(s);
    } else if (tid < nw - 1) {
        long long s = 0;
        for (int r = 0; r < W; ++r)
            if (seen_of[r] != 0) s += words[(size_t)r * nw + tid];
        words_out[tid] = s;
    } else if (tid == nw - 1) {
        const long long kept = total_rows < out_cap ? total_rows : out_cap;
        words_out[tid] = seen_rows == kept ? kept : out_cap + (seen_rows - kept);
    }
}

}  // namespace

extern "C" int fmmt_eval_merge(int W, int NL, int64_t cap, int64_t out_cap, const int64_t* words, const float* results, const int64_t* truths,
                               int64_t* words_out, float* results_out, int64_t* truths_out, void* stream) {
    if (W < 1 || W > EM_MAXW || NL < 1 || NL > EM_MAXNL || cap < 0 || out_cap < 0) return FMMT_EINVAL;
    if (!words || !results || !truths || !words_out || !results_out || !truths_out) return FMMT_EINVAL;
    if (((uintptr_t)words | (uintptr_t)truths | (uintptr_t)words_out | (uintptr_t)truths_out) & 7) return FMMT_EALIGN;
    if (((uintptr_t)results | (uintptr_t)results_out) & 3) return FMMT_EALIGN;
    static_assert(2 + EM_MAXNL * EM_MAXNL + 1 <= EM_THREADS && EM_MAXW <= EM_THREADS, "one thread per word of a rank, one per rank");
    const long long elems = (long long)cap * NL * W;
    long long blocks = (elems + EM_THREADS - 1) / EM_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > EM_MAXGRID ? EM_MAXGRID : blocks);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(eval_merge_kernel, dim3((unsigned)blocks), dim3(EM_THREADS), 0, st, W, NL, (long long)cap, (long long)out_cap, (const long long*)words,
                       results, (const long long*)truths, (long long*)words_out, results_out, (long long*)truths_out);
    FMMT_CHECK_LAUNCH();
    return 0;
}
