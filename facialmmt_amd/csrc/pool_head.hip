// The tail of the V-only classifier behind its one real GEMM (modules/Transformer.py:8-45 AdditiveAttention, src/models.py:183-188 / :219-221: dropout ->
// classifier, train.py:245-273: cross-entropy), two launches per direction instead of ~42 dependent 2-4 us torch launches (tanh, a 1-column F.linear,
// masked_fill, softmax, bmm, Dropout, the classifier, cross_entropy and their backwards).  ph = P h + b_P and qq = Q query_vector + b_Q stay GEMMs of the caller.
//
//   score_t = v . tanh(ph_t + qq) + v_b, -inf where mask == 0;  alpha = softmax_t(score);  pooled = sum_t alpha_t h_t;
//   logits = W (keep * pooled) + b;  loss = mean_b (logsumexp(logits_b) - logits_b[label_b])
//
// The problem is latency, not bytes (B = 1..16 rows on 256 CUs, 4 x 326 x 768 x 2 tensors ~ 4 MB), so a row's tokens are split over NS workgroups:
//   forward  1: grid (NS, B), 4 waves; a wave owns a token at a time: 16-byte loads of its ph / h rows (lane -> vectors lane + 64 j), the score through a DPP
//               row sum + the gfx950 row / half swaps, flash-style running (max, sum, partial pooled) in fp32 and the log2 domain; the four waves meet in LDS;
//               out: the raw log2 scores (in `alpha`) and one (max, sum, pooled[H]) partial per workgroup.
//   forward  2: ONE workgroup, a wave per row (B <= 16: all rows side by side): merges the NS partials in their order, normalises alpha, draws the keep mask
//               (the counter-based element generator of fmmt_common.h), the NL x H classifier, the row's cross-entropy; the row losses meet in LDS and are
//               summed in a fixed order.  No atomics anywhere.
//   backward 1: grid (NS, B): d(logits) -> d(pooled) (NL x H, recomputed per workgroup: 5 k FMA), then per token
//               d(score_t) = alpha_t (d(pooled) . h_t - d(pooled) . pooled)      (sum_u alpha_u d(alpha_u) IS d(pooled) . pooled: no second pass over the tokens)
//               dh_t = alpha_t d(pooled),  dph_t = d(score_t) v (1 - tanh^2)  (tanh recomputed), and per-lane fp32 sums of d(qq), d(v), d(v_b) over the wave's
//               tokens -> the four waves in LDS in wave order -> one partial row per workgroup.
//   backward 2: grid H / 64: a thread per channel adds the B NS partials in their order (d(qq), d(v)) and forms dW = d(logits)^T (keep * pooled); workgroup 0 also
//               d(b) and d(v_b).  Fixed order throughout: two runs give the same bits.
// The _rows entry points (include/fmmt_pool_head_rows.h) run the SAME four kernels with a divisor source: n_rows != NULL makes the forward's finishing launch count
// the rows whose label lies in [0, NL), store the count and divide by it, and makes the backward read that word on the device instead of dividing by B.
// n_rows == NULL is the B-divisor pair.  Every label valid: count == B, the same division, the same bits.
// The _crit entry points (include/fmmt_loss.h) instantiate the finishing launch and the token launch with CRIT: the row loss and d(logits) of the
// class-weighted, label-smoothed cross-entropy, the divisor a float device word (sum of w[label]).  No weights and eps == 0: the bits of the _rows pair.
// FMMT_BF16: h / ph / dh / dph bf16, everything else and all arithmetic fp32;  FMMT_F32: the same template, nothing rounded.
#include "fmmt_common.h"
#include "../../include/fmmt.h"

namespace {

constexpr int PH_THREADS = 256, PH_WAVES = 4, PH_MAXH = 1024, PH_MAXL = 1024, PH_MAXB = 1024, PH_MAXNL = 8, PH_MAXSPLIT = 32, PH_FIN_WAVES = 16;
constexpr float PH_LOG2E = 1.4426950408889634f;
constexpr unsigned long long PH_SALT = 0x706f6f6c68656164ull;          // "poolhead": the call site of the element generator

// sum over the 64 lanes, the same bits in every lane: DPP rotations inside a 16-lane row (fixed order, as mlp_fused.hip), then the row / half swaps
__device__ __forceinline__ float ph_wave_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));   // row_ror:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));   // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));   // row_ror:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));   // row_ror:1
    return swap_sum(v);
}
// the value of the first lane as a wave-uniform scalar (what follows branches on it)
__device__ __forceinline__ float ph_uniform(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }

// tanh(x) = 1 - 2 / (2^(2 x log2 e) + 1): one v_exp + one v_rcp, absolute error ~1e-7, exact limits +-1
__device__ __forceinline__ float ph_tanh(float x) {
    const float e = __builtin_amdgcn_exp2f(x * (2.0f * PH_LOG2E));
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

template <int VN> __device__ __forceinline__ void ph_loadf(const float* p, float* out) {
#pragma unroll
    for (int q = 0; q < VN / 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[4 * q + e] = v[e];
    }
}

// tokens per workgroup and workgroups per row: about 256 workgroups in all, at least 8 tokens each, at most PH_MAXSPLIT per row
__host__ __device__ inline int ph_splits(int B, int L, int* chunk) {
    int want = 256 / B;
    want = want < 1 ? 1 : (want > PH_MAXSPLIT ? PH_MAXSPLIT : want);
    const int most = (L + 7) / 8;
    const int ns0 = want < most ? want : most;
    *chunk = (L + ns0 - 1) / ns0;
    return (L + *chunk - 1) / *chunk;
}

template <typename T>
__global__ __launch_bounds__(PH_THREADS) void ph_fwd_partial_kernel(int L, int H, int chunk, int NS, const T* __restrict__ h, const T* __restrict__ ph,
                                                                    const float* __restrict__ qq, const float* __restrict__ vw, const float* __restrict__ vb,
                                                                    const float* __restrict__ mask, float* __restrict__ alpha, float* __restrict__ ml,
                                                                    float* __restrict__ ppool) {
    constexpr int VN = Vec<T>::N, JMAX = PH_MAXH / (VN * 64);
    __shared__ float sacc[PH_WAVES][PH_MAXH];
    __shared__ float sm[PH_WAVES], sl[PH_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, b = blockIdx.y;
    const int HV = H / VN;
    float qv[JMAX][VN], vv[JMAX][VN], acc[JMAX][VN];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        const int v = lane + 64 * j;
        if (v < HV) {
            ph_loadf<VN>(qq + v * VN, qv[j]);
            ph_loadf<VN>(vw + v * VN, vv[j]);
        }
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            acc[j][e] = 0.f;
            if (v >= HV) qv[j][e] = vv[j][e] = 0.f;
        }
    }
    const float vbias = vb[0];
    float m = -INFINITY, l = 0.f;
    const int t0 = s * chunk, t1 = min(L, t0 + chunk);
    for (int t = t0 + wave; t < t1; t += PH_WAVES) {
        const size_t row = ((size_t)b * L + t) * H;
        Vec<T> pv[JMAX], hv[JMAX];
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            const int v = lane + 64 * j;
            if (v < HV) {
                pv[j] = ldvec<T>(ph + row + v * VN);
                hv[j] = ldvec<T>(h + row + v * VN);
            } else {
                pv[j] = zerovec<T>();
                hv[j] = zerovec<T>();
            }
        }
        float sc = 0.f;
#pragma unroll
        for (int j = 0; j < JMAX; ++j)
#pragma unroll
            for (int e = 0; e < VN; ++e) sc = fmaf(vv[j][e], ph_tanh(pv[j].get(e) + qv[j][e]), sc);
        sc = ph_uniform(ph_wave_sum(sc)) + vbias;
        const float s2 = mask[(size_t)b * L + t] == 0.f ? -INFINITY : sc * PH_LOG2E;
        if (lane == 0) alpha[(size_t)b * L + t] = s2;       // the raw log2 score: normalised by the finishing launch
        const float mn = fmaxf(m, s2);
        if (mn > -INFINITY) {                               // (wave-uniform) nothing to add while every token so far is masked
            const float f = __builtin_amdgcn_exp2f(m - mn), pr = __builtin_amdgcn_exp2f(s2 - mn);
            l = fmaf(l, f, pr);
#pragma unroll
            for (int j = 0; j < JMAX; ++j)
#pragma unroll
                for (int e = 0; e < VN; ++e) acc[j][e] = fmaf(acc[j][e], f, pr * hv[j].get(e));
            m = mn;
        }
    }
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        const int v = lane + 64 * j;
        if (v < HV) {
#pragma unroll
            for (int e = 0; e < VN; ++e) sacc[wave][v * VN + e] = acc[j][e];
        }
    }
    if (lane == 0) {
        sm[wave] = m;
        sl[wave] = l;
    }
    __syncthreads();
    float M = sm[0];
#pragma unroll
    for (int w = 1; w < PH_WAVES; ++w) M = fmaxf(M, sm[w]);
    float f[PH_WAVES];
#pragma unroll
    for (int w = 0; w < PH_WAVES; ++w) f[w] = sm[w] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sm[w] - M);
    const size_t part = (size_t)b * NS + s;
    for (int c = tid; c < H; c += PH_THREADS) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < PH_WAVES; ++w) a = fmaf(sacc[w][c], f[w], a);       // wave order: fixed
        ppool[part * H + c] = a;
    }
    if (tid == 0) {
        float ls = 0.f;
#pragma unroll
        for (int w = 0; w < PH_WAVES; ++w) ls = fmaf(sl[w], f[w], ls);
        ml[part * 2] = M;
        ml[part * 2 + 1] = ls;
    }
}

template <bool CRIT>
__global__ __launch_bounds__(PH_FIN_WAVES * 64) void ph_fwd_finish_kernel(int B, int L, int H, int NL, int NS, const float* __restrict__ ml,
                                                                          const float* __restrict__ ppool, const float* __restrict__ W,
                                                                          const float* __restrict__ bias, const long long* __restrict__ labels, float p,
                                                                          unsigned long long seed_i, const unsigned long long* __restrict__ seed_ptr,
                                                                          float* __restrict__ alpha, float* __restrict__ pooled, float* __restrict__ keep,
                                                                          float* __restrict__ logits, float* __restrict__ loss,
                                                                          int* __restrict__ n_rows, const float* __restrict__ class_w, float eps,
                                                                          float* __restrict__ den) {
    constexpr int KMAX = PH_MAXH / 64;
    __shared__ float rl[PH_MAXB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    for (int i = tid; i < PH_MAXB; i += blockDim.x) rl[i] = 0.f;
    __syncthreads();
    const ElemDrop dr = elem_drop_setup(p, seed_ptr ? seed_ptr[0] : seed_i, PH_SALT);
    for (int b = wave; b < B; b += nw) {
        const float* mlb = ml + (size_t)b * NS * 2;
        float M = -INFINITY;
        for (int s = 0; s < NS; ++s) M = fmaxf(M, mlb[2 * s]);
        float pl[KMAX], ls = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) pl[k] = 0.f;
        for (int s = 0; s < NS; ++s) {                      // split order: fixed
            const float ms = mlb[2 * s];
            const float f = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - M);
            ls = fmaf(mlb[2 * s + 1], f, ls);
            const float* pp = ppool + ((size_t)b * NS + s) * H;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int c = lane + 64 * k;
                if (c < H) pl[k] = fmaf(pp[c], f, pl[k]);
            }
        }
        const float inv = 1.0f / ls;                        // a row without a valid token: 0 * inf = NaN, as softmax over -inf gives
        float pd[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int c = lane + 64 * k;
            pd[k] = 0.f;
            if (c < H) {
                const size_t e = (size_t)b * H + c;
                const float pr = pl[k] * inv;
                float kp = 1.0f;
                if (p > 0.f) kp = (elem_keep4(dr, (uint32_t)(e >> 2)) >> (e & 3)) & 1u ? dr.inv : 0.f;
                pooled[e] = pr;
                keep[e] = kp;
                pd[k] = pr * kp;
            }
        }
        for (int t = lane; t < L; t += 64) {
            const size_t i = (size_t)b * L + t;
            alpha[i] = __builtin_amdgcn_exp2f(alpha[i] - M) * inv;
        }
        float lg[PH_MAXNL], mx = -INFINITY;
#pragma unroll
        for (int n = 0; n < PH_MAXNL; ++n) {
            lg[n] = -INFINITY;
            if (n < NL) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < KMAX; ++k) {
                    const int c = lane + 64 * k;
                    if (c < H) a = fmaf(W[(size_t)n * H + c], pd[k], a);
                }
                lg[n] = ph_wave_sum(a) + bias[n];
                mx = fmaxf(mx, lg[n]);
            }
        }
        float z = 0.f;
#pragma unroll
        for (int n = 0; n < PH_MAXNL; ++n) z += n < NL ? expf(lg[n] - mx) : 0.f;
        const float lse = mx + logf(z);
        const long long label = labels[b];
        float vl = lse;                                     // a label outside [0, NL) addresses nothing and adds nothing
#pragma unroll
        for (int n = 0; n < PH_MAXNL; ++n) {
            vl = n == (int)label && label >= 0 && label < NL ? lg[n] : vl;
            if (lane == n && n < NL) logits[(size_t)b * NL + n] = lg[n];
        }
        float row = lse - vl;
        if constexpr (CRIT) {                               // include/fmmt_loss.h: (1 - eps) w[y] (-log p_y) + eps / NL sum_c w_c (-log p_c); 0 without a label
            const bool valid = label >= 0 && label < NL;
            float wy = 0.f, t2 = 0.f;
#pragma unroll
            for (int n = 0; n < PH_MAXNL; ++n) {
                const float wn = n < NL ? (class_w != nullptr ? class_w[n] : 1.f) : 0.f;
                wy = n == (int)label ? wn : wy;
                t2 += n < NL ? wn * (lse - lg[n]) : 0.f;
            }
            row = valid ? (1.0f - eps) * wy * row : 0.f;
            if (valid && eps > 0.f) row = fmaf(eps / (float)NL, t2, row);
        }
        if (lane == 0) rl[b] = row;
    }
    __syncthreads();
    if (wave == 0) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < PH_MAXB / 64; ++k) a += rl[lane + 64 * k];
        a = ph_wave_sum(a);
        if (!CRIT && n_rows == nullptr) {
            if (lane == 0) loss[0] = a / (float)B;
        } else {                                            // the mean over the rows that have a label: counted here, in floats (exact: B <= 1024)
            float c = 0.f;
#pragma unroll
            for (int k = 0; k < PH_MAXB / 64; ++k) {
                const int b = lane + 64 * k;
                if (b < B) {
                    const long long label = labels[b];
                    if constexpr (CRIT)                     // the weighted mean's divisor: sum of w[label] over the labelled rows
                        c += label >= 0 && label < NL ? (class_w != nullptr ? class_w[label] : 1.f) : 0.f;
                    else
                        c += label >= 0 && label < NL ? 1.f : 0.f;
                }
            }
            c = ph_wave_sum(c);
            if (lane == 0) {
                if constexpr (CRIT)
                    den[0] = c;
                else
                    n_rows[0] = (int)c;                     // an ordinary vector store
                loss[0] = c > 0.f ? a / c : 0.f;
            }
        }
    }
}

template <typename T, bool CRIT>
__global__ __launch_bounds__(PH_THREADS) void ph_bwd_token_kernel(int B, int L, int H, int NL, int chunk, int NS, const float* __restrict__ dloss,
                                                                  const T* __restrict__ h, const T* __restrict__ ph, const float* __restrict__ qq,
                                                                  const float* __restrict__ vw, const float* __restrict__ W, const long long* __restrict__ labels,
                                                                  const float* __restrict__ logits, const float* __restrict__ alpha,
                                                                  const float* __restrict__ pooled, const float* __restrict__ keep, T* __restrict__ dh,
                                                                  T* __restrict__ dph, float* __restrict__ pq, float* __restrict__ pv, float* __restrict__ pvb,
                                                                  float* __restrict__ dlg, const int* __restrict__ n_rows, const float* __restrict__ class_w,
                                                                  float eps, const float* __restrict__ den) {
    constexpr int VN = Vec<T>::N, JMAX = PH_MAXH / (VN * 64);
    __shared__ float sdp[PH_MAXH];
    __shared__ float sq[PH_WAVES][PH_MAXH], sv[PH_WAVES][PH_MAXH];
    __shared__ float sred[PH_WAVES], svb[PH_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, b = blockIdx.y;
    const int HV = H / VN;
    // d(logits) of the row: dloss / B * (softmax - onehot); n_rows: dloss / (rows that have a label), 0 when there is none
    float dl[PH_MAXNL], mx = -INFINITY;
#pragma unroll
    for (int n = 0; n < PH_MAXNL; ++n) {
        dl[n] = n < NL ? logits[(size_t)b * NL + n] : -INFINITY;
        mx = fmaxf(mx, dl[n]);
    }
    float z = 0.f;
#pragma unroll
    for (int n = 0; n < PH_MAXNL; ++n) {
        dl[n] = n < NL ? expf(dl[n] - mx) : 0.f;
        z += dl[n];
    }
    float g;
    if constexpr (CRIT) {
        const float dn = den[0];
        g = dn > 0.f ? dloss[0] / dn : 0.f;
    } else {
        const int nr = n_rows == nullptr ? B : n_rows[0];
        g = nr > 0 ? dloss[0] / (float)nr : 0.f;
    }
    const long long label = labels[b];
    float k1 = 1.f, k2 = 0.f, tsum = 1.f, cw[PH_MAXNL];
    if constexpr (CRIT) {                                   // include/fmmt_loss.h: t_n = (1 - eps) w[y] [n == y] + eps / NL w_n, d(logits) = g (p sum_n t_n - t)
        float wy = 0.f, wsum = 0.f;
#pragma unroll
        for (int n = 0; n < PH_MAXNL; ++n) {
            cw[n] = n < NL ? (class_w != nullptr ? class_w[n] : 1.f) : 0.f;
            wy = n == (int)label ? cw[n] : wy;
            wsum += cw[n];
        }
        k1 = (1.0f - eps) * wy;
        k2 = eps / (float)NL;
        tsum = fmaf(k2, wsum, k1);
    }
#pragma unroll
    for (int n = 0; n < PH_MAXNL; ++n) {
        const bool valid = label >= 0 && label < NL;
        if constexpr (CRIT)
            dl[n] = valid && n < NL ? g * (dl[n] / z * tsum - fmaf(k2, cw[n], n == (int)label ? k1 : 0.f)) : 0.f;
        else
            dl[n] = valid && n < NL ? g * (dl[n] / z - (n == (int)label ? 1.f : 0.f)) : 0.f;
        if (s == 0 && tid == n) dlg[(size_t)b * PH_MAXNL + n] = dl[n];
    }
    // d(pooled) = keep * W^T d(logits), and its product with the pooled vector
    float part = 0.f;
    for (int c = tid; c < H; c += PH_THREADS) {
        float a = 0.f;
#pragma unroll
        for (int n = 0; n < PH_MAXNL; ++n)
            if (n < NL) a = fmaf(W[(size_t)n * H + c], dl[n], a);
        a *= keep[(size_t)b * H + c];
        sdp[c] = a;
        part = fmaf(a, pooled[(size_t)b * H + c], part);
    }
    part = ph_wave_sum(part);
    if (lane == 0) sred[wave] = part;
    __syncthreads();
    const float dot = ((sred[0] + sred[1]) + sred[2]) + sred[3];
    float qv[JMAX][VN], vv[JMAX][VN], dpv[JMAX][VN], dqa[JMAX][VN], dva[JMAX][VN];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        const int v = lane + 64 * j;
        if (v < HV) {
            ph_loadf<VN>(qq + v * VN, qv[j]);
            ph_loadf<VN>(vw + v * VN, vv[j]);
        }
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            dqa[j][e] = dva[j][e] = 0.f;
            dpv[j][e] = v < HV ? sdp[v * VN + e] : 0.f;
            if (v >= HV) qv[j][e] = vv[j][e] = 0.f;
        }
    }
    float dvb = 0.f;
    const int t0 = s * chunk, t1 = min(L, t0 + chunk);
    for (int t = t0 + wave; t < t1; t += PH_WAVES) {
        const size_t row = ((size_t)b * L + t) * H;
        const float a = alpha[(size_t)b * L + t];
        Vec<T> pvx[JMAX], hv[JMAX];
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            const int v = lane + 64 * j;
            if (v < HV) {
                pvx[j] = ldvec<T>(ph + row + v * VN);
                hv[j] = ldvec<T>(h + row + v * VN);
            } else {
                pvx[j] = zerovec<T>();
                hv[j] = zerovec<T>();
            }
        }
        float da = 0.f;
#pragma unroll
        for (int j = 0; j < JMAX; ++j)
#pragma unroll
            for (int e = 0; e < VN; ++e) da = fmaf(dpv[j][e], hv[j].get(e), da);
        const float ds = a * (ph_uniform(ph_wave_sum(da)) - dot);
        dvb += ds;
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            const int v = lane + 64 * j;
            Vec<T> oh, op;
#pragma unroll
            for (int e = 0; e < VN; ++e) {
                const float th = ph_tanh(pvx[j].get(e) + qv[j][e]);
                const float gp = ds * vv[j][e] * (1.0f - th * th);
                dqa[j][e] += gp;
                dva[j][e] = fmaf(ds, th, dva[j][e]);
                op.set(e, gp);
                oh.set(e, a * dpv[j][e]);
            }
            if (v < HV) {
                stvec<T>(dph + row + v * VN, op);
                stvec<T>(dh + row + v * VN, oh);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        const int v = lane + 64 * j;
        if (v < HV) {
#pragma unroll
            for (int e = 0; e < VN; ++e) {
                sq[wave][v * VN + e] = dqa[j][e];
                sv[wave][v * VN + e] = dva[j][e];
            }
        }
    }
    if (lane == 0) svb[wave] = dvb;
    __syncthreads();
    const size_t prt = (size_t)b * NS + s;
    for (int c = tid; c < H; c += PH_THREADS) {             // wave order: fixed
        pq[prt * H + c] = ((sq[0][c] + sq[1][c]) + sq[2][c]) + sq[3][c];
        pv[prt * H + c] = ((sv[0][c] + sv[1][c]) + sv[2][c]) + sv[3][c];
    }
    if (tid == 0) pvb[prt] = ((svb[0] + svb[1]) + svb[2]) + svb[3];
}

__global__ __launch_bounds__(64) void ph_bwd_finish_kernel(int B, int H, int NL, int NS, const float* __restrict__ pq, const float* __restrict__ pv,
                                                           const float* __restrict__ pvb, const float* __restrict__ dlg, const float* __restrict__ pooled,
                                                           const float* __restrict__ keep, float* __restrict__ dqq, float* __restrict__ dv,
                                                           float* __restrict__ dvb, float* __restrict__ dW, float* __restrict__ db) {
    const int lane = threadIdx.x, c = blockIdx.x * 64 + lane;
    const int NP = B * NS;
    if (c < H) {
        float aq = 0.f, av = 0.f;
#pragma unroll 4
        for (int i = 0; i < NP; ++i) {                       // (row, split) order: fixed
            aq += pq[(size_t)i * H + c];
            av += pv[(size_t)i * H + c];
        }
        dqq[c] = aq;
        dv[c] = av;
        float w[PH_MAXNL];
#pragma unroll
        for (int n = 0; n < PH_MAXNL; ++n) w[n] = 0.f;
        for (int b = 0; b < B; ++b) {
            const float pd = pooled[(size_t)b * H + c] * keep[(size_t)b * H + c];
#pragma unroll
            for (int n = 0; n < PH_MAXNL; ++n) w[n] = fmaf(dlg[(size_t)b * PH_MAXNL + n], pd, w[n]);
        }
#pragma unroll
        for (int n = 0; n < PH_MAXNL; ++n)
            if (n < NL) dW[(size_t)n * H + c] = w[n];
    }
    if (blockIdx.x == 0) {
        if (lane < NL) {
            float a = 0.f;
            for (int b = 0; b < B; ++b) a += dlg[(size_t)b * PH_MAXNL + lane];
            db[lane] = a;
        }
        if (lane == PH_MAXNL) {
            float a = 0.f;
            for (int i = 0; i < NP; ++i) a += pvb[i];
            dvb[0] = a;
        }
    }
}

inline size_t ph_round(size_t n) { return (n + 255) / 256 * 256; }

int ph_check_shape(int dtype, int B, int L, int H, int NL) {
    if (dtype != FMMT_BF16 && dtype != FMMT_F32) return FMMT_EINVAL;
    if (B < 1 || B > PH_MAXB || L < 2 || L > PH_MAXL || H < 8 || H > PH_MAXH || H % 8 || NL < 1 || NL > PH_MAXNL) return FMMT_EINVAL;
    return 0;
}

}  // namespace

// one size for both directions (the backward's is the larger): [B NS][H] x 2 + [B NS] partials and the [B][8] d(logits); the forward uses
// [B NS][2] + [B NS][H] of it
extern "C" size_t fmmt_pool_head_bwd_workspace(int B, int L, int H) {
    if (B < 1 || B > PH_MAXB || L < 2 || L > PH_MAXL || H < 8 || H > PH_MAXH) return 0;
    int chunk;
    const size_t np = (size_t)B * ph_splits(B, L, &chunk);
    return ph_round(np * H * 4) * 2 + ph_round(np * 4) + ph_round((size_t)B * PH_MAXNL * 4);
}

namespace {

// the loss of include/fmmt_loss.h behind the classifier: den != NULL instantiates the finishing / token kernels with it
struct PhCrit {
    const float* class_w = nullptr;
    float eps = 0.f;
    float* den = nullptr;
};

// the forward entry points: n_rows == NULL divides by B, else by the counted rows (stored in n_rows[0]); crit.den: by the weight sum stored there
int ph_fwd(int dtype, int B, int L, int H, int NL, const void* h, const void* ph, const float* qq, const float* value_w, const float* value_b, const float* mask,
           const float* cls_w, const float* cls_b, const int64_t* labels, float p, uint64_t seed, const uint64_t* seed_dev, float* logits, float* loss, float* alpha,
           float* pooled, float* keep, int32_t* n_rows, void* workspace, size_t workspace_bytes, void* stream, PhCrit crit = PhCrit()) {
    if (int rc = ph_check_shape(dtype, B, L, H, NL)) return rc;
    if (!(p >= 0.f) || !(p < 1.f)) return FMMT_EINVAL;
    if (!h || !ph || !qq || !value_w || !value_b || !mask || !cls_w || !cls_b || !labels || !logits || !loss || !alpha || !pooled || !keep || !workspace) return FMMT_EINVAL;
    if (((uintptr_t)h | (uintptr_t)ph | (uintptr_t)qq | (uintptr_t)value_w | (uintptr_t)workspace) & 15) return FMMT_EALIGN;
    if (workspace_bytes < fmmt_pool_head_bwd_workspace(B, L, H)) return FMMT_EWORKSPACE;
    int chunk;
    const int NS = ph_splits(B, L, &chunk);
    float* ppool = (float*)workspace;
    float* ml = (float*)((char*)workspace + ph_round((size_t)B * NS * H * 4));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(NS, B);
    if (dtype == FMMT_BF16)
        hipLaunchKernelGGL(ph_fwd_partial_kernel<bf16>, grid, dim3(PH_THREADS), 0, st, L, H, chunk, NS, (const bf16*)h, (const bf16*)ph, qq, value_w, value_b, mask,
                           alpha, ml, ppool);
    else
        hipLaunchKernelGGL(ph_fwd_partial_kernel<float>, grid, dim3(PH_THREADS), 0, st, L, H, chunk, NS, (const float*)h, (const float*)ph, qq, value_w, value_b, mask,
                           alpha, ml, ppool);
    FMMT_CHECK_LAUNCH();
    const int nw = B < PH_FIN_WAVES ? B : PH_FIN_WAVES;
    if (crit.den != nullptr)
        hipLaunchKernelGGL(ph_fwd_finish_kernel<true>, dim3(1), dim3(nw * 64), 0, st, B, L, H, NL, NS, ml, ppool, cls_w, cls_b, (const long long*)labels, p,
                           (unsigned long long)seed, (const unsigned long long*)seed_dev, alpha, pooled, keep, logits, loss, (int*)nullptr, crit.class_w, crit.eps,
                           crit.den);
    else
        hipLaunchKernelGGL(ph_fwd_finish_kernel<false>, dim3(1), dim3(nw * 64), 0, st, B, L, H, NL, NS, ml, ppool, cls_w, cls_b, (const long long*)labels, p,
                           (unsigned long long)seed, (const unsigned long long*)seed_dev, alpha, pooled, keep, logits, loss, (int*)n_rows, (const float*)nullptr, 0.f,
                           (float*)nullptr);
    FMMT_CHECK_LAUNCH();
    return 0;
}

// the backward entry points: crit.den != NULL divides by that float device word; n_rows == NULL divides by B, else by the device word the forward wrote
int ph_bwd(int dtype, int B, int L, int H, int NL, const float* dloss, const void* h, const void* ph, const float* qq, const float* value_w, const float* cls_w,
           const int64_t* labels, const float* logits, const float* alpha, const float* pooled, const float* keep, const int32_t* n_rows, void* dh, void* dph,
           float* dqq, float* dv, float* dvb, float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream, PhCrit crit = PhCrit()) {
    if (int rc = ph_check_shape(dtype, B, L, H, NL)) return rc;
    if (!dloss || !h || !ph || !qq || !value_w || !cls_w || !labels || !logits || !alpha || !pooled || !keep || !dh || !dph || !dqq || !dv || !dvb || !dW || !db ||
        !workspace)
        return FMMT_EINVAL;
    if (((uintptr_t)h | (uintptr_t)ph | (uintptr_t)qq | (uintptr_t)value_w | (uintptr_t)dh | (uintptr_t)dph | (uintptr_t)workspace) & 15) return FMMT_EALIGN;
    if (workspace_bytes < fmmt_pool_head_bwd_workspace(B, L, H)) return FMMT_EWORKSPACE;
    int chunk;
    const int NS = ph_splits(B, L, &chunk);
    const size_t np = (size_t)B * NS;
    char* w = (char*)workspace;
    float* pq = (float*)w;
    float* pv = (float*)(w + ph_round(np * H * 4));
    float* pvb = (float*)(w + 2 * ph_round(np * H * 4));
    float* dlg = (float*)(w + 2 * ph_round(np * H * 4) + ph_round(np * 4));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(NS, B);
    const float* cwp = crit.class_w;
    const float* dnp = crit.den;
    if (dtype == FMMT_BF16 && dnp != nullptr)
        hipLaunchKernelGGL((ph_bwd_token_kernel<bf16, true>), grid, dim3(PH_THREADS), 0, st, B, L, H, NL, chunk, NS, dloss, (const bf16*)h, (const bf16*)ph, qq, value_w,
                           cls_w, (const long long*)labels, logits, alpha, pooled, keep, (bf16*)dh, (bf16*)dph, pq, pv, pvb, dlg, (const int*)nullptr, cwp, crit.eps, dnp);
    else if (dtype == FMMT_BF16)
        hipLaunchKernelGGL((ph_bwd_token_kernel<bf16, false>), grid, dim3(PH_THREADS), 0, st, B, L, H, NL, chunk, NS, dloss, (const bf16*)h, (const bf16*)ph, qq, value_w,
                           cls_w, (const long long*)labels, logits, alpha, pooled, keep, (bf16*)dh, (bf16*)dph, pq, pv, pvb, dlg, (const int*)n_rows, cwp, 0.f, dnp);
    else if (dnp != nullptr)
        hipLaunchKernelGGL((ph_bwd_token_kernel<float, true>), grid, dim3(PH_THREADS), 0, st, B, L, H, NL, chunk, NS, dloss, (const float*)h, (const float*)ph, qq, value_w,
                           cls_w, (const long long*)labels, logits, alpha, pooled, keep, (float*)dh, (float*)dph, pq, pv, pvb, dlg, (const int*)nullptr, cwp, crit.eps, dnp);
    else
        hipLaunchKernelGGL((ph_bwd_token_kernel<float, false>), grid, dim3(PH_THREADS), 0, st, B, L, H, NL, chunk, NS, dloss, (const float*)h, (const float*)ph, qq, value_w,
                           cls_w, (const long long*)labels, logits, alpha, pooled, keep, (float*)dh, (float*)dph, pq, pv, pvb, dlg, (const int*)n_rows, cwp, 0.f, dnp);
    FMMT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ph_bwd_finish_kernel, dim3((H + 63) / 64), dim3(64), 0, st, B, H, NL, NS, pq, pv, pvb, dlg, pooled, keep, dqq, dv, dvb, dW, db);
    FMMT_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int fmmt_pool_head_fwd(int dtype, int B, int L, int H, int NL, const void* h, const void* ph, const float* qq, const float* value_w,
                                  const float* value_b, const float* mask, const float* cls_w, const float* cls_b, const int64_t* labels, float p, uint64_t seed,
                                  const uint64_t* seed_dev, float* logits, float* loss, float* alpha, float* pooled, float* keep, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return ph_fwd(dtype, B, L, H, NL, h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p, seed, seed_dev, logits, loss, alpha, pooled, keep, nullptr, workspace,
                  workspace_bytes, stream);
}

extern "C" int fmmt_pool_head_bwd(int dtype, int B, int L, int H, int NL, const float* dloss, const void* h, const void* ph, const float* qq,
                                  const float* value_w, const float* cls_w, const int64_t* labels, const float* logits, const float* alpha, const float* pooled,
                                  const float* keep, void* dh, void* dph, float* dqq, float* dv, float* dvb, float* dW, float* db, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return ph_bwd(dtype, B, L, H, NL, dloss, h, ph, qq, value_w, cls_w, labels, logits, alpha, pooled, keep, nullptr, dh, dph, dqq, dv, dvb, dW, db, workspace,
                  workspace_bytes, stream);
}

// the mean over the rows that have a label (include/fmmt_pool_head_rows.h): the same launches, the divisor counted on the device
extern "C" int fmmt_pool_head_fwd_rows(int dtype, int B, int L, int H, int NL, const void* h, const void* ph, const float* qq, const float* value_w,
                                       const float* value_b, const float* mask, const float* cls_w, const float* cls_b, const int64_t* labels, float p,
                                       uint64_t seed, const uint64_t* seed_dev, float* logits, float* loss, float* alpha, float* pooled, float* keep,
                                       int32_t* n_rows, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = ph_check_shape(dtype, B, L, H, NL)) return rc;     // the shape first, as the B-divisor pair answers it
    if (!n_rows) return FMMT_EINVAL;
    return ph_fwd(dtype, B, L, H, NL, h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p, seed, seed_dev, logits, loss, alpha, pooled, keep, n_rows, workspace,
                  workspace_bytes, stream);
}

extern "C" int fmmt_pool_head_bwd_rows(int dtype, int B, int L, int H, int NL, const float* dloss, const void* h, const void* ph, const float* qq,
                                       const float* value_w, const float* cls_w, const int64_t* labels, const float* logits, const float* alpha,
                                       const float* pooled, const float* keep, const int32_t* n_rows, void* dh, void* dph, float* dqq, float* dv, float* dvb,
                                       float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = ph_check_shape(dtype, B, L, H, NL)) return rc;
    if (!n_rows) return FMMT_EINVAL;
    return ph_bwd(dtype, B, L, H, NL, dloss, h, ph, qq, value_w, cls_w, labels, logits, alpha, pooled, keep, n_rows, dh, dph, dqq, dv, dvb, dW, db, workspace,
                  workspace_bytes, stream);
}

// the head with the loss of include/fmmt_loss.h: the same launches, the divisor a float device word (sum of w[label] over the labelled rows)
extern "C" int fmmt_pool_head_fwd_crit(int dtype, int B, int L, int H, int NL, const void* h, const void* ph, const float* qq, const float* value_w,
                                       const float* value_b, const float* mask, const float* cls_w, const float* cls_b, const int64_t* labels, float p,
                                       uint64_t seed, const uint64_t* seed_dev, float* logits, float* loss, float* alpha, float* pooled, float* keep,
                                       const float* class_w, float smoothing, float* den, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = ph_check_shape(dtype, B, L, H, NL)) return rc;
    if (!den || !(smoothing >= 0.f) || !(smoothing < 1.f)) return FMMT_EINVAL;
    PhCrit crit;
    crit.class_w = class_w;
    crit.eps = smoothing;
    crit.den = den;
    return ph_fwd(dtype, B, L, H, NL, h, ph, qq, value_w, value_b, mask, cls_w, cls_b, labels, p, seed, seed_dev, logits, loss, alpha, pooled, keep, nullptr, workspace,
                  workspace_bytes, stream, crit);
}

extern "C" int fmmt_pool_head_bwd_crit(int dtype, int B, int L, int H, int NL, const float* dloss, const void* h, const void* ph, const float* qq,
                                       const float* value_w, const float* cls_w, const int64_t* labels, const float* logits, const float* alpha,
                                       const float* pooled, const float* keep, const float* class_w, float smoothing, const float* den, void* dh, void* dph,
                                       float* dqq, float* dv, float* dvb, float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = ph_check_shape(dtype, B, L, H, NL)) return rc;
    if (!den || !(smoothing >= 0.f) || !(smoothing < 1.f)) return FMMT_EINVAL;
    PhCrit crit;
    crit.class_w = class_w;
    crit.eps = smoothing;
    crit.den = const_cast<float*>(den);
    return ph_bwd(dtype, B, L, H, NL, dloss, h, ph, qq, value_w, cls_w, labels, logits, alpha, pooled, keep, nullptr, dh, dph, dqq, dv, dvb, dW, db, workspace,
                  workspace_bytes, stream, crit);
}
