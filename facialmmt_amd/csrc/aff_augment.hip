// The Aff-Wild2 training augmentation of the auxiliary task (utils/util.py:22-60, utils/random_erasing.py) inside the uint8 pre-step: bicubic resize ->
// Grayscale(3) -> the frame's ColorJitter operations -> Pillow's GaussianBlur (three box passes along x, three along y) -> ToTensor / Normalize table ->
// RandomErasing's rectangle of N(0, 1) values -> 4x4 patch gather (-> PatchEmbed's projection + LayerNorm).  include/fmmt_aug.h states the arithmetic
// and the noise generator; tests/support_aff_augment.py restates both in numpy, the byte stages held to Pillow bit for bit.
//
// The blur needs six rows of the jittered frame above and below a band, and the jitter's contrast needs the whole frame's mean, so the frame goes
// through a byte workspace (n, 224, 224, 3) once.  Three launches on the same grid (56 bands, n):
//   jitter_stats_kernel  (jitter_core.h, reading this record, grayscale in front)      -> partial[n][56]       (frames without contrast: exit)
//   aug_pixels_kernel    resize, grayscale, the jitter operations                      -> frames_ws, the band's bytes
//   aug_finish_kernel    rows 4p-6 .. 4p+9 of frames_ws in LDS, the six passes between two LDS images, table, rectangle, gather (, projection + LayerNorm)
// A y pass is valid on two rows fewer per side than its input; after three the band's four rows remain.  Every index is clamped to the FRAME (as
// Pillow clamps to the image), never to the staged window: rows outside the frame are staged as copies of the edge row and not read again.
#include "jitter_core.h"

namespace {

constexpr int HALO = FMMT_AUG_HALO;           // rows above / below the band that three y passes reach (2 per pass at r = 1)
constexpr int SROWS = 4 + 2 * HALO;           // staged rows
constexpr int ROWW = ROWB / 4;                // a row in 32-bit words
static_assert(HALO == 3 * (FMMT_AUG_MAX_RADIUS + 1) && ROWB % 16 == 0, "the halo is sized for the largest radius; rows are whole 16-byte chunks");

struct AugRec {
    JitRec j;
    bool gray;
    int r;                                    // -1: no blur
    uint32_t ww, fw;
    int top, left, eh, ew;                    // eh == 0: nothing erased
    uint32_t ka, kb;                          // the hashed noise key
};
__device__ __forceinline__ AugRec load_aug(const int32_t* __restrict__ aug, int n) {
    const int32_t* r = aug + (size_t)n * FMMT_AUG_WORDS;
    AugRec a;
    a.j = load_rec(r, 0);
    a.gray = r[8] & FMMT_AUG_FLAG_GRAY;
    a.r = (r[9] == 0 || r[9] == 1) ? r[9] : -1;
    a.ww = (uint32_t)r[10];
    a.fw = (uint32_t)r[11];
    a.top = r[12];
    a.left = r[13];
    a.eh = r[14];
    a.ew = r[15];
    a.ka = mix32a((uint32_t)r[16] ^ 0x9e3779b9U);
    a.kb = mix32b((uint32_t)r[17] ^ 0x7f4a7c15U);
    return a;
}

// N(0, 1) of counter n under the hashed key (fmmt_aug.h): Box-Muller on two 24-bit uniforms, library logf / sinf / sqrtf
__device__ __forceinline__ float aug_noise(uint32_t n, uint32_t ka, uint32_t kb) {
    const uint32_t h1 = mix32a(mix32b(n ^ ka) + kb), h2 = mix32b(mix32a(n + kb) ^ ka);
    const float u1 = (float)((h1 >> 8) + 1u) * 0x1p-24f, x = (float)(h2 >> 8) * 0x1p-23f;      // x = 2 u2 in [0, 2), exact
    // cos(pi x) = cos(pi (2 - x)) = sin(pi (1/2 - x)): both reductions are exact in float32, so the product keeps its RELATIVE accuracy at the cosine's
    // zero crossings (cosf of a rounded 2 pi u2, and cospif, are only good to an ulp of 1 there)
    return sqrtf(-2.0f * logf(u1)) * sinf(3.14159265358979f * (0.5f - fminf(x, 2.0f - x)));
}

// one box pass at a position from the five values around it (r = 0 reads three of them)
__device__ __forceinline__ uint8_t box_px(uint32_t m2, uint32_t m1, uint32_t c, uint32_t p1, uint32_t p2, int r, uint32_t ww, uint32_t fw) {
    const uint32_t sum = r ? m1 + c + p1 : c, far = r ? m2 + p2 : m1 + p1;
    return (uint8_t)((ww * sum + fw * far + (1u << 23)) >> 24);
}

// block = (patch row p, image n); 256 threads: the band's resized, greyed and jittered bytes -> frames_ws
template <bool PIL>
__global__ __launch_bounds__(256) void aug_pixels_kernel(const uint8_t* __restrict__ img, int S, const int32_t* __restrict__ tab,
                                                         const int32_t* __restrict__ aug, const int32_t* __restrict__ partial,
                                                         uint8_t* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) uint8_t src[RMAX * SMAX * 3];
    __shared__ __attribute__((aligned(16))) uint8_t rb[4 * ROWB];
    const int p = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int32_t* rec = aug + (size_t)n * FMMT_AUG_WORDS;
    const JitRec j = load_rec(rec, 0);
    const bool gray = rec[8] & FMMT_AUG_FLAG_GRAY;
    float m = 0.f;
    if (has_contrast(j)) {                                   // uniform addresses: scalar loads; Pillow's int(mean + 0.5) in integers
        int total = 0;
        for (int q = 0; q < GRID; ++q) total += partial[(size_t)n * GRID + q];
        m = (float)((2 * total + NPIX) / (2 * NPIX));
    }
    resize_band<PIL>(img, S, tab, p, n, tid, src, rb);
    const bool any = gray || j.op[0] != FMMT_JITTER_NONE || j.op[1] != FMMT_JITTER_NONE || j.op[2] != FMMT_JITTER_NONE || j.op[3] != FMMT_JITTER_NONE;
    if (any) {                                               // uniform; a thread rewrites its own pixels in place
        for (int q = tid; q < 4 * OUT; q += 256) {
            int r = rb[q * 3], g = rb[q * 3 + 1], b = rb[q * 3 + 2];
            if (gray) r = g = b = luma(r, g, b);
            jitter_px<false>(r, g, b, j, m);
            rb[q * 3] = (uint8_t)r;
            rb[q * 3 + 1] = (uint8_t)g;
            rb[q * 3 + 2] = (uint8_t)b;
        }
        __syncthreads();
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(ws + ((size_t)n * OUT + 4 * p) * ROWB);      // the band's four rows are contiguous
    const uint32_t* rb4 = reinterpret_cast<const uint32_t*>(rb);
    for (int i = tid; i < 4 * ROWW; i += 256) out[i] = rb4[i];
}

// block = (patch row p, image n); 256 threads: blur, table, rectangle, gather (, projection + LayerNorm) of band p from frames_ws
template <typename T, bool FUSE>
__global__ __launch_bounds__(256) void aug_finish_kernel(const uint8_t* __restrict__ ws, const float* __restrict__ lut, const int32_t* __restrict__ aug,
                                                         T* __restrict__ cols, PeTail<T> tail) {
    __shared__ __attribute__((aligned(16))) uint8_t bufa[SROWS * ROWB];
    __shared__ __attribute__((aligned(16))) uint8_t bufb[SROWS * ROWB];
    __shared__ __attribute__((aligned(16))) T colsl[64 * CPITCH];
    __shared__ float slut[256];
    const int p = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    slut[tid] = lut[tid];
    const AugRec a = load_aug(aug, n);
    if constexpr (FUSE) {
        for (int e = tid; e < 8 * KPATCH; e += 256) colsl[(GRID + e / KPATCH) * CPITCH + e % KPATCH] = from_f32<T>(0.f);   // rows 56-63 of the last wave's tile
    }
    const int y0 = 4 * p - HALO;                             // frame row of staged row 0
    const uint32_t* w4 = reinterpret_cast<const uint32_t*>(ws + (size_t)n * NPIX * 3);
    uint32_t* a4 = reinterpret_cast<uint32_t*>(bufa);
    const int s_lo = a.r >= 0 ? 0 : HALO, s_n = a.r >= 0 ? SROWS : 4;         // without a blur: the band's rows alone
    for (int i = tid; i < s_n * ROWW; i += 256) {
        const int s = s_lo + i / ROWW, k = i % ROWW;
        const int y = min(max(y0 + s, 0), OUT - 1);
        a4[s * ROWW + k] = w4[y * ROWW + k];
    }
    __syncthreads();                                         // (covers slut and the tile's zero rows)
    const uint8_t* in = bufa;
    if (a.r >= 0) {                                          // uniform
        uint8_t* out = bufb;
        const int r = a.r;
        for (int pass = 0; pass < 3; ++pass) {               // along x, every staged row
            for (int e = tid; e < SROWS * ROWB; e += 256) {
                const int s = e / ROWB, rem = e - s * ROWB, x = rem / 3, c = rem - 3 * x;
                const uint8_t* row = in + s * ROWB + c;
                const uint32_t v0 = row[x * 3], m1 = row[max(x - 1, 0) * 3], p1 = row[min(x + 1, OUT - 1) * 3];
                uint32_t m2 = 0, p2 = 0;
                if (r) {
                    m2 = row[max(x - 2, 0) * 3];
                    p2 = row[min(x + 2, OUT - 1) * 3];
                }
                out[e] = box_px(m2, m1, v0, p1, p2, r, a.ww, a.fw);
            }
            __syncthreads();
            const uint8_t* t = in;
            in = out;
            out = const_cast<uint8_t*>(t);
        }
        for (int pass = 1; pass <= 3; ++pass) {              // along y: staged rows 2 pass .. 15 - 2 pass that lie in the frame, reading rows of the frame
            const int lo = 2 * pass, cnt = SROWS - 4 * pass;
            for (int e = tid; e < cnt * ROWB; e += 256) {
                const int s = lo + e / ROWB, col = e % ROWB, y = y0 + s;
                if (y < 0 || y >= OUT) continue;
                const int at = col - y0 * ROWB;              // in[at + yy * ROWB]: frame row yy; yy - y0 stays in 2 pass - 2 .. 17 - 2 pass
                const uint32_t v0 = in[at + y * ROWB], m1 = in[at + max(y - 1, 0) * ROWB], p1 = in[at + min(y + 1, OUT - 1) * ROWB];
                uint32_t m2 = 0, p2 = 0;
                if (r) {
                    m2 = in[at + max(y - 2, 0) * ROWB];
                    p2 = in[at + min(y + 2, OUT - 1) * ROWB];
                }
                out[s * ROWB + col] = box_px(m2, m1, v0, p1, p2, r, a.ww, a.fw);
            }
            __syncthreads();
            const uint8_t* t = in;
            in = out;
            out = const_cast<uint8_t*>(t);
        }
    }
    const uint8_t* band = in + HALO * ROWB;                  // six passes: back in bufa
    for (int q = tid; q < 4 * OUT; q += 256) {
        const int dy = q / OUT, x = q - dy * OUT, y = 4 * p + dy;
        float vr = slut[band[q * 3]], vg = slut[band[q * 3 + 1]], vb = slut[band[q * 3 + 2]];
        if ((unsigned)(y - a.top) < (unsigned)a.eh && (unsigned)(x - a.left) < (unsigned)a.ew) {      // eh, ew <= 0: never
            const uint32_t ctr = (uint32_t)(y * OUT + x);
            vr = aug_noise(ctr, a.ka, a.kb);
            vg = aug_noise(ctr + NPIX, a.ka, a.kb);
            vb = aug_noise(ctr + 2 * NPIX, a.ka, a.kb);
        }
        T* o = colsl + (x >> 2) * CPITCH + dy * 4 + (x & 3);
        o[0] = from_f32<T>(vr);
        o[16] = from_f32<T>(vg);
        o[32] = from_f32<T>(vb);
    }
    __syncthreads();
    if (!FUSE || cols) {                                     // the patch matrix of the band: 56 rows of 48 values, whole 16-byte chunks
        constexpr int CH = 16 / (int)sizeof(T), CPR = KPATCH / CH;
        T* out = cols + ((size_t)n * GRID + p) * GRID * KPATCH;
        for (int q = tid; q < GRID * CPR; q += 256) {
            const int patch = q / CPR, ch = q - patch * CPR;
            *reinterpret_cast<uint4*>(out + patch * KPATCH + ch * CH) = *reinterpret_cast<const uint4*>(colsl + patch * CPITCH + ch * CH);
        }
    }
    if constexpr (FUSE) {
        using E = ElemTrait<T>;
        const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
        const int patch = wave * 16 + li;
        const typename E::frag c0 = E::ld(colsl + patch * CPITCH + lg * 8);
        const typename E::frag c1 = lg < 2 ? E::ld(colsl + patch * CPITCH + 32 + lg * 8) : E::zero();
        patch_ln_tile_lean<T>(tail.w, tail.bias, tail.gamma, tail.beta, c0, c1, tail.eps, ((size_t)n * GRID + p) * GRID + patch, patch < GRID, li, lg,
                              tail.x_pre, tail.y, tail.mean, tail.rstd);
    }
}

template <typename T, bool FUSE>
int launch(int mode, int n_img, int in_size, const uint8_t* img, const int32_t* tab, const float* lut, const int32_t* aug, int32_t* partial, uint8_t* ws,
           T* cols, const PeTail<T>& tail, hipStream_t st) {
    dim3 grid(GRID, n_img);
    if (mode == FMMT_RESIZE_PIL) {
        hipLaunchKernelGGL((jitter_stats_kernel<true, FMMT_AUG_WORDS, 8>), grid, dim3(256), 0, st, img, in_size, tab, aug, partial);
        hipLaunchKernelGGL((aug_pixels_kernel<true>), grid, dim3(256), 0, st, img, in_size, tab, aug, partial, ws);
    } else {
        hipLaunchKernelGGL((jitter_stats_kernel<false, FMMT_AUG_WORDS, 8>), grid, dim3(256), 0, st, img, in_size, tab, aug, partial);
        hipLaunchKernelGGL((aug_pixels_kernel<false>), grid, dim3(256), 0, st, img, in_size, tab, aug, partial, ws);
    }
    hipLaunchKernelGGL((aug_finish_kernel<T, FUSE>), grid, dim3(256), 0, st, ws, lut, aug, cols, tail);
    FMMT_CHECK_LAUNCH();
    return 0;
}

int check_common(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev, const float* lut_dev, const int32_t* aug_dev,
                 const int32_t* partial, const void* ws, size_t ws_bytes) {
    if ((dtype != FMMT_BF16 && dtype != FMMT_F32) || (mode != FMMT_RESIZE_PIL && mode != FMMT_RESIZE_CV2)) return FMMT_EINVAL;
    if (n_img <= 0 || n_img > 65535 || in_size < 4 || in_size > SMAX || !img_u8 || !table_dev || !lut_dev || !aug_dev || !partial || !ws) return FMMT_EINVAL;
    if (ws_bytes < fmmt_aug_workspace_bytes(n_img)) return FMMT_EWORKSPACE;
    if ((reinterpret_cast<uintptr_t>(table_dev) | reinterpret_cast<uintptr_t>(ws)) & 15) return FMMT_EALIGN;
    if ((reinterpret_cast<uintptr_t>(aug_dev) | reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(lut_dev)) & 3) return FMMT_EALIGN;
    return 0;
}

}  // namespace

extern "C" size_t fmmt_aug_workspace_bytes(int n_img) { return n_img > 0 ? (size_t)n_img * NPIX * 3 : 0; }

extern "C" int fmmt_aug_table_check(const int32_t* table, int n_img) {
    if (!table || n_img <= 0) return FMMT_EINVAL;
    for (int i = 0; i < n_img; ++i) {
        const int32_t* r = table + (size_t)i * FMMT_AUG_WORDS;
        if (fmmt_jitter_table_check(r, 1) != 0) return FMMT_EINVAL;
        if (r[8] & ~FMMT_AUG_FLAG_GRAY) return FMMT_EINVAL;
        if (r[9] < -1 || r[9] > FMMT_AUG_MAX_RADIUS) return FMMT_EINVAL;
        if (r[9] >= 0) {
            const int64_t rest = ((int64_t)1 << 24) - (int64_t)(2 * r[9] + 1) * r[10];
            if (r[10] <= 0 || rest < 0 || r[11] != rest / 2) return FMMT_EINVAL;
        }
        if (r[14] != 0) {
            if (r[14] < 1 || r[14] >= OUT || r[15] < 1 || r[15] >= OUT) return FMMT_EINVAL;
            if (r[12] < 0 || r[13] < 0 || r[12] + r[14] > OUT || r[13] + r[15] > OUT) return FMMT_EINVAL;
        }
        if (r[18] != 0 || r[19] != 0) return FMMT_EINVAL;
    }
    return 0;
}

extern "C" int fmmt_patch_embed_u8_aug(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev, const float* lut_dev,
                                       const int32_t* aug_dev, int32_t* partial, void* frames_ws, size_t ws_bytes, void* cols, void* stream) {
    if (const int rc = check_common(dtype, mode, n_img, in_size, img_u8, table_dev, lut_dev, aug_dev, partial, frames_ws, ws_bytes)) return rc;
    if (!cols) return FMMT_EINVAL;
    if (reinterpret_cast<uintptr_t>(cols) & 15) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t* img = reinterpret_cast<const uint8_t*>(img_u8);
    uint8_t* ws = reinterpret_cast<uint8_t*>(frames_ws);
    if (dtype == FMMT_BF16) return launch<bf16, false>(mode, n_img, in_size, img, table_dev, lut_dev, aug_dev, partial, ws, (bf16*)cols, PeTail<bf16>{}, st);
    return launch<float, false>(mode, n_img, in_size, img, table_dev, lut_dev, aug_dev, partial, ws, (float*)cols, PeTail<float>{}, st);
}

extern "C" int fmmt_patch_embed_u8_aug_ln_fwd(int dtype, int mode, int n_img, int in_size, const void* img_u8, const int32_t* table_dev,
                                              const float* lut_dev, const int32_t* aug_dev, int32_t* partial, void* frames_ws, size_t ws_bytes,
                                              const void* w, const float* bias, const float* ln_gamma, const float* ln_beta, float eps, void* cols,
                                              void* x_pre, void* y, float* mean, float* rstd, void* stream) {
    if (!w || !ln_gamma || !ln_beta || !y || (mean == nullptr) != (rstd == nullptr)) return FMMT_EINVAL;
    if (const int rc = check_common(dtype, mode, n_img, in_size, img_u8, table_dev, lut_dev, aug_dev, partial, frames_ws, ws_bytes)) return rc;
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!al16(w) || !al16(y) || (x_pre && !al16(x_pre)) || (cols && !al16(cols)) || (bias && !al16(bias)) || !al16(ln_gamma) || !al16(ln_beta)) return FMMT_EALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t* img = reinterpret_cast<const uint8_t*>(img_u8);
    uint8_t* ws = reinterpret_cast<uint8_t*>(frames_ws);
    if (dtype == FMMT_BF16) {
        const PeTail<bf16> t{(const bf16*)w, bias, ln_gamma, ln_beta, eps, (bf16*)x_pre, (bf16*)y, mean, rstd};
        return launch<bf16, true>(mode, n_img, in_size, img, table_dev, lut_dev, aug_dev, partial, ws, (bf16*)cols, t, st);
    }
    const PeTail<float> t{(const float*)w, bias, ln_gamma, ln_beta, eps, (float*)x_pre, (float*)y, mean, rstd};
    return launch<float, true>(mode, n_img, in_size, img, table_dev, lut_dev, aug_dev, partial, ws, (float*)cols, t, st);
}
