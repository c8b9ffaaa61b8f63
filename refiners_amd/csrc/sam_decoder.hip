// SegmentAnything mask decoder (src/refiners/foundationals/segment_anything/mask_decoder.py, transformer.py, utils.py): the
// launches no GEMM / LayerNorm epilogue covers -- attention with 16- and 32-wide heads over short key or short query sets, the
// LayerNorm2d + GELU + 2x scatter after the first transposed convolution, the fused second transposed convolution + GELU +
// hypernetwork contraction, and the two bilinear resizes of postprocess_masks.  Token-major layouts, float32 arithmetic,
// float32 or bfloat16 storage; every output is written by exactly one lane (no atomics: replays are bit-equal).
#include "common.cuh"
#include "../../include/mi355x_refiners.h"
#include "sam_mask_head.cuh"

namespace {

inline int blocks_for(int64_t work, int per_block = 256, int cap = 8192) {
    int64_t b = (work + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

#define SAM_LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)
#define SAM_DISPATCH(dtype, CALL)        \
    do {                                 \
        if ((dtype) == MI355X_F32) {     \
            using T = float;             \
            CALL;                        \
        } else if ((dtype) == MI355X_BF16) { \
            using T = bf16_t;            \
            CALL;                        \
        } else {                         \
            return MI355X_EDTYPE;        \
        }                                \
    } while (0)

constexpr int SAM_KEY_CHUNK = 256;  // keys per workgroup of the split (short-query) regime

MI_DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
MI_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------------- attention, Lk <= 64
// grid (ceil(Lq / 256), H, B): all keys / values of one (sample, head) in LDS, one query per lane, scores in registers
template <typename T, int D>
__global__ __launch_bounds__(256) void sam_attn_short_keys(mi355x_sam_attn_args a) {
    __shared__ float ks[64][D + 1];
    __shared__ float vs[64][D + 1];
    const int h = blockIdx.y, b = blockIdx.z;
    const T* k = static_cast<const T*>(a.k) + (int64_t)b * a.k_batch_stride + h * D;
    const T* v = static_cast<const T*>(a.v) + (int64_t)b * a.v_batch_stride + h * D;
    for (int i = threadIdx.x; i < a.Lk * D; i += 256) {
        const int j = i / D, d = i % D;
        ks[j][d] = to_f32(k[(int64_t)j * a.ldk + d]);
        vs[j][d] = to_f32(v[(int64_t)j * a.ldv + d]);
    }
    __syncthreads();
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= a.Lq) return;
    const T* q = static_cast<const T*>(a.q) + (int64_t)b * a.q_batch_stride + (int64_t)qi * a.ldq + h * D;
    float qv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) qv[d] = to_f32(q[d]) * a.scale;
    float s[64];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        float acc = 0.f;
        if (j < a.Lk) {
#pragma unroll
            for (int d = 0; d < D; ++d) acc += qv[d] * ks[j][d];
            mx = fmaxf(mx, acc);
        }
        s[j] = acc;
    }
    float o[D];
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] = 0.f;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        if (j < a.Lk) {
            const float p = __expf(s[j] - mx);
            sum += p;
#pragma unroll
            for (int d = 0; d < D; ++d) o[d] += p * vs[j][d];
        }
    }
    const float inv = 1.f / sum;
    T* out = static_cast<T*>(a.out) + (int64_t)b * a.o_batch_stride + (int64_t)qi * a.ldo + h * D;
#pragma unroll
    for (int d = 0; d < D; ++d) out[d] = from_f32<T>(o[d] * inv);
}

// ---------------------------------------------------------------------------------------------------- attention, Lq <= 64
// pass 1, grid (nsplit, H, B): one chunk of SAM_KEY_CHUNK keys per workgroup, one query per wave at a time; writes the chunk's
// (max, sum, unnormalised output) to ws[((b H + h) nsplit + split) Lq + i][D + 2]
template <typename T, int D>
__global__ __launch_bounds__(256) void sam_attn_split_partial(mi355x_sam_attn_args a, int nsplit) {
    __shared__ float ks[SAM_KEY_CHUNK][D + 1];
    __shared__ float vs[SAM_KEY_CHUNK][D + 1];
    __shared__ float ps[4][SAM_KEY_CHUNK];
    __shared__ float qs[4][D];
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int j0 = split * SAM_KEY_CHUNK;
    const int nk = min(SAM_KEY_CHUNK, a.Lk - j0);
    const T* k = static_cast<const T*>(a.k) + (int64_t)b * a.k_batch_stride + (int64_t)j0 * a.ldk + h * D;
    const T* v = static_cast<const T*>(a.v) + (int64_t)b * a.v_batch_stride + (int64_t)j0 * a.ldv + h * D;
    for (int i = threadIdx.x; i < nk * D; i += 256) {
        const int j = i / D, d = i % D;
        ks[j][d] = to_f32(k[(int64_t)j * a.ldk + d]);
        vs[j][d] = to_f32(v[(int64_t)j * a.ldv + d]);
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int KPL = SAM_KEY_CHUNK / 64;  // keys per lane
    constexpr int G = 64 / D;                // lane groups of the output reduction
    for (int q0 = 0; q0 < a.Lq; q0 += 4) {  // the same trip count in every wave (barriers below); wave w takes query q0 + w
        const int qi = min(q0 + w, a.Lq - 1);
        const bool active = q0 + w < a.Lq;
        const T* q = static_cast<const T*>(a.q) + (int64_t)b * a.q_batch_stride + (int64_t)qi * a.ldq + h * D;
        if (lane < D) qs[w][lane] = to_f32(q[lane]) * a.scale;
        __syncthreads();
        float s[KPL];
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < KPL; ++c) {
            const int j = lane + 64 * c;
            float acc = -INFINITY;
            if (j < nk) {
                acc = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) acc += qs[w][d] * ks[j][d];
            }
            s[c] = acc;
            mx = fmaxf(mx, acc);
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < KPL; ++c) {
            const int j = lane + 64 * c;
            const float p = j < nk ? __expf(s[c] - mx) : 0.f;
            ps[w][j] = p;
            sum += p;
        }
        sum = wave_sum(sum);
        __syncthreads();
        const int d = lane % D, grp = lane / D;
        float o = 0.f;
        for (int j = grp; j < nk; j += G) o += ps[w][j] * vs[j][d];
#pragma unroll
        for (int off = D; off < 64; off <<= 1) o += __shfl_xor(o, off);
        float* dst = a.ws + ((((int64_t)b * a.H + h) * nsplit + split) * a.Lq + qi) * (D + 2);
        if (active && lane < D) dst[2 + lane] = o;
        if (active && lane == 0) {
            dst[0] = mx;
            dst[1] = sum;
        }
        __syncthreads();
    }
}

// pass 2: one lane per (b, h, query, d): the chunks combined in split order (deterministic)
template <typename T, int D>
__global__ __launch_bounds__(256) void sam_attn_split_combine(mi355x_sam_attn_args a, int nsplit) {
    const int64_t total = (int64_t)a.B * a.H * a.Lq * D;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int d = (int)(t % D);
        const int64_t r = t / D;  // (b, h, qi)
        const int qi = (int)(r % a.Lq);
        const int64_t bh = r / a.Lq;
        const int h = (int)(bh % a.H), b = (int)(bh / a.H);
        const float* src = a.ws + (bh * nsplit * a.Lq + qi) * (D + 2);
        const int64_t step = (int64_t)a.Lq * (D + 2);
        float m = -INFINITY;
        for (int s = 0; s < nsplit; ++s) m = fmaxf(m, src[s * step]);
        float l = 0.f, o = 0.f;
        for (int s = 0; s < nsplit; ++s) {
            const float f = __expf(src[s * step] - m);
            l += src[s * step + 1] * f;
            o += src[s * step + 2 + d] * f;
        }
        T* out = static_cast<T*>(a.out) + (int64_t)b * a.o_batch_stride + (int64_t)qi * a.ldo + h * D + d;
        *out = from_f32<T>(o / l);
    }
}

template <typename T, int D>
int sam_attention_launch(const mi355x_sam_attn_args& a, hipStream_t st) {
    if (a.Lk <= 64) {
        hipLaunchKernelGGL((sam_attn_short_keys<T, D>), dim3((a.Lq + 255) / 256, a.H, a.B), dim3(256), 0, st, a);
        return SAM_LAUNCH_OK();
    }
    const int nsplit = (a.Lk + SAM_KEY_CHUNK - 1) / SAM_KEY_CHUNK;
    if ((int64_t)a.B * a.H * nsplit * a.Lq * (D + 2) > a.ws_floats) return MI355X_EARG;
    hipLaunchKernelGGL((sam_attn_split_partial<T, D>), dim3(nsplit, a.H, a.B), dim3(256), 0, st, a, nsplit);
    hipLaunchKernelGGL((sam_attn_split_combine<T, D>), dim3(blocks_for((int64_t)a.B * a.H * a.Lq * D)), dim3(256), 0, st, a, nsplit);
    return SAM_LAUNCH_OK();
}

// ---------------------------------------------------------------------------------------------------- LayerNorm2d + GELU (+ 2x scatter)
// one lane per (item, channel); the C lanes of an item are consecutive, so the reductions are xor shuffles inside the segment
template <typename T>
__global__ __launch_bounds__(256) void sam_ln_gelu_kernel(const T* __restrict__ x, int64_t ldx, int64_t M, int C, int G, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, T* __restrict__ out, int64_t ldo, int Hs, int Ws) {
    const int64_t items = M * G;
    const int64_t lanes = items * C;  // C divides 64: every wave holds whole items
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < lanes; t0 += stride) {  // block-uniform trip count (shuffles below)
        const int64_t t = t0 + threadIdx.x;
        const bool ok = t < lanes;
        const int64_t item = ok ? t / C : 0;
        const int c = (int)(t % C);
        const int64_t m = item / G;
        const int g = (int)(item % G);
        const float xv = ok ? to_f32(x[m * ldx + (int64_t)g * C + c]) : 0.f;
        float s = xv;
        for (int o = 1; o < C; o <<= 1) s += __shfl_xor(s, o);
        const float mean = s / C;
        const float dv = xv - mean;
        float s2 = dv * dv;
        for (int o = 1; o < C; o <<= 1) s2 += __shfl_xor(s2, o);
        const float y = gelu_exact(dv * rsqrtf(s2 / C + eps) * gamma[c] + beta[c]);
        if (!ok) continue;
        if (Hs > 0) {  // row m = pixel (p, yy, xx) of an Hs x Ws grid, group g = (dy, dx): output pixel (p, 2 yy + dy, 2 xx + dx), channel c
            const int64_t p = m / ((int64_t)Hs * Ws);
            const int yy = (int)((m / Ws) % Hs), xx = (int)(m % Ws);
            const int64_t row = (p * 2 * Hs + 2 * yy + (g >> 1)) * (2 * Ws) + 2 * xx + (g & 1);
            out[row * ldo + c] = from_f32<T>(y);
        } else {
            out[m * ldo + (int64_t)g * C + c] = from_f32<T>(y);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- postprocess_masks
// PyTorch's bilinear source index (align_corners=False): src = max(scale (dst + 0.5) - 0.5, 0) with scale = in / out in float
struct Tap {
    int i0, i1;
    float l0, l1;
};
MI_DEV Tap bilinear_tap(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    float src = scale * (dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

template <typename T>
__global__ __launch_bounds__(256) void sam_postprocess_kernel(mi355x_sam_postprocess_args a) {
    const int64_t total = (int64_t)a.N * a.H * a.W;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int ox = (int)(t % a.W);
        const int oy = (int)((t / a.W) % a.H);
        const int64_t n = t / ((int64_t)a.W * a.H);
        const T* src = static_cast<const T*>(a.in) + n * a.in_plane_stride;
        // outer resize: (sh, sw) crop of the R x R upsampled mask -> (H, W); each of its taps is the inner resize (Hin, Win) -> (R, R)
        const Tap ty = bilinear_tap(oy, a.sh, a.H), tx = bilinear_tap(ox, a.sw, a.W);
        float v = 0.f;
#pragma unroll
        for (int iy = 0; iy < 2; ++iy) {
            const Tap sy = bilinear_tap(iy ? ty.i1 : ty.i0, a.Hin, a.R);
            float row = 0.f;
#pragma unroll
            for (int ix = 0; ix < 2; ++ix) {
                const Tap sx = bilinear_tap(ix ? tx.i1 : tx.i0, a.Win, a.R);
                const T* r0 = src + (int64_t)sy.i0 * a.Win;
                const T* r1 = src + (int64_t)sy.i1 * a.Win;
                const float inner = sy.l0 * (sx.l0 * to_f32(r0[sx.i0]) + sx.l1 * to_f32(r0[sx.i1])) + sy.l1 * (sx.l0 * to_f32(r1[sx.i0]) + sx.l1 * to_f32(r1[sx.i1]));
                row += (ix ? tx.l1 : tx.l0) * inner;
            }
            v += (iy ? ty.l1 : ty.l0) * row;
        }
        if (a.binarize) static_cast<uint8_t*>(a.out)[t] = v > a.threshold ? 1 : 0;
        else static_cast<T*>(a.out)[t] = from_f32<T>(v);
    }
}

}  // namespace

extern "C" int mi355x_sam_attention(const mi355x_sam_attn_args* a, void* stream) {
    if (!a || !a->q || !a->k || !a->v || !a->out || a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->Lk <= 0) return MI355X_EARG;
    if (a->D != 16 && a->D != 32) return MI355X_ESHAPE;
    if (a->Lk > 64 && (a->Lq > 64 || !a->ws)) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->dtype == MI355X_F32) return a->D == 16 ? sam_attention_launch<float, 16>(*a, st) : sam_attention_launch<float, 32>(*a, st);
    if (a->dtype == MI355X_BF16) return a->D == 16 ? sam_attention_launch<bf16_t, 16>(*a, st) : sam_attention_launch<bf16_t, 32>(*a, st);
    return MI355X_EDTYPE;
}

extern "C" int mi355x_convt2x2_ln_gelu(int32_t dtype, const void* x, int64_t ldx, int64_t M, int32_t C, int32_t G, const float* gamma, const float* beta,
                                       float eps, void* out, int64_t ldo, int32_t Hs, int32_t Ws, void* stream) {
    if (!x || !out || !gamma || !beta || M <= 0 || C <= 0 || G <= 0 || Hs < 0 || Ws < 0) return MI355X_EARG;
    if (C > 64 || (64 % C) || (Hs > 0 && (G != 4 || M % ((int64_t)Hs * Ws)))) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SAM_DISPATCH(dtype, hipLaunchKernelGGL((sam_ln_gelu_kernel<T>), dim3(blocks_for(M * G * C)), dim3(256), 0, st, static_cast<const T*>(x), ldx, M, C, G,
                                           gamma, beta, eps, static_cast<T*>(out), ldo, Hs, Ws));
    return SAM_LAUNCH_OK();
}

extern "C" int mi355x_sam_mask_head(const mi355x_sam_mask_head_args* a, void* stream) {
    if (!a || !a->x || !a->w || !a->bias || !a->hyper || !a->out || a->P <= 0 || a->Hin <= 0 || a->Win <= 0) return MI355X_EARG;
    if (a->nk < 1 || a->nk > 4 || (reinterpret_cast<uintptr_t>(a->w) & 15)) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntiles = (int64_t)a->P * ((a->Hin * a->Win + 63) / 64);
    SAM_DISPATCH(a->dtype, hipLaunchKernelGGL((sam_mask_head_kernel<T, false>), dim3((int)(ntiles < 2048 ? ntiles : 2048)), dim3(256), 0, st, *a, nullptr, (int64_t)0));
    return SAM_LAUNCH_OK();
}

extern "C" int mi355x_sam_postprocess_masks(const mi355x_sam_postprocess_args* a, void* stream) {
    if (!a || !a->in || !a->out || a->N <= 0 || a->Hin <= 0 || a->Win <= 0 || a->R <= 0 || a->H <= 0 || a->W <= 0) return MI355X_EARG;
    if (a->sh <= 0 || a->sw <= 0 || a->sh > a->R || a->sw > a->R) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SAM_DISPATCH(a->dtype, hipLaunchKernelGGL((sam_postprocess_kernel<T>), dim3(blocks_for((int64_t)a->N * a->H * a->W)), dim3(256), 0, st, *a));
    return SAM_LAUNCH_OK();
}
