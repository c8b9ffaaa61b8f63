// HQ-SAM mask prediction (src/refiners/foundationals/segment_anything/hq_sam.py:16-167): the folded 3x3 mask head, the mask head that
// also stores the upscaled dense embedding, and LayerNorm2d + GELU + 2x scatter at 128 / 256 channels.  float32 arithmetic, float32 or
// bfloat16 storage; every output is written by exactly one lane (no atomics: replays are bit-equal).
#include "common.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_sam_hq.h"
#include "sam_mask_head.cuh"

namespace {

#define HQ_LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)

// 4 consecutive elements as float32 (16-byte load for float, 8-byte for bfloat16)
MI_DEV f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
MI_DEV f32x4 load4(const bf16_t* p) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// ---------------------------------------------------------------------------------------------------- folded HQ mask head
constexpr int HQ_TW = 16, HQ_TH = 8;                     // output pixels of one tile: two lanes per pixel, 32 channels each
constexpr int HQ_HW = HQ_TW + 2, HQ_HH = HQ_TH + 2;      // the tile with its one-pixel halo
constexpr int HQ_NPIX = HQ_HW * HQ_HH;                   // 180
constexpr int HQ_ROW = 68;                               // floats per LDS pixel row: 64 + one 16-byte slot, so that consecutive pixels start one slot apart

// grid (tiles of a prompt taken round-robin, P).  Prologue: weff[tap][ci] = sum_c h[c] w2[c][tap][ci] and hb = h . b2 into LDS.  Per tile:
// 16 lanes per halo pixel stage z = GELU(LayerNorm2d(y)) (0 outside the image) into LDS, then lane (pixel, half) sums its 9 x 32 products
// and its 16 channels of h . F; the two halves of a pixel meet in one shuffle.
template <typename T>
__global__ __launch_bounds__(256) void sam_hq_mask_head_kernel(mi355x_sam_hq_mask_head_args a) {
    __shared__ __attribute__((aligned(16))) float zs[HQ_NPIX * HQ_ROW];
    __shared__ __attribute__((aligned(16))) float weff[9 * 64];
    __shared__ float hs[32];
    __shared__ float hb;
    const int tid = threadIdx.x, p = blockIdx.y;
    const int H = a.H, W = a.W;
    const T* hv = static_cast<const T*>(a.h) + (int64_t)p * a.h_stride;
    if (tid < 32) hs[tid] = to_f32(hv[tid]);
    __syncthreads();
    if (tid < 144) {  // four consecutive (tap, ci) entries per lane
        const f32x4* w4 = reinterpret_cast<const f32x4*>(a.w2) + tid;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < 32; ++c) acc += hs[c] * w4[c * 144];
        reinterpret_cast<f32x4*>(weff)[tid] = acc;
    } else if (tid == 144) {
        float s = 0.f;
        for (int c = 0; c < 32; ++c) s += hs[c] * a.b2[c];
        hb = s;
    }
    const int l16 = tid & 15;
    float g[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        g[j] = a.gamma[4 * l16 + j];
        b[j] = a.beta[4 * l16 + j];
    }
    const int tiles_x = (W + HQ_TW - 1) / HQ_TW, tiles_y = (H + HQ_TH - 1) / HQ_TH;
    const int ntiles = tiles_x * tiles_y;
    const T* yb = static_cast<const T*>(a.y) + (int64_t)p * H * W * a.ldy;
    const T* fq = static_cast<const T*>(a.fq);
    T* ob = static_cast<T*>(a.out) + (int64_t)p * a.out_batch_stride;
    const int pi = tid >> 1, half = tid & 1, px = pi & (HQ_TW - 1), py = pi / HQ_TW;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * HQ_TH, tx0 = (tile % tiles_x) * HQ_TW;
        __syncthreads();  // the previous tile's readers are done with zs (first tile: weff and hb are written)
        for (int i0 = 0; i0 < HQ_NPIX; i0 += 16) {  // block-uniform trip count (shuffles below): 16 halo pixels per pass
            const int i = i0 + (tid >> 4);
            const int hy = i / HQ_HW, hx = i - hy * HQ_HW;
            const int gy = ty0 + hy - 1, gx = tx0 + hx - 1;
            const bool ok = i < HQ_NPIX && gy >= 0 && gy < H && gx >= 0 && gx < W;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = load4(yb + ((int64_t)gy * W + gx) * a.ldy + 4 * l16);
            float s = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
            const float mean = s * (1.f / 64.f);
            const f32x4 d = v - mean;
            float s2 = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) s2 += __shfl_xor(s2, o);
            const float rstd = rsqrtf(s2 * (1.f / 64.f) + a.eps);
            f32x4 z;
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = ok ? gelu_exact(d[j] * rstd * g[j] + b[j]) : 0.f;  // zero padding of the ACTIVATED tensor
            if (i < HQ_NPIX) *reinterpret_cast<f32x4*>(&zs[i * HQ_ROW + 4 * l16]) = z;
        }
        __syncthreads();
        float acc = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const f32x4* zr = reinterpret_cast<const f32x4*>(&zs[((py + tap / 3) * HQ_HW + px + tap % 3) * HQ_ROW + half * 32]);
            const f32x4* wr = reinterpret_cast<const f32x4*>(&weff[tap * 64 + half * 32]);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const f32x4 zv = zr[k], wv = wr[k];
                acc += zv[0] * wv[0];
                acc += zv[1] * wv[1];
                acc += zv[2] * wv[2];
                acc += zv[3] * wv[3];
            }
        }
        const int gy = ty0 + py, gx = tx0 + px;
        const bool valid = gy < H && gx < W;
        if (valid) {
            const T* fr = fq + ((int64_t)(gy >> 1) * (W >> 1) + (gx >> 1)) * a.ldf + ((gy & 1) * 2 + (gx & 1)) * 32 + half * 16;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 fv = load4(fr + 4 * k);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += hs[half * 16 + 4 * k + j] * fv[j];
            }
        }
        acc += __shfl_xor(acc, 1);
        if (valid && half == 0) ob[(int64_t)gy * W + gx] = from_f32<T>(acc + hb);
    }
}

// ---------------------------------------------------------------------------------------------------- LayerNorm2d + GELU + 2x scatter, C = 64 VPL
// one wave per (row m, group g): lane owns channels VPL lane .. VPL lane + VPL - 1
template <typename T, int VPL>
__global__ __launch_bounds__(256) void ln2d_gelu_wide_kernel(const T* __restrict__ x, int64_t ldx, int64_t M, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, T* __restrict__ out, int64_t ldo, int Hs, int Ws) {
    constexpr int C = 64 * VPL;
    const int lane = threadIdx.x & 63;
    const int64_t items = M * 4;
    float g[VPL], b[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        g[j] = gamma[VPL * lane + j];
        b[j] = beta[VPL * lane + j];
    }
    for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += (int64_t)gridDim.x * 4) {  // wave-uniform
        const int64_t m = item >> 2;
        const int grp = (int)(item & 3);
        const T* xr = x + m * ldx + (int64_t)grp * C + VPL * lane;
        float v[VPL];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            v[j] = to_f32(xr[j]);
            s += v[j];
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
        const float mean = s * (1.f / C);
        float s2 = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            v[j] -= mean;
            s2 += v[j] * v[j];
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) s2 += __shfl_xor(s2, o);
        const float rstd = rsqrtf(s2 * (1.f / C) + eps);
        const int64_t p = m / ((int64_t)Hs * Ws);
        const int yy = (int)((m / Ws) % Hs), xx = (int)(m % Ws);
        const int64_t row = (p * 2 * Hs + 2 * yy + (grp >> 1)) * (2 * Ws) + 2 * xx + (grp & 1);
        T* orow = out + row * ldo + VPL * lane;
#pragma unroll
        for (int j = 0; j < VPL; ++j) orow[j] = from_f32<T>(gelu_exact(v[j] * rstd * g[j] + b[j]));
    }
}

inline bool aligned_to(const void* p, int64_t ld_elems, int dtype, int elems) {  // pointer and leading dimension on `elems` elements
    const int64_t bytes = (int64_t)elems * (dtype == MI355X_F32 ? 4 : 2);
    return (reinterpret_cast<uintptr_t>(p) % bytes) == 0 && ld_elems % elems == 0;
}

}  // namespace

extern "C" int mi355x_sam_hq_mask_head(const mi355x_sam_hq_mask_head_args* a, void* stream) {
    if (!a || !a->y || !a->gamma || !a->beta || !a->w2 || !a->b2 || !a->h || !a->fq || !a->out || a->P <= 0 || a->H <= 0 || a->W <= 0) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if ((a->H & 1) || (a->W & 1) || a->ldy < 64 || a->ldf < 128 || (reinterpret_cast<uintptr_t>(a->w2) & 15)) return MI355X_ESHAPE;
    if (!aligned_to(a->y, a->ldy, a->dtype, 4) || !aligned_to(a->fq, a->ldf, a->dtype, 4) || a->P > 65535) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ntiles = ((a->W + HQ_TW - 1) / HQ_TW) * ((a->H + HQ_TH - 1) / HQ_TH);
    int per_prompt = 1024 / a->P;  // about four workgroups per compute unit in all; each folds weff once and walks its share of the tiles
    per_prompt = per_prompt < 8 ? 8 : per_prompt;
    per_prompt = per_prompt > ntiles ? ntiles : per_prompt;
    const dim3 grid(per_prompt, a->P);
    if (a->dtype == MI355X_F32) hipLaunchKernelGGL((sam_hq_mask_head_kernel<float>), grid, dim3(256), 0, st, *a);
    else hipLaunchKernelGGL((sam_hq_mask_head_kernel<bf16_t>), grid, dim3(256), 0, st, *a);
    return HQ_LAUNCH_OK();
}

extern "C" int mi355x_sam_mask_head_up(const mi355x_sam_mask_head_up_args* a, void* stream) {
    if (!a || !a->x || !a->w || !a->bias || !a->hyper || !a->out || !a->u || a->P <= 0 || a->Hin <= 0 || a->Win <= 0) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->nk < 1 || a->nk > 4 || (reinterpret_cast<uintptr_t>(a->w) & 15)) return MI355X_ESHAPE;
    if (a->ldu < 32 || !aligned_to(a->u, a->ldu, a->dtype, a->dtype == MI355X_F32 ? 4 : 8)) return MI355X_ESHAPE;
    mi355x_sam_mask_head_args b;
    b.dtype = a->dtype;
    b.P = a->P, b.Hin = a->Hin, b.Win = a->Win, b.nk = a->nk;
    b.x = a->x, b.ldx = a->ldx, b.w = a->w, b.bias = a->bias;
    b.hyper = a->hyper, b.ld_hyper = a->ld_hyper, b.hyper_batch_stride = a->hyper_batch_stride;
    b.out = a->out, b.out_batch_stride = a->out_batch_stride;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntiles = (int64_t)a->P * ((a->Hin * a->Win + 63) / 64);
    const dim3 grid((int)(ntiles < 2048 ? ntiles : 2048));
    if (a->dtype == MI355X_F32) hipLaunchKernelGGL((sam_mask_head_kernel<float, true>), grid, dim3(256), 0, st, b, static_cast<float*>(a->u), a->ldu);
    else hipLaunchKernelGGL((sam_mask_head_kernel<bf16_t, true>), grid, dim3(256), 0, st, b, static_cast<bf16_t*>(a->u), a->ldu);
    return HQ_LAUNCH_OK();
}

extern "C" int mi355x_ln2d_gelu_wide(int32_t dtype, const void* x, int64_t ldx, int64_t M, int32_t C, const float* gamma, const float* beta, float eps,
                                     void* out, int64_t ldo, int32_t Hs, int32_t Ws, void* stream) {
    if (!x || !out || !gamma || !beta || M <= 0) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    if ((C != 128 && C != 256) || Hs <= 0 || Ws <= 0 || M % ((int64_t)Hs * Ws) || ldx < 4 * (int64_t)C || ldo < C) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t blocks = M;  // four waves = the four groups of one row
    const dim3 grid((int)(blocks < 8192 ? blocks : 8192));
#define HQ_LN(T, VPL) hipLaunchKernelGGL((ln2d_gelu_wide_kernel<T, VPL>), grid, dim3(256), 0, st, static_cast<const T*>(x), ldx, M, gamma, beta, eps, static_cast<T*>(out), ldo, Hs, Ws)
    if (dtype == MI355X_F32) {
        if (C == 128) HQ_LN(float, 2);
        else HQ_LN(float, 4);
    } else {
        if (C == 128) HQ_LN(bf16_t, 2);
        else HQ_LN(bf16_t, 4);
    }
#undef HQ_LN
    return HQ_LAUNCH_OK();
}
