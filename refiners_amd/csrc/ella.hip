// ELLA's timestep-aware text connector (foundationals/latent_diffusion/ella_adapter.py of the reference): the one streaming pass its
// Perceiver resampler needs beside the library's GEMM, attention and LayerNorm launches.
//   ella_adaln  Distribute(AdaLayerNorm, AdaLayerNorm) + to_kv = cat(latents_n, x_n) as ONE launch that writes the packed [B][Lp][C] rows the
//               Q|K|V^T GEMM reads (latent rows, text rows, zero rows up to the attention kernel's 64-key blocks); T = 0 is the feed-forward's.
// HBM-bound, float32 arithmetic, one wave per row with the row in registers (two-pass mean / variance like layernorm_kernel of norm.hip),
// 16-byte loads and stores, no LDS, no atomics: replays are bit-equal.
#include "common.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_ella.h"

namespace {

// bytes spanned by B batch rows of `rows` rows of C elements
inline int64_t span(int64_t B, int64_t bs, int64_t rows, int64_t ld, int C, int es) { return ((B - 1) * bs + (rows - 1) * ld + C) * es; }

struct AdaLnP {
    const void *latents, *x, *shift_l, *scale_l, *shift_x, *scale_x;
    void* out;
    int64_t ldl, lbs, ldx, xbs, mbs, ldo, obs;
    int B, Nl, T, Lp, C;
    float eps;
};

template <typename T, int MAXV>
__global__ __launch_bounds__(256) void ella_adaln_kernel(AdaLnP p) {
    constexpr int EPC = DT<T>::EPC;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wid;  // wave-uniform
    if (row >= (int64_t)p.B * p.Lp) return;
    const int b = (int)(row / p.Lp), r = (int)(row % p.Lp);
    const int nvec = p.C / EPC;
    T* op = static_cast<T*>(p.out) + (int64_t)b * p.obs + (int64_t)r * p.ldo;
    if (r >= p.Nl + p.T) {  // padding rows: exact zeros, whatever the buffer held
        Vec16<T> z;
#pragma unroll
        for (int e = 0; e < EPC; ++e) z.set(e, 0.f);
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int vi = lane + 64 * k;
            if (vi < nvec) store16<T>(op + vi * EPC, z);
        }
        return;
    }
    const bool lat = r < p.Nl;
    const T* xp = lat ? static_cast<const T*>(p.latents) + (int64_t)b * p.lbs + (int64_t)r * p.ldl
                      : static_cast<const T*>(p.x) + (int64_t)b * p.xbs + (int64_t)(r - p.Nl) * p.ldx;
    const T* sh = static_cast<const T*>(lat ? p.shift_l : p.shift_x) + (int64_t)b * p.mbs;
    const T* sc = static_cast<const T*>(lat ? p.scale_l : p.scale_x) + (int64_t)b * p.mbs;
    float v[MAXV][EPC];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        const int vi = lane + 64 * k;
        if (vi < nvec) {
            const Vec16<T> t = load16<T>(xp + vi * EPC);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                v[k][e] = t.get(e);
                s += v[k][e];
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    const float mean = s / (float)p.C;
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        const int vi = lane + 64 * k;
        if (vi < nvec) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const float d = v[k][e] - mean;
                ss += d * d;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
    const float rstd = rsqrtf(ss / (float)p.C + p.eps);
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        const int vi = lane + 64 * k;
        if (vi < nvec) {
            const Vec16<T> a = load16<T>(sc + vi * EPC), c = load16<T>(sh + vi * EPC);
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, (v[k][e] - mean) * rstd * (1.0f + a.get(e)) + c.get(e));
            store16<T>(op + vi * EPC, o);
        }
    }
}

template <typename T>
int run_adaln(const AdaLnP& p, hipStream_t st) {
    const int nvec = p.C / DT<T>::EPC;
    const dim3 grid((unsigned)(((int64_t)p.B * p.Lp + 3) / 4)), block(256);
    if (nvec <= 64) hipLaunchKernelGGL((ella_adaln_kernel<T, 1>), grid, block, 0, st, p);
    else if (nvec <= 128) hipLaunchKernelGGL((ella_adaln_kernel<T, 2>), grid, block, 0, st, p);
    else if (nvec <= 256) hipLaunchKernelGGL((ella_adaln_kernel<T, 4>), grid, block, 0, st, p);
    else if (nvec <= 512) hipLaunchKernelGGL((ella_adaln_kernel<T, 8>), grid, block, 0, st, p);
    else if (nvec <= 1024) hipLaunchKernelGGL((ella_adaln_kernel<T, 16>), grid, block, 0, st, p);
    else return MI355X_ESHAPE;
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

}  // namespace

extern "C" int mi355x_ella_adaln(const mi355x_ella_adaln_args* a, void* stream) {
    if (!a || !a->latents || !a->shift_l || !a->scale_l || !a->out) return MI355X_EARG;
    if (a->T > 0 && (!a->x || !a->shift_x || !a->scale_x)) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B < 1 || a->Nl < 1 || a->T < 0 || a->C < 1 || a->C > 4096 || (int64_t)a->Lp < (int64_t)a->Nl + a->T) return MI355X_ESHAPE;
    if ((a->C * es) % 16 || (a->ldl * es) % 16 || (a->l_batch_stride * es) % 16 || (a->ldo * es) % 16 || (a->out_batch_stride * es) % 16 || (a->mod_batch_stride * es) % 16)
        return MI355X_ESHAPE;
    if (a->ldl < a->C || a->ldo < a->C || a->mod_batch_stride < 0 || a->l_batch_stride < 0) return MI355X_ESHAPE;
    if (a->B > 1 && a->out_batch_stride < (int64_t)(a->Lp - 1) * a->ldo + a->C) return MI355X_ESHAPE;
    if (!al16(a->latents) || !al16(a->shift_l) || !al16(a->scale_l) || !al16(a->out)) return MI355X_ESHAPE;
    if (a->T > 0) {
        if ((a->ldx * es) % 16 || (a->x_batch_stride * es) % 16 || a->ldx < a->C || a->x_batch_stride < 0) return MI355X_ESHAPE;
        if (!al16(a->x) || !al16(a->shift_x) || !al16(a->scale_x)) return MI355X_ESHAPE;
    }
    const int64_t obytes = span(a->B, a->out_batch_stride, a->Lp, a->ldo, a->C, es);
    if (overlap(a->latents, span(a->B, a->l_batch_stride, a->Nl, a->ldl, a->C, es), a->out, obytes)) return MI355X_EARG;
    if (a->T > 0 && overlap(a->x, span(a->B, a->x_batch_stride, a->T, a->ldx, a->C, es), a->out, obytes)) return MI355X_EARG;
    AdaLnP p;
    p.latents = a->latents, p.x = a->T > 0 ? a->x : nullptr, p.shift_l = a->shift_l, p.scale_l = a->scale_l;
    p.shift_x = a->T > 0 ? a->shift_x : nullptr, p.scale_x = a->T > 0 ? a->scale_x : nullptr, p.out = a->out;
    p.ldl = a->ldl, p.lbs = a->l_batch_stride, p.ldx = a->ldx, p.xbs = a->x_batch_stride, p.mbs = a->mod_batch_stride, p.ldo = a->ldo, p.obs = a->out_batch_stride;
    p.B = a->B, p.Nl = a->Nl, p.T = a->T, p.Lp = a->Lp, p.C = a->C, p.eps = a->eps;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return a->dtype == MI355X_F32 ? run_adaln<float>(p, st) : run_adaln<bf16_t>(p, st);
}
