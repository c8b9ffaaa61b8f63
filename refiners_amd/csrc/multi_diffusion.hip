// MultiDiffusion (latent_diffusion/multi_diffusion.py:98-123 of the reference): the three streaming passes around the UNet launches of a tiled step.
//   md_gather       T tiles of one size cut from the canvas (or noised init latents) -> the solver's views [T, C, h, w] and the CFG batch [2T, C, h, w]
//   md_target_step  guidance + solver update with one coefficient row PER TARGET (mi355x_cfg_ddim_step / mi355x_cfg_linear_step take one per batch)
//   md_blend        the canvas update in gather form: one thread per canvas element walks the targets in list order
// All HBM-bound.  A tile's left edge and the canvas width are arbitrary, so a tile row starts at any element: the canvas side of gather and the tile
// side of blend are read element-wise (consecutive lanes still read consecutive addresses), the contiguous side moves as 4-element vectors where
// the row length allows.  float32 arithmetic, one rounding at the store.  No float atomics: blend sums in target order, replays are bit-equal.
// The sums of gather's add_noise form and of blend are single-rounding operations (no fused multiply-add: contraction is off in this file), which is
// what torch's separate mul / add kernels compute: in float32 both passes give the reference's bits.
#include "common.cuh"
#include "solver_update.cuh"
#include "../../include/mi355x_refiners.h"

// every product and sum below is rounded on its own unless it is written as fmaf(): the float32 results are compared bit for bit with torch's
#pragma clang fp contract(off)

namespace {

// Single-rounding product / sum / quotient.  Defined HERE, under the pragma: the runtime header's __fmul_rn / __fadd_rn are compiled under the
// header's own contraction mode, and once inlined their product and sum are fused into one fma (seen in the 4-wide blend: 1 ulp off torch).
MI_DEV float mul_rn(float a, float b) { return a * b; }
MI_DEV float add_rn(float a, float b) { return a + b; }
MI_DEV float div_rn(float a, float b) { return a / b; }

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)

inline int grid_for(int64_t work, int cap = 4096) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <typename T> struct Q4;  // four consecutive elements: 16 bytes of float32, 8 of bfloat16
template <> struct Q4<float> { typedef f32x4 V; };
template <> struct Q4<bf16_t> { typedef bf16x4 V; };

template <typename T, int VEC> MI_DEV void load_n(const T* p, T (&r)[VEC]) {
    if constexpr (VEC == 4) {
        const typename Q4<T>::V v = *reinterpret_cast<const typename Q4<T>::V*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = v[e];
    } else {
        r[0] = p[0];
    }
}
template <typename T, int VEC> MI_DEV void store_n(T* p, const T (&r)[VEC]) {
    if constexpr (VEC == 4) {
        typename Q4<T>::V v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = r[e];
        *reinterpret_cast<typename Q4<T>::V*>(p) = v;
    } else {
        p[0] = r[0];
    }
}

// grid (blocks, T).  VEC = 4: w % 4 == 0, a thread owns four consecutive columns of one tile row; the source row starts anywhere, so it is read by element.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void md_gather_kernel(const T* __restrict__ canvas, const T* __restrict__ noise, const T* __restrict__ init,
                                                         const mi355x_md_gather_desc* __restrict__ desc, T* __restrict__ view, T* __restrict__ model_in,
                                                         int nt, int C, int h, int w, int H, int W, int n_init) {
    const int t = blockIdx.y;
    const mi355x_md_gather_desc d = desc[t];
    // the host validated its copy of the rows; a device row that left the contract since (a replay with new values) moves nothing
    if (d.top < 0 || d.left < 0 || d.top > H - h || d.left > W - w) return;
    const bool noised = d.kind == MI355X_MD_SRC_INIT;
    if (noised && (!init || !noise || d.init_row < 0 || d.init_row >= n_init)) return;
    const int64_t n = (int64_t)C * h * w;
    const T* ini = noised ? init + (int64_t)d.init_row * n : nullptr;
    T* vo = view + (int64_t)t * n;
    T* mu = model_in + (int64_t)t * n;
    T* mc = model_in + (int64_t)(nt + t) * n;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n / VEC; q += (int64_t)gridDim.x * 256) {
        const int64_t i = q * VEC;
        const int c = (int)(i / (h * w));
        const int r = (int)(i - (int64_t)c * h * w);
        const int y = r / w, x = r - y * w;
        const int64_t src = ((int64_t)c * H + d.top + y) * W + d.left + x;
        T v[VEC], m[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (noised)  // Solver.add_noise (solvers/solver.py:244-266): scale * x + std * noise, two products and a sum
                v[e] = from_f32<T>(add_rn(mul_rn(d.a, to_f32(ini[i + e])), mul_rn(d.b, to_f32(noise[src + e]))));
            else
                v[e] = canvas[src + e];
            m[e] = from_f32<T>(d.s * to_f32(v[e]));  // Solver.scale_model_input on the STORED view, as mi355x_cfg_linear_step scales the stored latents
        }
        store_n<T, VEC>(vo + i, v);
        store_n<T, VEC>(mu + i, m);
        store_n<T, VEC>(mc + i, m);
    }
}

// grid (blocks, T).  coef + 8 t: {cfg, sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)} (LINEAR == false) or {cfg, hx, he, kx, ke, kd, kp, -}.
// One element is the guided step_elem of the batch kernel (solver_update.cuh, solver_step.hip), so a target under its own coefficient row gets the bits
// the batch gets (tests/test_multi_diffusion_kernels_gpu.py compares them at T = 1).
template <typename T, int VEC, bool LINEAR>
__global__ __launch_bounds__(256) void md_target_step_kernel(const T* __restrict__ view, const T* __restrict__ uo, T* __restrict__ stepped, T* __restrict__ hist,
                                                              const float* __restrict__ coef, int nt, int64_t n) {
    constexpr StepForm FORM = LINEAR ? STEP_LINEAR : STEP_DDIM;
    const int t = blockIdx.y;
    float k[9] = {};
#pragma unroll
    for (int i = 0; i < 7; ++i) k[i] = coef[8 * t + i];
    const T* xv = view + (int64_t)t * n;
    const T* u = uo + (int64_t)t * n;
    const T* c = uo + (int64_t)(nt + t) * n;
    T* so = stepped + (int64_t)t * n;
    T* ho = LINEAR ? hist + (int64_t)t * n : nullptr;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n / VEC; q += (int64_t)gridDim.x * 256) {
        const int64_t i = q * VEC;
        T a[VEC], b[VEC], g[VEC], hh[VEC], o[VEC];
        load_n<T, VEC>(xv + i, a);
        load_n<T, VEC>(u + i, b);
        load_n<T, VEC>(c + i, g);
        if constexpr (LINEAR) load_n<T, VEC>(ho + i, hh);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float hv = 0.0f, d;
            if constexpr (LINEAR) hv = to_f32(hh[e]);
            o[e] = from_f32<T>(step_elem<T, FORM, true>(to_f32(a[e]), to_f32(b[e]), to_f32(g[e]), hv, 0.0f, k, d));
            if constexpr (LINEAR) hh[e] = from_f32<T>(d);
        }
        store_n<T, VEC>(so + i, o);
        if constexpr (LINEAR) store_n<T, VEC>(ho + i, hh);
    }
}

// One thread per VEC consecutive canvas elements of one row (VEC = 4: W % 4 == 0).  The descriptor table goes through LDS once per workgroup; a row
// outside the contract (see md_gather_kernel) is given no rows and contributes nothing.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void md_blend_kernel(T* __restrict__ canvas, const T* __restrict__ stepped, int64_t stepped_elems,
                                                        const mi355x_md_blend_desc* __restrict__ desc, int nt, int C, int H, int W) {
    __shared__ mi355x_md_blend_desc sd[MI355X_MD_MAX_TARGETS];
    for (int t = threadIdx.x; t < nt; t += 256) {
        mi355x_md_blend_desc d = desc[t];
        const bool ok = d.top >= 0 && d.left >= 0 && d.h > 0 && d.w > 0 && d.top <= H - d.h && d.left <= W - d.w && d.stepped_off >= 0 &&
                        d.stepped_off + (int64_t)C * d.h * d.w <= stepped_elems;
        if (!ok) d.h = 0;
        sd[t] = d;
    }
    __syncthreads();
    const int64_t total = (int64_t)C * H * W / VEC;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t i = q * VEC;
        const int c = (int)(i / ((int64_t)H * W));
        const int r = (int)(i - (int64_t)c * H * W);
        const int y = r / W, x0 = r - y * W;
        T xv[VEC];
        load_n<T, VEC>(canvas + i, xv);
        float num[VEC], cum[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) num[e] = 0.f, cum[e] = 0.f;
        for (int t = 0; t < nt; ++t) {  // list order: the reference's summation order (multi_diffusion.py:100-121)
            const mi355x_md_blend_desc& d = sd[t];
            const int ty = y - d.top;
            if (ty < 0 || ty >= d.h) continue;
            const T* tile = stepped + d.stepped_off + ((int64_t)c * d.h + ty) * d.w;
            const float* mrow = d.mask ? d.mask + c * d.mask_sc + ty * d.mask_sh : nullptr;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int tx = x0 + e - d.left;
                if (tx < 0 || tx >= d.w) continue;
                const float wgt = mrow ? mul_rn(d.weight, mrow[tx * d.mask_sw]) : d.weight;  // weight * opacity_mask
                num[e] = add_rn(num[e], wgt);
                cum[e] = add_rn(cum[e], mul_rn(wgt, to_f32(tile[tx])));
            }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (num[e] > 0.f) xv[e] = from_f32<T>(div_rn(cum[e], num[e]));  // where(num_updates > 0, cumulative / num_updates, x)
        store_n<T, VEC>(canvas + i, xv);
    }
}

}  // namespace

extern "C" int mi355x_md_gather(const mi355x_md_gather_args* a, void* stream) {
    if (!a || !a->canvas || !a->desc || !a->desc_host || !a->view || !a->model_in) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->T < 1 || a->T > MI355X_MD_MAX_TARGETS || a->C < 1 || a->h < 1 || a->w < 1 || a->H < a->h || a->W < a->w || a->n_init < 0) return MI355X_ESHAPE;
    const int64_t es = a->dtype == MI355X_F32 ? 4 : 2;
    const int64_t n = (int64_t)a->C * a->h * a->w, cn = (int64_t)a->C * a->H * a->W;
    for (int t = 0; t < a->T; ++t) {
        const mi355x_md_gather_desc& d = a->desc_host[t];
        if (d.kind != MI355X_MD_SRC_CANVAS && d.kind != MI355X_MD_SRC_INIT) return MI355X_EARG;
        if (d.top < 0 || d.left < 0 || d.top > a->H - a->h || d.left > a->W - a->w) return MI355X_ESHAPE;  // a tile outside the canvas
        if (d.kind == MI355X_MD_SRC_INIT && (!a->init || !a->noise || d.init_row < 0 || d.init_row >= a->n_init)) return MI355X_EARG;
    }
    const void* ins[3] = {a->canvas, a->noise, a->init};
    const int64_t inb[3] = {cn * es, cn * es, (int64_t)a->n_init * n * es};
    for (int i = 0; i < 3; ++i)
        if (overlap(a->view, a->T * n * es, ins[i], inb[i]) || overlap(a->model_in, 2 * a->T * n * es, ins[i], inb[i])) return MI355X_EARG;
    if (overlap(a->view, a->T * n * es, a->model_in, 2 * a->T * n * es)) return MI355X_EARG;
    const bool vec = a->w % 4 == 0 && al16(a->view) && al16(a->model_in);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(vec ? n / 4 : n), a->T);
#define MD_GATHER(TT, V)                                                                                                                              \
    hipLaunchKernelGGL((md_gather_kernel<TT, V>), grid, dim3(256), 0, st, static_cast<const TT*>(a->canvas), static_cast<const TT*>(a->noise),          \
                       static_cast<const TT*>(a->init), a->desc, static_cast<TT*>(a->view), static_cast<TT*>(a->model_in), a->T, a->C, a->h, a->w, a->H, \
                       a->W, a->n_init)
    if (a->dtype == MI355X_F32) {
        if (vec) MD_GATHER(float, 4); else MD_GATHER(float, 1);
    } else {
        if (vec) MD_GATHER(bf16_t, 4); else MD_GATHER(bf16_t, 1);
    }
#undef MD_GATHER
    return LAUNCH_OK();
}

extern "C" int mi355x_md_target_step(const mi355x_md_step_args* a, void* stream) {
    if (!a || !a->view || !a->unet_out || !a->stepped || !a->coef) return MI355X_EARG;
    if (a->form != MI355X_MD_FORM_DDIM && a->form != MI355X_MD_FORM_LINEAR) return MI355X_EARG;
    if (a->form == MI355X_MD_FORM_LINEAR && !a->hist) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->T < 1 || a->T > MI355X_MD_MAX_TARGETS || a->n < 1) return MI355X_ESHAPE;
    const int64_t es = a->dtype == MI355X_F32 ? 4 : 2, b = a->T * a->n * es;
    const void* hist = a->form == MI355X_MD_FORM_LINEAR ? a->hist : nullptr;
    // stepped may BE view (the update in place, as the batch kernels do it); any other sharing of bytes is refused
    if ((a->stepped != a->view && overlap(a->stepped, b, a->view, b)) || overlap(a->stepped, b, a->unet_out, 2 * b) || overlap(hist, b, a->view, b) ||
        overlap(hist, b, a->stepped, b) || overlap(hist, b, a->unet_out, 2 * b))
        return MI355X_EARG;
    const bool vec = a->n % 4 == 0 && al16(a->view) && al16(a->unet_out) && al16(a->stepped) && (!hist || al16(hist));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(vec ? a->n / 4 : a->n), a->T);
#define MD_STEP(TT, V, L)                                                                                                                           \
    hipLaunchKernelGGL((md_target_step_kernel<TT, V, L>), grid, dim3(256), 0, st, static_cast<const TT*>(a->view), static_cast<const TT*>(a->unet_out), \
                       static_cast<TT*>(a->stepped), static_cast<TT*>(a->hist), a->coef, a->T, a->n)
#define MD_STEP_V(TT, L)                \
    do {                                \
        if (vec) MD_STEP(TT, 4, L);     \
        else MD_STEP(TT, 1, L);         \
    } while (0)
    const bool lin = a->form == MI355X_MD_FORM_LINEAR;
    if (a->dtype == MI355X_F32) {
        if (lin) MD_STEP_V(float, true); else MD_STEP_V(float, false);
    } else {
        if (lin) MD_STEP_V(bf16_t, true); else MD_STEP_V(bf16_t, false);
    }
#undef MD_STEP_V
#undef MD_STEP
    return LAUNCH_OK();
}

extern "C" int mi355x_md_blend(const mi355x_md_blend_args* a, void* stream) {
    if (!a || !a->canvas) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->n_targets < 0 || a->n_targets > MI355X_MD_MAX_TARGETS || a->C < 1 || a->H < 1 || a->W < 1) return MI355X_ESHAPE;
    if (a->n_targets == 0) return MI355X_OK;  // no update anywhere: the canvas keeps x
    if (!a->stepped || !a->desc || !a->desc_host || a->stepped_elems < 1) return MI355X_EARG;
    const int64_t es = a->dtype == MI355X_F32 ? 4 : 2, cn = (int64_t)a->C * a->H * a->W;
    if (overlap(a->canvas, cn * es, a->stepped, a->stepped_elems * es)) return MI355X_EARG;
    for (int t = 0; t < a->n_targets; ++t) {
        const mi355x_md_blend_desc& d = a->desc_host[t];
        if (d.h < 1 || d.w < 1 || d.top < 0 || d.left < 0 || d.top > a->H - d.h || d.left > a->W - d.w) return MI355X_ESHAPE;  // a tile outside the canvas
        if (d.stepped_off < 0 || d.stepped_off + (int64_t)a->C * d.h * d.w > a->stepped_elems) return MI355X_EARG;
        if (d.mask && (d.mask_sc < 0 || d.mask_sh < 0 || d.mask_sw < 0 || (reinterpret_cast<uintptr_t>(d.mask) & 3))) return MI355X_EARG;
        if (d.mask && overlap(a->canvas, cn * es, d.mask, 4)) return MI355X_EARG;
    }
    const bool vec = a->W % 4 == 0 && al16(a->canvas);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(vec ? cn / 4 : cn));
#define MD_BLEND(TT, V)                                                                                                                        \
    hipLaunchKernelGGL((md_blend_kernel<TT, V>), grid, dim3(256), 0, st, static_cast<TT*>(a->canvas), static_cast<const TT*>(a->stepped),        \
                       a->stepped_elems, a->desc, a->n_targets, a->C, a->H, a->W)
    if (a->dtype == MI355X_F32) {
        if (vec) MD_BLEND(float, 4); else MD_BLEND(float, 1);
    } else {
        if (vec) MD_BLEND(bf16_t, 4); else MD_BLEND(bf16_t, 1);
    }
#undef MD_BLEND
    return LAUNCH_OK();
}
