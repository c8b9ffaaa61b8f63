// The launch that ends a denoising step of a plain batch: (classifier-free guidance +) solver update + history + the next step's model input.
// ONE kernel, step_kernel<T, FORM, GUIDED>, behind six entry points:
//   FORM     DDIM                      x' = ddim(x, eps);                                                     model_in = x'
//            LINEAR                    d = hx x + he eps;  x' = kx x + ke eps + kd d + kp hist;  hist = d;    model_in = s_next x'
//            SDE                       LINEAR plus kn noise, the step's Gaussian draw as a fifth, read-only operand (SDE DPM-Solver++ 2M)
//   GUIDED   unet_out = [uncond ; cond] (2n elements), eps = u + cfg (c - u), both halves of model_in (2n elements) written; otherwise
//            eps = unet_out (n elements: LCM, LCM-LoRA, SDXL-Lightning) and model_in has n
// The arithmetic of one element is step_elem (solver_update.cuh).  HBM-bound streaming kernel: 16-byte vectors, grid-stride, the last n % EPC
// elements (or everything, behind a pointer that is not 16-byte aligned) one element per lane.  In the guided form the conditional half of unet_out
// and the second half of model_in start n elements in, so the vector loop also needs n to be a whole number of vectors.
#include "common.cuh"
#include "solver_update.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_solver_step.h"
#include "../../include/mi355x_refiners_sde_step.h"

namespace {

inline int grid_for(int64_t work, int per_block = 256, int cap = 4096) {
    int64_t b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// nv = number of 16-byte vectors the vector loop covers (0 when an operand is misaligned); elements [nv * EPC, n) go through the element loop.
// hist is read and written by LINEAR and SDE only, noise read by SDE only; model_in may be NULL (nothing written).
template <typename T, StepForm FORM, bool GUIDED>
__global__ __launch_bounds__(256) void step_kernel(T* __restrict__ x, const T* __restrict__ uo, T* __restrict__ hist, const T* __restrict__ noise,
                                                    T* __restrict__ model_in, const float* __restrict__ coef, int64_t n, int64_t nv) {
    constexpr int EPC = DT<T>::EPC;
    constexpr bool KEEPS = FORM != STEP_DDIM;              // has a history operand and an input scale
    constexpr int NK = FORM == STEP_DDIM ? 5 : (FORM == STEP_LINEAR ? 8 : 9);  // callers pass rows of exactly this many floats
    float k[9] = {};
#pragma unroll
    for (int i = 0; i < NK; ++i) k[i] = coef[i];
    const float sn = k[7];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t v = tid; v < nv; v += stride) {
        const int64_t i = v * EPC;
        const Vec16<T> xv = load16<T>(x + i), uv = load16<T>(uo + i);
        Vec16<T> cv = uv, hv = uv, zv = uv, xo, ho, mo;
        if constexpr (GUIDED) cv = load16<T>(uo + n + i);
        if constexpr (KEEPS) hv = load16<T>(hist + i);
        if constexpr (FORM == STEP_SDE) zv = load16<T>(noise + i);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            float d;
            xo.set(e, step_elem<T, FORM, GUIDED>(xv.get(e), uv.get(e), cv.get(e), hv.get(e), zv.get(e), k, d));
            ho.set(e, d);
            mo.set(e, sn * xo.get(e));  // the next step scales the STORED latents, as solver.scale_model_input does
        }
        store16<T>(x + i, xo);
        if constexpr (KEEPS) store16<T>(hist + i, ho);
        if (model_in) {
            store16<T>(model_in + i, KEEPS ? mo : xo);
            if constexpr (GUIDED) store16<T>(model_in + n + i, KEEPS ? mo : xo);
        }
    }
    for (int64_t i = nv * EPC + tid; i < n; i += stride) {
        float d;
        const float u = to_f32(uo[i]), c = GUIDED ? to_f32(uo[n + i]) : u;
        const float hv = KEEPS ? to_f32(hist[i]) : 0.0f, nz = FORM == STEP_SDE ? to_f32(noise[i]) : 0.0f;
        const T xs = from_f32<T>(step_elem<T, FORM, GUIDED>(to_f32(x[i]), u, c, hv, nz, k, d));
        x[i] = xs;
        if constexpr (KEEPS) hist[i] = from_f32<T>(d);
        if (model_in) {
            const T mi = KEEPS ? from_f32<T>(sn * to_f32(xs)) : xs;
            model_in[i] = mi;
            if constexpr (GUIDED) model_in[n + i] = mi;
        }
    }
}

// hist / noise: NULL from the entry points whose form has no such operand
template <StepForm FORM, bool GUIDED>
int launch_step(int32_t dtype, void* x, const void* uo, void* hist, const void* noise, void* model_in, const float* coef, int64_t n, void* stream) {
    if (!x || !uo || !coef || n <= 0 || (FORM != STEP_DDIM && !hist) || (FORM == STEP_SDE && !noise)) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int epc = dtype == MI355X_F32 ? 4 : 8;
    // (guided: unet_out + n and model_in + n are 16-byte aligned only when n is a whole number of vectors)
    const bool vec = al16(x) && al16(uo) && al16(hist) && al16(noise) && al16(model_in) && (!GUIDED || n % epc == 0);
    const int64_t nv = vec ? n / epc : 0;
    const dim3 grid(grid_for(nv > 0 ? nv : n)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == MI355X_F32)
        hipLaunchKernelGGL((step_kernel<float, FORM, GUIDED>), grid, block, 0, st, static_cast<float*>(x), static_cast<const float*>(uo),
                           static_cast<float*>(hist), static_cast<const float*>(noise), static_cast<float*>(model_in), coef, n, nv);
    else
        hipLaunchKernelGGL((step_kernel<bf16_t, FORM, GUIDED>), grid, block, 0, st, static_cast<bf16_t*>(x), static_cast<const bf16_t*>(uo),
                           static_cast<bf16_t*>(hist), static_cast<const bf16_t*>(noise), static_cast<bf16_t*>(model_in), coef, n, nv);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

}  // namespace

extern "C" int mi355x_cfg_ddim_step(int32_t dtype, void* x, const void* unet_out, const float* coef, int64_t n, void* stream) {
    return launch_step<STEP_DDIM, true>(dtype, x, unet_out, nullptr, nullptr, nullptr, coef, n, stream);
}

extern "C" int mi355x_cfg_linear_step(int32_t dtype, void* x, const void* unet_out, void* hist, void* model_in, const float* coef, int64_t n,
                                      void* stream) {
    return launch_step<STEP_LINEAR, true>(dtype, x, unet_out, hist, nullptr, model_in, coef, n, stream);
}

extern "C" int mi355x_ddim_step(int32_t dtype, void* x, const void* unet_out, void* model_in, const float* coef, int64_t n, void* stream) {
    return launch_step<STEP_DDIM, false>(dtype, x, unet_out, nullptr, nullptr, model_in, coef, n, stream);
}

extern "C" int mi355x_linear_step(int32_t dtype, void* x, const void* unet_out, void* hist, void* model_in, const float* coef, int64_t n,
                                  void* stream) {
    return launch_step<STEP_LINEAR, false>(dtype, x, unet_out, hist, nullptr, model_in, coef, n, stream);
}

extern "C" int mi355x_cfg_sde_step(int32_t dtype, void* x, const void* unet_out, void* hist, const void* noise, void* model_in, const float* coef,
                                   int64_t n, void* stream) {
    return launch_step<STEP_SDE, true>(dtype, x, unet_out, hist, noise, model_in, coef, n, stream);
}

extern "C" int mi355x_sde_step(int32_t dtype, void* x, const void* unet_out, void* hist, const void* noise, void* model_in, const float* coef,
                               int64_t n, void* stream) {
    return launch_step<STEP_SDE, false>(dtype, x, unet_out, hist, noise, model_in, coef, n, stream);
}
