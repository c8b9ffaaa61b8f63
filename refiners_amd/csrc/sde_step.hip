// Stochastic solver updates (SDE DPM-Solver++ 2M, solvers/dpm.py:241-246, 284-290): the arithmetic of cfg_linear_kernel (elementwise.hip) /
// linear_step_kernel (solver_step.hip) plus the step's Gaussian draw as a fifth, read-only operand:
//   eps = u + cfg (c - u) (guided) or the UNet's output;  d = hx x + he eps;  x' = kx x + ke eps + kd d + kp hist + kn noise;  hist = d
// HBM-bound streaming kernels: 16-byte vectors, grid-stride, the last n % EPC elements (or everything, behind a pointer that is not 16-byte
// aligned) one element per lane.  In the guided form the conditional half of unet_out and the second half of model_in start n elements in, so
// the vector loop also needs n to be a whole number of vectors.
#include "common.cuh"
#include "solver_update.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_sde_step.h"

namespace {

inline int grid_for(int64_t work, int per_block = 256, int cap = 4096) {
    int64_t b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One latent element.  eps = fma(cfg, c - u, u) is what mi355x_cfg_linear_step computes (the list in solver_update.cuh).
template <typename T, bool GUIDED> MI_DEV float sde_elem(float xv, float u, float c, float hv, float nz, const float (&k)[9], float& d) {
    const float eps = GUIDED ? fmaf(k[0], c - u, u) : u;
    return sde_update<T>(xv, eps, hv, nz, k[1], k[2], k[3], k[4], k[5], k[6], k[8], d);
}

// nv = number of 16-byte vectors the vector loop covers (0 when an operand is misaligned); elements [nv * EPC, n) go through the scalar loop
template <typename T, bool GUIDED>
__global__ __launch_bounds__(256) void sde_step_kernel(T* __restrict__ x, const T* __restrict__ uo, T* __restrict__ hist, const T* __restrict__ noise,
                                                        T* __restrict__ model_in, const float* __restrict__ coef, int64_t n, int64_t nv) {
    constexpr int EPC = DT<T>::EPC;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = coef[i];
    const float sn = k[7];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t v = tid; v < nv; v += stride) {
        const int64_t i = v * EPC;
        const Vec16<T> xv = load16<T>(x + i), uv = load16<T>(uo + i), hv = load16<T>(hist + i), zv = load16<T>(noise + i);
        Vec16<T> cv = uv, xo, ho, mo;
        if constexpr (GUIDED) cv = load16<T>(uo + n + i);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            float d;
            xo.set(e, sde_elem<T, GUIDED>(xv.get(e), uv.get(e), cv.get(e), hv.get(e), zv.get(e), k, d));
            ho.set(e, d);
            mo.set(e, sn * xo.get(e));  // the next step scales the STORED latents, as solver.scale_model_input does
        }
        store16<T>(x + i, xo);
        store16<T>(hist + i, ho);
        if (model_in) {
            store16<T>(model_in + i, mo);
            if constexpr (GUIDED) store16<T>(model_in + n + i, mo);
        }
    }
    for (int64_t i = nv * EPC + tid; i < n; i += stride) {
        float d;
        const float u = to_f32(uo[i]), c = GUIDED ? to_f32(uo[n + i]) : u;
        const T xs = from_f32<T>(sde_elem<T, GUIDED>(to_f32(x[i]), u, c, to_f32(hist[i]), to_f32(noise[i]), k, d));
        x[i] = xs;
        hist[i] = from_f32<T>(d);
        if (model_in) {
            const T mi = from_f32<T>(sn * to_f32(xs));
            model_in[i] = mi;
            if constexpr (GUIDED) model_in[n + i] = mi;
        }
    }
}

template <typename T, bool GUIDED>
void launch_sde_step(hipStream_t st, void* x, const void* uo, void* hist, const void* noise, void* model_in, const float* coef, int64_t n) {
    constexpr int EPC = DT<T>::EPC;
    // (guided: unet_out + n and model_in + n are 16-byte aligned only when n is a whole number of vectors)
    const bool vec = al16(x) && al16(uo) && al16(hist) && al16(noise) && al16(model_in) && (!GUIDED || n % EPC == 0);
    const int64_t nv = vec ? n / EPC : 0;
    const int grid = grid_for(nv > 0 ? nv : n);
    hipLaunchKernelGGL((sde_step_kernel<T, GUIDED>), dim3(grid), dim3(256), 0, st, static_cast<T*>(x), static_cast<const T*>(uo), static_cast<T*>(hist),
                       static_cast<const T*>(noise), static_cast<T*>(model_in), coef, n, nv);
}

template <bool GUIDED>
int sde_step(int32_t dtype, void* x, const void* uo, void* hist, const void* noise, void* model_in, const float* coef, int64_t n, void* stream) {
    if (!x || !uo || !hist || !noise || !coef || n <= 0) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == MI355X_F32) launch_sde_step<float, GUIDED>(st, x, uo, hist, noise, model_in, coef, n);
    else launch_sde_step<bf16_t, GUIDED>(st, x, uo, hist, noise, model_in, coef, n);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

}  // namespace

extern "C" int mi355x_cfg_sde_step(int32_t dtype, void* x, const void* unet_out, void* hist, const void* noise, void* model_in, const float* coef,
                                   int64_t n, void* stream) {
    return sde_step<true>(dtype, x, unet_out, hist, noise, model_in, coef, n, stream);
}

extern "C" int mi355x_sde_step(int32_t dtype, void* x, const void* unet_out, void* hist, const void* noise, void* model_in, const float* coef,
                               int64_t n, void* stream) {
    return sde_step<false>(dtype, x, unet_out, hist, noise, model_in, coef, n, stream);
}
