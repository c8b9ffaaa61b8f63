// Guidance-free solver updates (classifier_free_guidance = False: LCM, LCM-LoRA, SDXL-Lightning): the arithmetic of cfg_ddim_kernel /
// cfg_linear_kernel (elementwise.hip) with eps = the UNet's output (n rows, no [uncond ; cond] pair).  HBM-bound streaming kernels: 16-byte
// vectors, grid-stride, the last n % EPC elements (or everything, behind a pointer that is not 16-byte aligned) one element per lane.
#include "common.cuh"
#include "solver_update.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_solver_step.h"

namespace {

inline int grid_for(int64_t work, int per_block = 256, int cap = 4096) {
    int64_t b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// nv = number of 16-byte vectors the vector loop covers (0 when an operand is misaligned); elements [nv * EPC, n) go through the scalar loop
template <typename T>
__global__ __launch_bounds__(256) void ddim_step_kernel(T* __restrict__ x, const T* __restrict__ uo, T* __restrict__ model_in,
                                                         const float* __restrict__ coef, int64_t n, int64_t nv) {
    constexpr int EPC = DT<T>::EPC;
    const float sa = coef[1], s1a = coef[2], sap = coef[3], s1ap = coef[4];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < nv; i += stride) {
        const Vec16<T> xv = load16<T>(x + i * EPC), ev = load16<T>(uo + i * EPC);
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.set(e, ddim_update(xv.get(e), ev.get(e), sa, s1a, sap, s1ap));
        store16<T>(x + i * EPC, o);
        if (model_in) store16<T>(model_in + i * EPC, o);
    }
    for (int64_t i = nv * EPC + tid; i < n; i += stride) {
        const T xs = from_f32<T>(ddim_update(to_f32(x[i]), to_f32(uo[i]), sa, s1a, sap, s1ap));
        x[i] = xs;
        if (model_in) model_in[i] = xs;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void linear_step_kernel(T* __restrict__ x, const T* __restrict__ uo, T* __restrict__ hist, T* __restrict__ model_in,
                                                           const float* __restrict__ coef, int64_t n, int64_t nv) {
    constexpr int EPC = DT<T>::EPC;
    const float hx = coef[1], he = coef[2], kx = coef[3], ke = coef[4], kd = coef[5], kp = coef[6], sn = coef[7];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < nv; i += stride) {
        const Vec16<T> xv = load16<T>(x + i * EPC), ev = load16<T>(uo + i * EPC), hv = load16<T>(hist + i * EPC);
        Vec16<T> xo, ho, mo;
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            float d;
            xo.set(e, linear_update<T>(xv.get(e), ev.get(e), hv.get(e), hx, he, kx, ke, kd, kp, d));
            ho.set(e, d);
            mo.set(e, sn * xo.get(e));  // the next step scales the STORED latents, as solver.scale_model_input does
        }
        store16<T>(x + i * EPC, xo);
        store16<T>(hist + i * EPC, ho);
        if (model_in) store16<T>(model_in + i * EPC, mo);
    }
    for (int64_t i = nv * EPC + tid; i < n; i += stride) {
        float d;
        const T xs = from_f32<T>(linear_update<T>(to_f32(x[i]), to_f32(uo[i]), to_f32(hist[i]), hx, he, kx, ke, kd, kp, d));
        x[i] = xs;
        hist[i] = from_f32<T>(d);
        if (model_in) model_in[i] = from_f32<T>(sn * to_f32(xs));
    }
}

}  // namespace

#define DISPATCH_T(dtype, ...)                                    \
    do {                                                          \
        if ((dtype) == MI355X_F32) { using T = float; __VA_ARGS__; } \
        else if ((dtype) == MI355X_BF16) { using T = bf16_t; __VA_ARGS__; } \
        else return MI355X_EDTYPE;                                \
    } while (0)
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)

extern "C" int mi355x_ddim_step(int32_t dtype, void* x, const void* unet_out, void* model_in, const float* coef, int64_t n, void* stream) {
    if (!x || !unet_out || !coef || n <= 0) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = al16(x) && al16(unet_out) && al16(model_in);
    const int64_t nv = vec ? n / (dtype == MI355X_F32 ? 4 : 8) : 0;
    const int grid = grid_for(nv > 0 ? nv : n);
    DISPATCH_T(dtype, hipLaunchKernelGGL((ddim_step_kernel<T>), dim3(grid), dim3(256), 0, st, static_cast<T*>(x), static_cast<const T*>(unet_out),
                                         static_cast<T*>(model_in), coef, n, nv));
    return LAUNCH_OK();
}

extern "C" int mi355x_linear_step(int32_t dtype, void* x, const void* unet_out, void* hist, void* model_in, const float* coef, int64_t n,
                                  void* stream) {
    if (!x || !unet_out || !hist || !coef || n <= 0) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = al16(x) && al16(unet_out) && al16(hist) && al16(model_in);
    const int64_t nv = vec ? n / (dtype == MI355X_F32 ? 4 : 8) : 0;
    const int grid = grid_for(nv > 0 ? nv : n);
    DISPATCH_T(dtype, hipLaunchKernelGGL((linear_step_kernel<T>), dim3(grid), dim3(256), 0, st, static_cast<T*>(x), static_cast<const T*>(unet_out),
                                         static_cast<T*>(hist), static_cast<T*>(model_in), coef, n, nv));
    return LAUNCH_OK();
}
