// Step-constant UNet input channels (SD1.5 inpainting, IC-Light): the UNet reads model_in [n or 2n][C + E][hw] while the latents stay [n][C][hw].
//   cond_step            the step's last launch: the latent update of the batch step kernel (solver_step.hip; solver_update.cuh's step_elem, so x and
//                        hist are bit-equal to it) + the next step's model input, latents re-strided into C + E channel images, constants rescaled
//   cond_fill            primes a model input from x and / or the constants (first step; the second pass of Self-Attention Guidance)
//   inpaint_conditions   uint8 image + mask -> masked image in [-1, 1] and the nearest-resampled binary mask (set_inpainting_conditions minus the VAE)
// HBM-bound streaming kernels of a few hundred KB: 16-byte vectors when a channel row is a whole number of them and every pointer is aligned,
// single elements otherwise; grid-stride over "units" (one vector or one element), latents first, constants behind them.  No LDS.
#include "common.cuh"
#include "solver_update.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_cond_input.h"

namespace {

inline int grid_for(int64_t work, int per_block = 256, int cap = 4096) {
    int64_t b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}
// elements of an [a][b][c] tensor, or -1 when the product leaves 2^40 (no real latent does; keeps every byte count below inside int64)
inline int64_t elems(int64_t a, int64_t b, int64_t c) {
    int64_t r;
    if (__builtin_mul_overflow(a, b, &r) || __builtin_mul_overflow(r, c, &r) || r > ((int64_t)1 << 40)) return -1;
    return r;
}
// [a, a + ab) meets [b, b + bb); a NULL operand meets nothing
inline bool overlaps(const void* a, int64_t ab, const void* b, int64_t bb) {
    if (!a || !b || ab <= 0 || bb <= 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

// chw = C * hw, ehw = E * hw (elements per image); VEC: both are multiples of EPC and every pointer is 16-byte aligned.
// Units [0, n * chw / U) are the latents, the B * ehw / U behind them the constants (cond != NULL), U = EPC or 1, B = 2n guided, n not.
// One latent element is step_elem (solver_update.cuh), as in the batch kernel (solver_step.hip); the addressing is this kernel's own.
template <typename T, bool LINEAR, bool GUIDED, bool VEC>
__global__ __launch_bounds__(256) void cond_step_kernel(T* __restrict__ x, const T* __restrict__ uo, T* __restrict__ hist, T* __restrict__ model_in,
                                                         const T* __restrict__ cond, const float* __restrict__ coef, int n, int nc, int64_t chw,
                                                         int64_t ehw) {
    constexpr int U = VEC ? DT<T>::EPC : 1;
    constexpr StepForm FORM = LINEAR ? STEP_LINEAR : STEP_DDIM;
    float k[9] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = coef[i];
    const float sn = LINEAR ? k[7] : 1.0f;
    const int64_t lu = chw / U, cu = ehw / U, lat = (int64_t)n * lu, row = chw + ehw;
    const int B = GUIDED ? 2 * n : n;
    const int64_t total = lat + (cond ? (int64_t)B * cu : 0);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        if (q < lat) {
            const int64_t img = q / lu, i = q * U, o = img * row + (q - img * lu) * U;
            if constexpr (VEC) {
                const Vec16<T> xv = load16<T>(x + i), uv = load16<T>(uo + i);
                Vec16<T> cv = uv, hv = uv, xo, ho, mo;
                if constexpr (GUIDED) cv = load16<T>(uo + (int64_t)n * chw + i);
                if constexpr (LINEAR) hv = load16<T>(hist + i);
#pragma unroll
                for (int e = 0; e < U; ++e) {
                    float d;
                    xo.set(e, step_elem<T, FORM, GUIDED>(xv.get(e), uv.get(e), cv.get(e), hv.get(e), 0.0f, k, d));
                    ho.set(e, d);
                    mo.set(e, sn * xo.get(e));  // the next step scales the STORED latents, as solver.scale_model_input does
                }
                store16<T>(x + i, xo);
                if constexpr (LINEAR) store16<T>(hist + i, ho);
                store16<T>(model_in + o, LINEAR ? mo : xo);
                if constexpr (GUIDED) store16<T>(model_in + (int64_t)n * row + o, LINEAR ? mo : xo);
            } else {
                float d;
                const float u = to_f32(uo[i]), c = GUIDED ? to_f32(uo[(int64_t)n * chw + i]) : u, hv = LINEAR ? to_f32(hist[i]) : 0.0f;
                const T xs = from_f32<T>(step_elem<T, FORM, GUIDED>(to_f32(x[i]), u, c, hv, 0.0f, k, d));
                x[i] = xs;
                if constexpr (LINEAR) hist[i] = from_f32<T>(d);
                const T mi = LINEAR ? from_f32<T>(sn * to_f32(xs)) : xs;
                model_in[o] = mi;
                if constexpr (GUIDED) model_in[(int64_t)n * row + o] = mi;
            }
        } else {
            const int64_t p = q - lat, b = p / cu, r = (p - b * cu) * U;
            const T* src = cond + (nc == 1 ? 0 : b % n) * ehw + r;
            T* dst = model_in + b * row + chw + r;
            if constexpr (VEC) {
                const Vec16<T> v = load16<T>(src);
                Vec16<T> o;
#pragma unroll
                for (int e = 0; e < U; ++e) o.set(e, sn * v.get(e));
                store16<T>(dst, o);
            } else {
                *dst = from_f32<T>(sn * to_f32(*src));
            }
        }
    }
}

// Units [0, B * chw / U) are the latents (x != NULL), the B * ehw / U behind them the constants (cond != NULL).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void cond_fill_kernel(const T* __restrict__ x, const T* __restrict__ cond, T* __restrict__ model_in,
                                                         const float* __restrict__ s, int n, int B, int nc, int64_t chw, int64_t ehw) {
    constexpr int U = VEC ? DT<T>::EPC : 1;
    const float sv = s ? s[0] : 1.0f;
    const int64_t lu = chw / U, cu = ehw / U, lat = x ? (int64_t)B * lu : 0, row = chw + ehw;
    const int64_t total = lat + (cond ? (int64_t)B * cu : 0);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const bool is_lat = q < lat;
        const int64_t p = is_lat ? q : q - lat, per = is_lat ? lu : cu;
        const int64_t b = p / per, r = (p - b * per) * U;
        const T* src = is_lat ? x + (b % n) * chw + r : cond + (nc == 1 ? 0 : b % n) * ehw + r;
        T* dst = model_in + b * row + (is_lat ? 0 : chw) + r;
        if constexpr (VEC) {
            const Vec16<T> v = load16<T>(src);
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < U; ++e) o.set(e, sv * v.get(e));
            store16<T>(dst, o);
        } else {
            *dst = from_f32<T>(sv * to_f32(*src));
        }
    }
}

// Threads [0, n H W): one pixel each, three channel planes written (each plane coalesced); the nm h w behind them: one mask latent each.
template <typename T>
__global__ __launch_bounds__(256) void inpaint_conditions_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ mask,
                                                                  T* __restrict__ masked, T* __restrict__ mask_latents, int n, int nm, int H, int W,
                                                                  int h, int w) {
#pragma clang fp contract(off)
    const int64_t HW = (int64_t)H * W, pix = (int64_t)n * HW, total = pix + (int64_t)nm * h * w;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        if (q < pix) {
            const int64_t img = q / HW, p = q - img * HW;
            const float keep = 1.0f - (((float)mask[(nm == 1 ? 0 : img) * HW + p] / 255.0f > 0.5f) ? 1.0f : 0.0f);
            const uint8_t* px = image + q * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const T v = from_f32<T>((float)px[c] / 255.0f);       // image_to_tensor: float32 division, then the storage type
                const T t2 = from_f32<T>(to_f32(v) * 2.0f);           // `* 2 - 1` in the storage type: two materialised tensors
                const T t = from_f32<T>(to_f32(t2) - 1.0f);
                masked[(img * 3 + c) * HW + p] = from_f32<T>(to_f32(t) * keep);
            }
        } else {
            const int64_t p = q - pix, img = p / ((int64_t)h * w), r = p - img * h * w;
            const int dy = (int)(r / w), dx = (int)(r - (int64_t)dy * w);
            const float sy = (float)H / (float)h, sx = (float)W / (float)w;  // torch's nearest: min(floor(dst * scale), size - 1) in float32
            const int y = min((int)floorf((float)dy * sy), H - 1), xx = min((int)floorf((float)dx * sx), W - 1);
            mask_latents[p] = from_f32<T>(((float)mask[img * HW + (int64_t)y * W + xx] / 255.0f > 0.5f) ? 1.0f : 0.0f);
        }
    }
}

}  // namespace

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)

template <typename T, bool LINEAR, bool GUIDED>
static void launch_cond_step(bool vec, int grid, hipStream_t st, void* x, const void* uo, void* hist, void* model_in, const void* cond, const float* coef,
                             int n, int nc, int64_t chw, int64_t ehw) {
    if (vec)
        hipLaunchKernelGGL((cond_step_kernel<T, LINEAR, GUIDED, true>), dim3(grid), dim3(256), 0, st, static_cast<T*>(x), static_cast<const T*>(uo),
                           static_cast<T*>(hist), static_cast<T*>(model_in), static_cast<const T*>(cond), coef, n, nc, chw, ehw);
    else
        hipLaunchKernelGGL((cond_step_kernel<T, LINEAR, GUIDED, false>), dim3(grid), dim3(256), 0, st, static_cast<T*>(x), static_cast<const T*>(uo),
                           static_cast<T*>(hist), static_cast<T*>(model_in), static_cast<const T*>(cond), coef, n, nc, chw, ehw);
}

template <typename T>
static void dispatch_cond_step(int form, int guided, bool vec, int grid, hipStream_t st, void* x, const void* uo, void* hist, void* model_in,
                               const void* cond, const float* coef, int n, int nc, int64_t chw, int64_t ehw) {
    if (form == MI355X_COND_LINEAR) {
        if (guided) launch_cond_step<T, true, true>(vec, grid, st, x, uo, hist, model_in, cond, coef, n, nc, chw, ehw);
        else launch_cond_step<T, true, false>(vec, grid, st, x, uo, hist, model_in, cond, coef, n, nc, chw, ehw);
    } else {
        if (guided) launch_cond_step<T, false, true>(vec, grid, st, x, uo, hist, model_in, cond, coef, n, nc, chw, ehw);
        else launch_cond_step<T, false, false>(vec, grid, st, x, uo, hist, model_in, cond, coef, n, nc, chw, ehw);
    }
}

extern "C" int mi355x_cond_step(int32_t dtype, int32_t form, int32_t guided, void* x, const void* unet_out, void* hist, void* model_in,
                                const void* cond, const float* coef, int32_t n, int32_t C, int32_t E, int32_t nc, int64_t hw, void* stream) {
    if (!x || !unet_out || !model_in || !coef || n <= 0 || C <= 0 || hw <= 0 || E < 0) return MI355X_EARG;
    if ((form != MI355X_COND_DDIM && form != MI355X_COND_LINEAR) || (guided != 0 && guided != 1)) return MI355X_EARG;
    if (form == MI355X_COND_LINEAR && !hist) return MI355X_EARG;
    if (cond && ((nc != 1 && nc != n) || E == 0)) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int64_t B = guided ? 2 * (int64_t)n : n;
    if (elems(B, (int64_t)C + E, hw) < 0) return MI355X_ESHAPE;
    const int64_t es = dtype == MI355X_F32 ? 4 : 2, chw = (int64_t)C * hw, ehw = (int64_t)E * hw;
    const int64_t xb = n * chw * es, mb = B * (chw + ehw) * es;
    if (overlaps(model_in, mb, x, xb) || overlaps(model_in, mb, hist, xb) || overlaps(model_in, mb, unet_out, B * chw * es) ||
        overlaps(model_in, mb, cond, (int64_t)nc * ehw * es))
        return MI355X_EARG;
    const int epc = (int)(16 / es);
    const bool vec = (hw * es) % 16 == 0 && al16(x) && al16(unet_out) && al16(hist) && al16(model_in) && al16(cond);
    const int64_t u = vec ? epc : 1;
    const int grid = grid_for(n * chw / u + (cond ? B * ehw / u : 0));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == MI355X_F32) dispatch_cond_step<float>(form, guided, vec, grid, st, x, unet_out, hist, model_in, cond, coef, n, nc, chw, ehw);
    else dispatch_cond_step<bf16_t>(form, guided, vec, grid, st, x, unet_out, hist, model_in, cond, coef, n, nc, chw, ehw);
    return LAUNCH_OK();
}

template <typename T>
static void launch_cond_fill(bool vec, int grid, hipStream_t st, const void* x, const void* cond, void* model_in, const float* s, int n, int B, int nc,
                             int64_t chw, int64_t ehw) {
    if (vec)
        hipLaunchKernelGGL((cond_fill_kernel<T, true>), dim3(grid), dim3(256), 0, st, static_cast<const T*>(x), static_cast<const T*>(cond),
                           static_cast<T*>(model_in), s, n, B, nc, chw, ehw);
    else
        hipLaunchKernelGGL((cond_fill_kernel<T, false>), dim3(grid), dim3(256), 0, st, static_cast<const T*>(x), static_cast<const T*>(cond),
                           static_cast<T*>(model_in), s, n, B, nc, chw, ehw);
}

extern "C" int mi355x_cond_fill(int32_t dtype, const void* x, const void* cond, void* model_in, const float* s, int32_t n, int32_t B, int32_t C,
                                int32_t E, int32_t nc, int64_t hw, void* stream) {
    if (!model_in || (!x && !cond) || n <= 0 || C <= 0 || hw <= 0 || E < 0) return MI355X_EARG;
    if (B != n && (int64_t)B != 2 * (int64_t)n) return MI355X_EARG;
    if (cond && ((nc != 1 && nc != n) || E == 0)) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (elems(B, (int64_t)C + E, hw) < 0) return MI355X_ESHAPE;
    const int64_t es = dtype == MI355X_F32 ? 4 : 2, chw = (int64_t)C * hw, ehw = (int64_t)E * hw;
    const int64_t mb = (int64_t)B * (chw + ehw) * es;
    if (overlaps(model_in, mb, x, n * chw * es) || overlaps(model_in, mb, cond, (int64_t)nc * ehw * es)) return MI355X_EARG;
    const int epc = (int)(16 / es);
    const bool vec = (hw * es) % 16 == 0 && al16(x) && al16(cond) && al16(model_in);
    const int64_t u = vec ? epc : 1;
    const int grid = grid_for((x ? (int64_t)B * chw / u : 0) + (cond ? (int64_t)B * ehw / u : 0));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == MI355X_F32) launch_cond_fill<float>(vec, grid, st, x, cond, model_in, s, n, B, nc, chw, ehw);
    else launch_cond_fill<bf16_t>(vec, grid, st, x, cond, model_in, s, n, B, nc, chw, ehw);
    return LAUNCH_OK();
}

extern "C" int mi355x_inpaint_conditions(int32_t dtype, const void* image, const void* mask, void* masked_image, void* mask_latents, int32_t n,
                                         int32_t nm, int32_t H, int32_t W, int32_t h, int32_t w, void* stream) {
    if (!image || !mask || !masked_image || !mask_latents || n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return MI355X_EARG;
    if (nm != 1 && nm != n) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (elems(n, H, W) < 0 || elems(nm, h, w) < 0) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = grid_for((int64_t)n * H * W + (int64_t)nm * h * w);
    const uint8_t* im = static_cast<const uint8_t*>(image);
    const uint8_t* mk = static_cast<const uint8_t*>(mask);
    if (dtype == MI355X_F32)
        hipLaunchKernelGGL((inpaint_conditions_kernel<float>), dim3(grid), dim3(256), 0, st, im, mk, static_cast<float*>(masked_image),
                           static_cast<float*>(mask_latents), n, nm, H, W, h, w);
    else
        hipLaunchKernelGGL((inpaint_conditions_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, im, mk, static_cast<bf16_t*>(masked_image),
                           static_cast<bf16_t*>(mask_latents), n, nm, H, W, h, w);
    return LAUNCH_OK();
}
