// DINOv2's encoder (foundationals/dinov2/{vit,dinov2}.py of the reference): the streaming passes around its GEMMs and attention launches.
//   dinov2_pos_resample  InterpolateEmbedding as a separable filter over the channels-last position table -> float32 [h * w][D];
//                        bicubic, antialiased bicubic and bilinear are three host-built tap tables for ONE kernel (no NCHW permute)
//   dinov2_tokens        class row, register rows, patch rows + resampled positions, zero padding rows: the token matrix in one launch
//   glu_silu             GLU(SiLU()) of the giant model's feed-forward: x[:, :F] * silu(x[:, F:])
// All HBM-bound, float32 arithmetic, one lane per 16-byte output chunk, no atomics: replays are bit-equal.
#include "common.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_dinov2.h"

namespace {

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)
#define DISPATCH_T(dtype, CALL)              \
    do {                                     \
        if ((dtype) == MI355X_F32) {         \
            using T = float;                 \
            CALL;                            \
        } else {                             \
            using T = bf16_t;                \
            CALL;                            \
        }                                    \
    } while (0)

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline int grid_for(int64_t work, int cap = 16384) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
// bytes spanned by `rows` rows of E elements at stride ld
inline int64_t span(int64_t rows, int64_t ld, int E, int es) { return ((rows - 1) * ld + E) * es; }
inline bool bad_dtype(int32_t d) { return d != MI355X_F32 && d != MI355X_BF16; }

// EPC float32 values at p (16-byte aligned)
template <int EPC> MI_DEV void load_f32(const float* p, float (&v)[EPC]) {
#pragma unroll
    for (int c = 0; c < EPC / 4; ++c) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * c + e] = t[e];
    }
}
template <int EPC> MI_DEV void store_f32(float* p, const float (&v)[EPC]) {
#pragma unroll
    for (int c = 0; c < EPC / 4; ++c) {
        f32x4 t;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = v[4 * c + e];
        *reinterpret_cast<f32x4*>(p + 4 * c) = t;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ positions
struct ResampleP {
    const void* src;
    float* out;
    const int32_t *y0, *ny, *wy_off, *x0, *nx, *wx_off;
    const float *wy, *wx;
    int64_t lds, ldo;
    int Hs, Ws, h, w, nv, wy_len, wx_len;
};

// The tap tables live in device memory and the entry point cannot read them: every index taken from them is clamped to its range, so a
// table that breaks the caller's promise gives wrong numbers, never an access outside src / wy / wx.
template <typename T>
__global__ __launch_bounds__(256) void pos_resample_kernel(ResampleP p) {
    constexpr int EPC = DT<T>::EPC;
    const T* src = static_cast<const T*>(p.src);
    const int64_t work = (int64_t)p.h * p.w * p.nv;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < work; q += (int64_t)gridDim.x * 256) {
        const int cv = (int)(q % p.nv);
        const int64_t cell = q / p.nv;
        const int j = (int)(cell % p.w), i = (int)(cell / p.w);
        const int ys = p.y0[i], xs = p.x0[j], ty = p.ny[i], tx = p.nx[j], oy = p.wy_off[i], ox = p.wx_off[j];
        float acc[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
        for (int a = 0; a < ty; ++a) {
            const int yy = min(max(ys + a, 0), p.Hs - 1);
            const float fy = p.wy[min(max(oy + a, 0), p.wy_len - 1)];
            float row[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) row[e] = 0.f;
            for (int b = 0; b < tx; ++b) {
                const int xx = min(max(xs + b, 0), p.Ws - 1);
                const float fx = p.wx[min(max(ox + b, 0), p.wx_len - 1)];
                const Vec16<T> v = load16(src + ((int64_t)yy * p.Ws + xx) * p.lds + cv * EPC);
#pragma unroll
                for (int e = 0; e < EPC; ++e) row[e] += fx * v.get(e);
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] += fy * row[e];
        }
        store_f32<EPC>(p.out + cell * p.ldo + cv * EPC, acc);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ tokens
struct TokensP {
    const void *patch, *cls, *pos0, *reg;
    const float* pos;
    void* out;
    int64_t ldp, ldpos, ldr, ldo;
    int B, n, R, rows, nv;
};

template <typename T>
__global__ __launch_bounds__(256) void tokens_kernel(TokensP p) {
    constexpr int EPC = DT<T>::EPC;
    const T* patch = static_cast<const T*>(p.patch);
    const T* cls = static_cast<const T*>(p.cls);
    const T* pos0 = static_cast<const T*>(p.pos0);
    const T* reg = static_cast<const T*>(p.reg);
    T* out = static_cast<T*>(p.out);
    const int64_t work = (int64_t)p.B * p.rows * p.nv;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < work; q += (int64_t)gridDim.x * 256) {
        const int cv = (int)(q % p.nv);
        const int64_t row = q / p.nv;
        const int t = (int)(row % p.rows), b = (int)(row / p.rows);
        const int col = cv * EPC;
        Vec16<T> o;
        if (t == 0) {
            const Vec16<T> c = load16(cls + col), z = load16(pos0 + col);
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, c.get(e) + z.get(e));
        } else if (t <= p.R) {
            o = load16(reg + (int64_t)(t - 1) * p.ldr + col);
        } else if (t < 1 + p.R + p.n) {
            const int i = t - 1 - p.R;
            const Vec16<T> v = load16(patch + ((int64_t)b * p.n + i) * p.ldp + col);
            float z[EPC];
            load_f32<EPC>(p.pos + (int64_t)i * p.ldpos + col, z);
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, v.get(e) + z[e]);
        } else {
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, 0.f);
        }
        store16(out + row * p.ldo + col, o);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ GLU(SiLU)
template <typename T>
__global__ __launch_bounds__(256) void glu_silu_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ out, int64_t ldo, int M, int F, int nv) {
    constexpr int EPC = DT<T>::EPC;
    const int64_t work = (int64_t)M * nv;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < work; q += (int64_t)gridDim.x * 256) {
        const int cv = (int)(q % nv);
        const int64_t m = q / nv;
        const Vec16<T> a = load16(x + m * ldx + cv * EPC), g = load16(x + m * ldx + F + cv * EPC);
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const float gv = g.get(e);
            o.set(e, a.get(e) * (gv / (1.0f + __expf(-gv))));  // exp overflows to +inf for gv < -88: the quotient is -0, never NaN
        }
        store16(out + m * ldo + cv * EPC, o);
    }
}

}  // namespace

extern "C" int mi355x_dinov2_pos_resample(const mi355x_dinov2_pos_resample_args* a, void* stream) {
    if (!a || !a->src || !a->out || !a->y0 || !a->ny || !a->wy_off || !a->wy || !a->x0 || !a->nx || !a->wx_off || !a->wx || a->D < 1) return MI355X_EARG;
    if (bad_dtype(a->dtype)) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->h < 1 || a->w < 1 || a->Hs < 1 || a->Ws < 1 || a->wy_len < 1 || a->wx_len < 1 || a->lds < a->D || a->ldo < a->D) return MI355X_ESHAPE;
    if ((a->D * es) % 16 || (a->lds * es) % 16 || (a->ldo * 4) % 16 || !al16(a->src) || !al16(a->out)) return MI355X_ESHAPE;
    if (!al4(a->y0) || !al4(a->ny) || !al4(a->wy_off) || !al4(a->wy) || !al4(a->x0) || !al4(a->nx) || !al4(a->wx_off) || !al4(a->wx)) return MI355X_ESHAPE;
    if (overlap(a->src, span((int64_t)a->Hs * a->Ws, a->lds, a->D, es), a->out, span((int64_t)a->h * a->w, a->ldo, a->D, 4))) return MI355X_EARG;
    ResampleP p;
    p.src = a->src, p.out = a->out, p.y0 = a->y0, p.ny = a->ny, p.wy_off = a->wy_off, p.x0 = a->x0, p.nx = a->nx, p.wx_off = a->wx_off, p.wy = a->wy, p.wx = a->wx;
    p.lds = a->lds, p.ldo = a->ldo, p.Hs = a->Hs, p.Ws = a->Ws, p.h = a->h, p.w = a->w, p.nv = a->D * es / 16, p.wy_len = a->wy_len, p.wx_len = a->wx_len;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((int64_t)a->h * a->w * p.nv));
    DISPATCH_T(a->dtype, hipLaunchKernelGGL((pos_resample_kernel<T>), grid, dim3(256), 0, st, p));
    return LAUNCH_OK();
}

extern "C" int mi355x_dinov2_tokens(const mi355x_dinov2_tokens_args* a, void* stream) {
    if (!a || !a->patch || !a->pos || !a->cls || !a->pos0 || !a->out || a->D < 1 || (a->R > 0 && !a->reg)) return MI355X_EARG;
    if (bad_dtype(a->dtype)) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B < 1 || a->n < 1 || a->R < 0 || (int64_t)a->rows < (int64_t)1 + a->R + a->n || a->ldp < a->D || a->ldpos < a->D || a->ldo < a->D || (a->R > 0 && a->ldr < a->D)) return MI355X_ESHAPE;
    if ((a->D * es) % 16 || (a->ldp * es) % 16 || (a->ldo * es) % 16 || (a->ldpos * 4) % 16 || (a->R > 0 && (a->ldr * es) % 16)) return MI355X_ESHAPE;
    if (!al16(a->patch) || !al16(a->pos) || !al16(a->cls) || !al16(a->pos0) || !al16(a->out) || (a->R > 0 && !al16(a->reg))) return MI355X_ESHAPE;
    if (overlap(a->patch, span((int64_t)a->B * a->n, a->ldp, a->D, es), a->out, span((int64_t)a->B * a->rows, a->ldo, a->D, es))) return MI355X_EARG;
    TokensP p;
    p.patch = a->patch, p.cls = a->cls, p.pos0 = a->pos0, p.reg = a->R > 0 ? a->reg : nullptr, p.pos = a->pos, p.out = a->out;
    p.ldp = a->ldp, p.ldpos = a->ldpos, p.ldr = a->ldr, p.ldo = a->ldo, p.B = a->B, p.n = a->n, p.R = a->R, p.rows = a->rows, p.nv = a->D * es / 16;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((int64_t)a->B * a->rows * p.nv));
    DISPATCH_T(a->dtype, hipLaunchKernelGGL((tokens_kernel<T>), grid, dim3(256), 0, st, p));
    return LAUNCH_OK();
}

extern "C" int mi355x_glu_silu(int32_t dtype, const void* x, int64_t ldx, void* out, int64_t ldo, int32_t M, int32_t F, void* stream) {
    if (!x || !out || F < 1) return MI355X_EARG;
    if (bad_dtype(dtype)) return MI355X_EDTYPE;
    const int es = dtype == MI355X_F32 ? 4 : 2;
    if (M < 1 || ldx < 2 * (int64_t)F || ldo < F) return MI355X_ESHAPE;
    if ((F * es) % 16 || (ldx * es) % 16 || (ldo * es) % 16 || !al16(x) || !al16(out)) return MI355X_ESHAPE;
    if (overlap(x, span(M, ldx, 2 * F, es), out, span(M, ldo, F, es))) return MI355X_EARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nv = F * es / 16;
    DISPATCH_T(dtype, hipLaunchKernelGGL((glu_silu_kernel<T>), dim3(grid_for((int64_t)M * nv)), dim3(256), 0, st, static_cast<const T*>(x), ldx, static_cast<T*>(out), ldo, (int)M, (int)F, nv));
    return LAUNCH_OK();
}
