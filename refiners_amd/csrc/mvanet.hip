// MVANet's multi-view decoder (foundationals/swin/mvanet/{mvanet,mclm,mcrm,utils}.py of the reference): the streaming passes between its GEMMs,
// convolutions and attention launches.  Activations are channels-last token rows [views * S * S][E]; the reference's PatchMerge / PatchSplit /
// nearest and bilinear Interpolate / Rescale are index arithmetic here, never a copy.
//   mvanet_pool        MultiPool: average pools at up to three ratios -> key rows, padding rows zeroed
//   mvanet_gate        local *= sigmoid(conv1x1(global)) upsampled 2x and split into quadrants: one wave per global pixel
//   mvanet_resize_add  out = resize(f(a)) + g(b), f / g identity or PReLU (slope from device memory), bilinear / nearest, merged operands
//   mvanet_prelu       in-place PReLU
//   mvanet_split_views NCHW image -> its four quadrants and the 2 x 2 block means
// All HBM-bound, float32 arithmetic, one lane per output element (vector), no atomics: replays are bit-equal.
#include "common.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_mvanet.h"

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

inline bool al(const void* p, int es) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(es - 1)) == 0; }
inline int grid_for(int64_t work, int cap = 16384) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
// bytes spanned by `rows` rows of E elements at stride ld
inline int64_t span(int64_t rows, int64_t ld, int E, int es) { return ((rows - 1) * ld + E) * es; }

MI_DEV float prelu_f(float v, float s) { return fmaxf(v, 0.f) + s * fminf(v, 0.f); }
// row of pixel (Y, X) of the PatchMerge of four h x w views
MI_DEV int64_t merged_row(int Y, int X, int h, int w) { return ((int64_t)(2 * (Y / h) + X / w) * h + Y % h) * w + X % w; }

// ------------------------------------------------------------------------------------------------------------------------ pool
struct PoolP {
    const void* src;
    void* out;
    int64_t lds, ldo, group_stride;
    int mode, S, G, nv, rows, n;
    int ratio[MI355X_MVANET_MAX_RATIOS], base[MI355X_MVANET_MAX_RATIOS + 1];
};

template <typename T>
__global__ __launch_bounds__(256) void pool_kernel(PoolP p) {
    constexpr int EPC = DT<T>::EPC;
    const int grp = blockIdx.y;
    const T* src = static_cast<const T*>(p.src);
    T* out = static_cast<T*>(p.out) + grp * p.group_stride;
    const int64_t work = (int64_t)p.rows * p.nv;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < work; q += (int64_t)gridDim.x * 256) {
        const int cv = (int)(q % p.nv), row = (int)(q / p.nv);
        Vec16<T> o;
        float acc[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
        if (row < p.base[p.n]) {
            int i = 0;
            while (row >= p.base[i + 1]) ++i;
            const int r = p.ratio[i], side = p.G / r, local = row - p.base[i];
            const int py = local / side, px = local % side;
            for (int dy = 0; dy < r; ++dy)
                for (int dx = 0; dx < r; ++dx) {
                    const int Y = py * r + dy, X = px * r + dx;
                    const int64_t srow = p.mode == 0 ? merged_row(Y, X, p.S, p.S) : (int64_t)((grp >> 1) * p.G + Y) * p.S + (grp & 1) * p.G + X;
                    const Vec16<T> v = load16(src + srow * p.lds + cv * EPC);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) acc[e] += v.get(e);
                }
            const float inv = 1.f / (float)(r * r);
#pragma unroll
            for (int e = 0; e < EPC; ++e) acc[e] *= inv;
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.set(e, acc[e]);
        store16(out + (int64_t)row * p.ldo + cv * EPC, o);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ gate
template <typename T>
__global__ __launch_bounds__(256) void gate_kernel(const T* __restrict__ local, int64_t ldl, const T* __restrict__ glb, int64_t ldg, const T* __restrict__ w,
                                                   const T* __restrict__ b, T* out, int64_t ldo, int S, int E) {
    const int lane = threadIdx.x & 63;
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per pixel of the global view (uniform per wave)
    if (pix >= (int64_t)S * S) return;
    const T* g = glb + pix * ldg;
    float z = 0.f;
    for (int c = lane; c < E; c += 64) z += to_f32(w[c]) * to_f32(g[c]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) z += __shfl_xor(z, m, 64);
    const float gate = 1.f / (1.f + expf(-(z + to_f32(b[0]))));
    const int gy = (int)(pix / S), gx = (int)(pix % S);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t row = merged_row(2 * gy + (t >> 1), 2 * gx + (t & 1), S, S);
        for (int c = lane; c < E; c += 64) out[row * ldo + c] = from_f32<T>(to_f32(local[row * ldl + c]) * gate);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ resize + add
struct ResizeP {
    const void *a, *b, *slope_a, *slope_b;
    void* out;
    int64_t lda, ldb, ldo;
    int B, nv, Ha, Wa, Ho, Wo, a_merge, b_merge;
};

// source coordinate of torch's bilinear rule along one axis -> (i0, i1, l1)
MI_DEV void bilinear_axis(int dst, float scale, int in, int& i0, int& i1, float& l1) {
    const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    i0 = min((int)s, in - 1);
    i1 = min(i0 + 1, in - 1);
    l1 = s - (float)i0;
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void resize_add_kernel(ResizeP p) {
    constexpr int EPC = DT<T>::EPC;
    const T* a = static_cast<const T*>(p.a);
    const T* b = static_cast<const T*>(p.b);
    T* out = static_cast<T*>(p.out);
    const bool fa = p.slope_a != nullptr, fb = p.slope_b != nullptr;
    const float sa = fa ? to_f32(*static_cast<const T*>(p.slope_a)) : 1.f, sb = fb ? to_f32(*static_cast<const T*>(p.slope_b)) : 1.f;
    const float sy = (float)p.Ha / (float)p.Ho, sx = (float)p.Wa / (float)p.Wo;
    const int64_t work = (int64_t)p.B * p.Ho * p.Wo * p.nv;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < work; q += (int64_t)gridDim.x * 256) {
        const int cv = (int)(q % p.nv);
        const int64_t px = q / p.nv;
        const int x = (int)(px % p.Wo);
        const int64_t t = px / p.Wo;
        const int y = (int)(t % p.Ho), bi = (int)(t / p.Ho);
        auto arow = [&](int Y, int X) -> int64_t { return p.a_merge ? merged_row(Y, X, p.Ha / 2, p.Wa / 2) : ((int64_t)bi * p.Ha + Y) * p.Wa + X; };
        const int64_t brow = p.b_merge ? merged_row(y, x, p.Ho / 2, p.Wo / 2) : px;
        const Vec16<T> vb = load16(b + brow * p.ldb + cv * EPC);
        Vec16<T> o;
        if constexpr (MODE == 1) {
            const int Y = min((int)((int64_t)y * p.Ha / p.Ho), p.Ha - 1), X = min((int)((int64_t)x * p.Wa / p.Wo), p.Wa - 1);
            const Vec16<T> va = load16(a + arow(Y, X) * p.lda + cv * EPC);
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, (fa ? prelu_f(va.get(e), sa) : va.get(e)) + (fb ? prelu_f(vb.get(e), sb) : vb.get(e)));
        } else {
            int y0, y1, x0, x1;
            float h1, w1;
            bilinear_axis(y, sy, p.Ha, y0, y1, h1);
            bilinear_axis(x, sx, p.Wa, x0, x1, w1);
            const float h0 = 1.f - h1, w0 = 1.f - w1;
            const Vec16<T> v00 = load16(a + arow(y0, x0) * p.lda + cv * EPC), v01 = load16(a + arow(y0, x1) * p.lda + cv * EPC);
            const Vec16<T> v10 = load16(a + arow(y1, x0) * p.lda + cv * EPC), v11 = load16(a + arow(y1, x1) * p.lda + cv * EPC);
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                float c00 = v00.get(e), c01 = v01.get(e), c10 = v10.get(e), c11 = v11.get(e);
                if (fa) c00 = prelu_f(c00, sa), c01 = prelu_f(c01, sa), c10 = prelu_f(c10, sa), c11 = prelu_f(c11, sa);
                const float r = h0 * (w0 * c00 + w1 * c01) + h1 * (w0 * c10 + w1 * c11);
                o.set(e, r + (fb ? prelu_f(vb.get(e), sb) : vb.get(e)));
            }
        }
        store16(out + px * p.ldo + cv * EPC, o);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ PReLU, views
template <typename T>
__global__ __launch_bounds__(256) void prelu_kernel(T* x, const T* __restrict__ slope, int64_t nvec) {
    constexpr int EPC = DT<T>::EPC;
    const float s = to_f32(slope[0]);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nvec; q += (int64_t)gridDim.x * 256) {
        Vec16<T> v = load16(x + q * EPC);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v.set(e, prelu_f(v.get(e), s));
        store16(x + q * EPC, v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void split_views_kernel(const T* __restrict__ img, T* __restrict__ out, int C, int H, int W) {
    const int h = H / 2, w = W / 2;
    const int64_t plane = (int64_t)h * w, work = 5 * C * plane;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < work; q += (int64_t)gridDim.x * 256) {
        const int x = (int)(q % w);
        const int64_t t = q / w;
        const int y = (int)(t % h);
        const int64_t vc = t / h;
        const int c = (int)(vc % C), v = (int)(vc / C);
        const T* s = img + (int64_t)c * H * W;
        float r;
        if (v < 4) {
            r = to_f32(s[(int64_t)((v >> 1) * h + y) * W + (v & 1) * w + x]);
        } else {
            const T* s0 = s + (int64_t)(2 * y) * W + 2 * x;
            r = 0.5f * (0.5f * to_f32(s0[0]) + 0.5f * to_f32(s0[1])) + 0.5f * (0.5f * to_f32(s0[W]) + 0.5f * to_f32(s0[W + 1]));
        }
        out[q] = from_f32<T>(r);
    }
}

inline bool bad_dtype(int32_t d) { return d != MI355X_F32 && d != MI355X_BF16; }

}  // namespace

extern "C" int mi355x_mvanet_pool(const mi355x_mvanet_pool_args* a, void* stream) {
    if (!a || !a->src || !a->out || a->E < 1 || (a->mode != 0 && a->mode != 1)) return MI355X_EARG;
    if (bad_dtype(a->dtype)) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->S < 1 || (a->mode == 1 && a->S % 2) || a->n_ratios < 1 || a->n_ratios > MI355X_MVANET_MAX_RATIOS) return MI355X_ESHAPE;
    PoolP p;
    p.G = a->mode == 0 ? 2 * a->S : a->S / 2;
    p.base[0] = 0;
    for (int i = 0; i < MI355X_MVANET_MAX_RATIOS; ++i) {
        p.ratio[i] = 1;
        p.base[i + 1] = p.base[i];
        if (i >= a->n_ratios) continue;
        const int r = a->ratio[i];
        if (r < 1 || p.G % r) return MI355X_ESHAPE;
        p.ratio[i] = r;
        p.base[i + 1] = p.base[i] + (p.G / r) * (p.G / r);
    }
    const int groups = a->mode == 0 ? 1 : 4;
    if (a->rows < p.base[a->n_ratios] || a->lds < a->E || a->ldo < a->E || (groups > 1 && a->group_stride < (int64_t)a->rows * a->ldo)) return MI355X_ESHAPE;
    if ((a->E * es) % 16 || (a->lds * es) % 16 || (a->ldo * es) % 16 || (a->group_stride * es) % 16 || !al16(a->src) || !al16(a->out)) return MI355X_ESHAPE;
    const int64_t src_rows = (int64_t)(a->mode == 0 ? 4 : 1) * a->S * a->S;
    const int64_t out_bytes = ((groups - 1) * a->group_stride) * es + span(a->rows, a->ldo, a->E, es);
    if (overlap(a->src, span(src_rows, a->lds, a->E, es), a->out, out_bytes)) return MI355X_EARG;
    p.src = a->src, p.out = a->out, p.lds = a->lds, p.ldo = a->ldo, p.group_stride = a->group_stride;
    p.mode = a->mode, p.S = a->S, p.nv = a->E * es / 16, p.rows = a->rows, p.n = a->n_ratios;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((int64_t)a->rows * p.nv), groups);
    DISPATCH_T(a->dtype, hipLaunchKernelGGL((pool_kernel<T>), grid, dim3(256), 0, st, p));
    return LAUNCH_OK();
}

extern "C" int mi355x_mvanet_gate(const mi355x_mvanet_gate_args* a, void* stream) {
    if (!a || !a->local || !a->glb || !a->w || !a->b || !a->out || a->E < 1) return MI355X_EARG;
    if (bad_dtype(a->dtype)) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->S < 1 || a->ldl < a->E || a->ldg < a->E || a->ldo < a->E) return MI355X_ESHAPE;
    if ((a->ldl * es) % 16 || (a->ldg * es) % 16 || (a->ldo * es) % 16 || !al16(a->local) || !al16(a->glb) || !al16(a->out) || !al(a->w, es) || !al(a->b, es)) return MI355X_ESHAPE;
    const int64_t n = (int64_t)a->S * a->S;
    const int64_t out_bytes = span(4 * n, a->ldo, a->E, es);
    if (overlap(a->glb, span(n, a->ldg, a->E, es), a->out, out_bytes)) return MI355X_EARG;
    if (!(a->out == a->local && a->ldo == a->ldl) && overlap(a->local, span(4 * n, a->ldl, a->E, es), a->out, out_bytes)) return MI355X_EARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + 3) / 4));
    DISPATCH_T(a->dtype, hipLaunchKernelGGL((gate_kernel<T>), grid, dim3(256), 0, st, static_cast<const T*>(a->local), a->ldl, static_cast<const T*>(a->glb), a->ldg,
                                            static_cast<const T*>(a->w), static_cast<const T*>(a->b), static_cast<T*>(a->out), a->ldo, (int)a->S, (int)a->E));
    return LAUNCH_OK();
}

extern "C" int mi355x_mvanet_resize_add(const mi355x_mvanet_resize_add_args* a, void* stream) {
    if (!a || !a->a || !a->b || !a->out || a->E < 1 || (a->mode != 0 && a->mode != 1)) return MI355X_EARG;
    if (bad_dtype(a->dtype)) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B < 1 || a->Ha < 1 || a->Wa < 1 || a->Ho < 1 || a->Wo < 1 || a->lda < a->E || a->ldb < a->E || a->ldo < a->E) return MI355X_ESHAPE;
    if (a->a_merge && (a->B != 1 || a->Ha % 2 || a->Wa % 2)) return MI355X_ESHAPE;
    if (a->b_merge && (a->B != 1 || a->Ho % 2 || a->Wo % 2)) return MI355X_ESHAPE;
    if ((a->E * es) % 16 || (a->lda * es) % 16 || (a->ldb * es) % 16 || (a->ldo * es) % 16 || !al16(a->a) || !al16(a->b) || !al16(a->out)) return MI355X_ESHAPE;
    if ((a->slope_a && !al(a->slope_a, es)) || (a->slope_b && !al(a->slope_b, es))) return MI355X_ESHAPE;
    const int64_t na = (int64_t)a->B * a->Ha * a->Wa, no = (int64_t)a->B * a->Ho * a->Wo;
    const int64_t out_bytes = span(no, a->ldo, a->E, es);
    if (overlap(a->a, span(na, a->lda, a->E, es), a->out, out_bytes)) return MI355X_EARG;
    if (!(a->out == a->b && a->ldo == a->ldb && !a->b_merge) && overlap(a->b, span(no, a->ldb, a->E, es), a->out, out_bytes)) return MI355X_EARG;
    ResizeP p;
    p.a = a->a, p.b = a->b, p.slope_a = a->slope_a, p.slope_b = a->slope_b, p.out = a->out, p.lda = a->lda, p.ldb = a->ldb, p.ldo = a->ldo;
    p.B = a->B, p.nv = a->E * es / 16, p.Ha = a->Ha, p.Wa = a->Wa, p.Ho = a->Ho, p.Wo = a->Wo, p.a_merge = a->a_merge != 0, p.b_merge = a->b_merge != 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(no * p.nv));
    if (a->mode == 0)
        DISPATCH_T(a->dtype, hipLaunchKernelGGL((resize_add_kernel<T, 0>), grid, dim3(256), 0, st, p));
    else
        DISPATCH_T(a->dtype, hipLaunchKernelGGL((resize_add_kernel<T, 1>), grid, dim3(256), 0, st, p));
    return LAUNCH_OK();
}

extern "C" int mi355x_mvanet_prelu(int32_t dtype, void* x, const void* slope, int64_t n, void* stream) {
    if (!x || !slope || n < 1) return MI355X_EARG;
    if (bad_dtype(dtype)) return MI355X_EDTYPE;
    const int es = dtype == MI355X_F32 ? 4 : 2;
    if ((n * es) % 16 || !al16(x) || !al(slope, es)) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t nvec = n * es / 16;
    DISPATCH_T(dtype, hipLaunchKernelGGL((prelu_kernel<T>), dim3(grid_for(nvec)), dim3(256), 0, st, static_cast<T*>(x), static_cast<const T*>(slope), nvec));
    return LAUNCH_OK();
}

extern "C" int mi355x_mvanet_split_views(int32_t dtype, const void* img, void* out, int32_t C, int32_t H, int32_t W, void* stream) {
    if (!img || !out) return MI355X_EARG;
    if (bad_dtype(dtype)) return MI355X_EDTYPE;
    const int es = dtype == MI355X_F32 ? 4 : 2;
    if (C < 1 || H < 1 || W < 1 || H % 2 || W % 2 || !al(img, es) || !al(out, es)) return MI355X_ESHAPE;
    const int64_t n_in = (int64_t)C * H * W, n_out = 5 * (int64_t)C * (H / 2) * (W / 2);
    if (overlap(img, n_in * es, out, n_out * es)) return MI355X_EARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DISPATCH_T(dtype, hipLaunchKernelGGL((split_views_kernel<T>), dim3(grid_for(n_out)), dim3(256), 0, st, static_cast<const T*>(img), static_cast<T*>(out), (int)C, (int)H, (int)W));
    return LAUNCH_OK();
}
