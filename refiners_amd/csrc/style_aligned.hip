// StyleAligned shared self-attention (style_aligned.py:15-282 of the reference): per-(sample, channel) AdaIN statistics over the tokens, and the
// kernel pair that applies AdaIN to Q / K and packs [AdaIN(K_b) ; s_b K_r(b)] rows and [V_b^T | s_b V_r(b)^T] columns for a 2L-key attention launch.
// All HBM-streaming: 16-byte vectors per lane, a thread owns one 16-byte channel chunk over a strip of tokens, float32 arithmetic, one rounding at the
// store.  No float atomics anywhere: the statistics are (count, mean, M2) triples merged in a fixed order (row lane order inside a workgroup through
// LDS, slab order across workgroups through a scratch table), so replays are bit-equal.
#include "common.cuh"
#include "../../include/mi355x_refiners.h"

namespace {

constexpr int SA_CT = 16;     // 16-byte channel chunks per workgroup column tile (256 contiguous bytes per row: two 128-byte segments)
constexpr int SA_RL = 16;     // rows a workgroup touches at once (256 threads = 16 chunks x 16 row lanes)
constexpr int SA_ROWS = 128;  // rows per workgroup of the Q / K apply kernel (8 per thread: the statistics a thread holds are amortised over them)

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)

// Slabs of the token axis: rows per slab (a multiple of SA_RL, at least 64), about 256 (sample, slab) pairs per column tile.  Depends on (B, L) ONLY:
// neither the dtype nor the channel count moves the slab boundaries, so a channel's statistics are the same bits whether it is reduced as part of a
// packed Q|K buffer or of a separate one, and the scratch size is known without the dtype.
inline int slab_rows(int B, int L, int* S) {
    int64_t want = 256 / B;
    if (want < 1) want = 1;
    int64_t ls = (L + want - 1) / want;
    if (ls < 64) ls = 64;
    ls = (ls + SA_RL - 1) / SA_RL * SA_RL;
    *S = (int)((L + ls - 1) / ls);
    return (int)ls;
}

// Chan et al.: (na, ma, M2a) <- merge with (nb, mb, M2b)
MI_DEV void chan_merge(float& na, float& ma, float& m2a, float nb, float mb, float m2b) {
    if (nb == 0.f) return;
    const float nt = na + nb, d = mb - ma, w = nb / nt;
    ma = fmaf(d, w, ma);
    m2a += m2b + d * d * na * w;
    na = nt;
}

// grid (column tiles, slabs, B).  Thread (chunk ch, row lane rl) runs Welford over rows r0 + rl, r0 + rl + 16, ... of its slab for the EPC channels of
// its chunk; the 16 row lanes of a chunk are merged in lane order by one thread per channel.  final != 0 (one slab): (mean, std) straight to stats.
template <typename T>
__global__ __launch_bounds__(256) void adain_stats_kernel(const T* __restrict__ x, int64_t ldx, int64_t xbs, int L, int C, int Ls, int S,
                                                           float* __restrict__ ws, float* __restrict__ stats, int final) {
    constexpr int EPC = DT<T>::EPC;
    __shared__ float sm_mean[SA_RL][SA_CT * EPC];
    __shared__ float sm_m2[SA_RL][SA_CT * EPC];
    const int ch = threadIdx.x & (SA_CT - 1), rl = threadIdx.x >> 4;
    const int b = blockIdx.z, s = blockIdx.y;
    const int c0 = (blockIdx.x * SA_CT + ch) * EPC;
    const int r0 = s * Ls, r1 = min(L, r0 + Ls);
    float mean[EPC], m2[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) mean[e] = 0.f, m2[e] = 0.f;
    if (c0 < C) {
        const T* col = x + (int64_t)b * xbs + c0;
        int n = 0;
        for (int r = r0 + rl; r < r1; r += 4 * SA_RL) {
            Vec16<T> v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r + u * SA_RL < r1) v[u] = load16(col + (int64_t)(r + u * SA_RL) * ldx);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (r + u * SA_RL < r1) {
                    n += 1;
                    const float inv = 1.0f / (float)n;
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        const float t = v[u].get(e), d = t - mean[e];
                        mean[e] = fmaf(d, inv, mean[e]);
                        m2[e] = fmaf(d, t - mean[e], m2[e]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        sm_mean[rl][ch * EPC + e] = mean[e];
        sm_m2[rl][ch * EPC + e] = m2[e];
    }
    __syncthreads();
    const int t = threadIdx.x;
    const int c = blockIdx.x * SA_CT * EPC + t;
    if (t < SA_CT * EPC && c < C) {
        float na = 0.f, ma = 0.f, m2a = 0.f;
        for (int l = 0; l < SA_RL; ++l) {
            const int rows = r0 + l < r1 ? (r1 - r0 - l + SA_RL - 1) / SA_RL : 0;  // what row lane l counted
            chan_merge(na, ma, m2a, (float)rows, sm_mean[l][t], sm_m2[l][t]);
        }
        if (final) {
            float* o = stats + ((int64_t)b * C + c) * 2;
            o[0] = ma;
            o[1] = sqrtf(m2a / (float)(L - 1));
        } else {
            float* o = ws + (((int64_t)b * S + s) * C + c) * 2;
            o[0] = ma;
            o[1] = m2a;
        }
    }
}

// one thread per (sample, channel): the S slab triples in slab order -> (mean, unbiased std)
__global__ __launch_bounds__(256) void adain_stats_merge_kernel(const float* __restrict__ ws, float* __restrict__ stats, int B, int L, int C, int Ls, int S) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * C) return;
    const int b = (int)(i / C), c = (int)(i - (int64_t)b * C);
    float na = 0.f, ma = 0.f, m2a = 0.f;
    for (int s = 0; s < S; ++s) {
        const f32x2 p = *reinterpret_cast<const f32x2*>(ws + (((int64_t)b * S + s) * C + c) * 2);
        chan_merge(na, ma, m2a, (float)(min(L, (s + 1) * Ls) - s * Ls), p[0], p[1]);
    }
    f32x2 o;
    o[0] = ma;
    o[1] = sqrtf(m2a / (float)(L - 1));
    *reinterpret_cast<f32x2*>(stats + i * 2) = o;
}

struct PackP {
    int B, L, C, n;
    char* q;
    const char* k;
    const char* vt;
    char* k_sh;
    char* vt_sh;
    int64_t ldq, qbs, ldk, kbs, ldvt, vtbs, ld_ksh, kshbs, ld_vtsh, vtshbs, sbs;
    const float* q_stats;
    const float* k_stats;
    const float* scale;
    float eps;
};

// grid (column tiles, ceil(L / SA_ROWS), B).  A thread holds the AdaIN coefficients of its EPC channels for Q and K and streams 8 rows:
// q in place, AdaIN(k) to rows [0, L) of k_sh, s_b * k_r(b) to rows [L, 2 L).
template <typename T>
__global__ __launch_bounds__(256) void style_aligned_qk_kernel(PackP p) {
    constexpr int EPC = DT<T>::EPC;
    const int ch = threadIdx.x & (SA_CT - 1), rl = threadIdx.x >> 4;
    const int b = blockIdx.z;
    const int c0 = (blockIdx.x * SA_CT + ch) * EPC;
    if (c0 >= p.C) return;
    const int r = b / p.n * p.n;
    const bool own = b == r;
    const float s = own ? 1.0f : p.scale[0];
    float qm[EPC], qa[EPC], qr[EPC], km[EPC], ka[EPC], kr[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const f32x2 qb = *reinterpret_cast<const f32x2*>(p.q_stats + b * p.sbs + (int64_t)(c0 + e) * 2);
        const f32x2 qf = *reinterpret_cast<const f32x2*>(p.q_stats + r * p.sbs + (int64_t)(c0 + e) * 2);
        const f32x2 kb = *reinterpret_cast<const f32x2*>(p.k_stats + b * p.sbs + (int64_t)(c0 + e) * 2);
        const f32x2 kf = *reinterpret_cast<const f32x2*>(p.k_stats + r * p.sbs + (int64_t)(c0 + e) * 2);
        qm[e] = qb[0], qa[e] = qf[1] / (qb[1] + p.eps), qr[e] = qf[0];
        km[e] = kb[0], ka[e] = kf[1] / (kb[1] + p.eps), kr[e] = kf[0];
    }
    T* q = reinterpret_cast<T*>(p.q) + (int64_t)b * p.qbs + c0;
    const T* k = reinterpret_cast<const T*>(p.k) + (int64_t)b * p.kbs + c0;
    const T* kref = reinterpret_cast<const T*>(p.k) + (int64_t)r * p.kbs + c0;
    T* ko = reinterpret_cast<T*>(p.k_sh) + (int64_t)b * p.kshbs + c0;
    const int row0 = blockIdx.y * SA_ROWS + rl;
#pragma unroll 2
    for (int i = 0; i < SA_ROWS / SA_RL; i += 2) {
        Vec16<T> vq[2], vk[2], vr[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = row0 + (i + u) * SA_RL;
            if (row < p.L) {
                vq[u] = load16(q + (int64_t)row * p.ldq);
                vk[u] = load16(k + (int64_t)row * p.ldk);
                vr[u] = own ? vk[u] : load16(kref + (int64_t)row * p.ldk);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = row0 + (i + u) * SA_RL;
            if (row < p.L) {
                Vec16<T> oq, ok, orf;
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    oq.set(e, fmaf(vq[u].get(e) - qm[e], qa[e], qr[e]));
                    ok.set(e, fmaf(vk[u].get(e) - km[e], ka[e], kr[e]));
                    orf.set(e, s * vr[u].get(e));
                }
                store16(q + (int64_t)row * p.ldq, oq);
                store16(ko + (int64_t)row * p.ld_ksh, ok);
                store16(ko + (int64_t)(p.L + row) * p.ld_ksh, own ? vr[u] : orf);
            }
        }
    }
}

// V^T rows: one thread per (channel, sample, 16-byte chunk of the L columns), grid-stride
template <typename T>
__global__ __launch_bounds__(256) void style_aligned_vt_kernel(PackP p) {
    constexpr int EPC = DT<T>::EPC;
    const int JC = p.L / EPC;
    const int64_t total = (int64_t)p.C * p.B * JC;
    const float sc = p.scale[0];
    const T* vt = reinterpret_cast<const T*>(p.vt);
    T* out = reinterpret_cast<T*>(p.vt_sh);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i % JC);
        const int64_t row = i / JC;
        const int b = (int)(row % p.B), c = (int)(row / p.B);
        const int r = b / p.n * p.n;
        const Vec16<T> v = load16(vt + c * p.ldvt + b * p.vtbs + (int64_t)j * EPC);
        T* o = out + c * p.ld_vtsh + b * p.vtshbs + (int64_t)j * EPC;
        store16(o, v);
        if (b == r) {
            store16(o + p.L, v);
        } else {
            const Vec16<T> w = load16(vt + c * p.ldvt + r * p.vtbs + (int64_t)j * EPC);
            Vec16<T> ow;
#pragma unroll
            for (int e = 0; e < EPC; ++e) ow.set(e, sc * w.get(e));
            store16(o + p.L, ow);
        }
    }
}

// the same, element by element: token counts / strides that are not a multiple of 16 bytes (small latents only)
template <typename T>
__global__ __launch_bounds__(256) void style_aligned_vt_scalar_kernel(PackP p) {
    const int64_t total = (int64_t)p.C * p.B * p.L;
    const float sc = p.scale[0];
    const T* vt = reinterpret_cast<const T*>(p.vt);
    T* out = reinterpret_cast<T*>(p.vt_sh);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i % p.L);
        const int64_t row = i / p.L;
        const int b = (int)(row % p.B), c = (int)(row / p.B);
        const int r = b / p.n * p.n;
        T* o = out + c * p.ld_vtsh + b * p.vtshbs + j;
        o[0] = vt[c * p.ldvt + b * p.vtbs + j];
        const T w = vt[c * p.ldvt + r * p.vtbs + j];
        o[p.L] = b == r ? w : from_f32<T>(sc * to_f32(w));
    }
}

inline int grid_for(int64_t work, int cap = 8192) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" int64_t mi355x_adain_stats_ws_floats(int32_t B, int32_t L, int32_t C) {
    if (B <= 0 || L <= 0 || C <= 0) return 0;
    int S = 1;
    slab_rows(B, L, &S);
    return S > 1 ? (int64_t)B * S * C * 2 : 0;
}

extern "C" int mi355x_adain_stats(const mi355x_adain_stats_args* a, void* stream) {
    if (!a || !a->x || !a->stats) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2, epc = 16 / es;
    if (a->B <= 0 || a->L < 2 || a->C <= 0 || a->C % epc || a->ldx < a->C) return MI355X_ESHAPE;
    if (!al16(a->x) || (a->ldx * es) % 16 || (a->x_batch_stride * es) % 16 || (reinterpret_cast<uintptr_t>(a->stats) & 7)) return MI355X_ESHAPE;
    int S = 1;
    const int Ls = slab_rows(a->B, a->L, &S);
    if (S > 1 && (!a->ws || a->ws_floats < (int64_t)a->B * S * a->C * 2 || (reinterpret_cast<uintptr_t>(a->ws) & 7))) return MI355X_EARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((a->C / epc + SA_CT - 1) / SA_CT, S, a->B);
    if (a->dtype == MI355X_F32)
        hipLaunchKernelGGL((adain_stats_kernel<float>), grid, dim3(256), 0, st, static_cast<const float*>(a->x), a->ldx, a->x_batch_stride, a->L, a->C, Ls, S,
                           a->ws, a->stats, S == 1);
    else
        hipLaunchKernelGGL((adain_stats_kernel<bf16_t>), grid, dim3(256), 0, st, static_cast<const bf16_t*>(a->x), a->ldx, a->x_batch_stride, a->L, a->C, Ls, S,
                           a->ws, a->stats, S == 1);
    if (S > 1)
        hipLaunchKernelGGL(adain_stats_merge_kernel, dim3(grid_for((int64_t)a->B * a->C, 1 << 20)), dim3(256), 0, st, a->ws, a->stats, a->B, a->L, a->C, Ls, S);
    return LAUNCH_OK();
}

extern "C" int mi355x_style_aligned_pack(const mi355x_style_aligned_args* a, void* stream) {
    if (!a || !a->q || !a->k || !a->vt || !a->q_stats || !a->k_stats || !a->scale || !a->k_sh || !a->vt_sh) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2, epc = 16 / es;
    if (a->B <= 0 || a->L <= 0 || a->C <= 0 || a->n <= 0 || a->B % a->n || a->C % epc) return MI355X_ESHAPE;
    if (a->ldq < a->C || a->ldk < a->C || a->ld_ksh < a->C || a->ldvt < a->L || a->ld_vtsh < 2 * (int64_t)a->L) return MI355X_ESHAPE;
    if (a->B > 1 && (a->vt_batch_stride < a->L || a->vtsh_batch_stride < 2 * (int64_t)a->L || a->ksh_batch_stride < 2 * (int64_t)a->L * a->ld_ksh)) return MI355X_ESHAPE;
    if (!al16(a->q) || !al16(a->k) || !al16(a->k_sh) || a->ldq % epc || a->q_batch_stride % epc || a->ldk % epc || a->k_batch_stride % epc ||
        a->ld_ksh % epc || a->ksh_batch_stride % epc || (reinterpret_cast<uintptr_t>(a->q_stats) & 7) || (reinterpret_cast<uintptr_t>(a->k_stats) & 7) ||
        a->stats_batch_stride % 2)
        return MI355X_ESHAPE;
    // the packed buffers are written while other workgroups still read the raw keys / values of the reference rows: no overlap allowed
    auto span = [es](const void* base, int64_t batches, int64_t bstride, int64_t rows, int64_t ld, int64_t cols, uintptr_t* lo, uintptr_t* hi) {
        *lo = reinterpret_cast<uintptr_t>(base);
        *hi = *lo + (uintptr_t)(((batches - 1) * bstride + (rows - 1) * ld + cols) * es);
    };
    uintptr_t k0, k1, s0, s1, v0, v1, t0, t1;
    span(a->k, a->B, a->k_batch_stride, a->L, a->ldk, a->C, &k0, &k1);
    span(a->k_sh, a->B, a->ksh_batch_stride, 2 * (int64_t)a->L, a->ld_ksh, a->C, &s0, &s1);
    span(a->vt, a->B, a->vt_batch_stride, a->C, a->ldvt, a->L, &v0, &v1);
    span(a->vt_sh, a->B, a->vtsh_batch_stride, a->C, a->ld_vtsh, 2 * (int64_t)a->L, &t0, &t1);
    if ((k0 < s1 && s0 < k1) || (v0 < t1 && t0 < v1)) return MI355X_EARG;
    PackP p{};
    p.B = a->B, p.L = a->L, p.C = a->C, p.n = a->n;
    p.q = static_cast<char*>(a->q), p.k = static_cast<const char*>(a->k), p.vt = static_cast<const char*>(a->vt);
    p.k_sh = static_cast<char*>(a->k_sh), p.vt_sh = static_cast<char*>(a->vt_sh);
    p.ldq = a->ldq, p.qbs = a->q_batch_stride, p.ldk = a->ldk, p.kbs = a->k_batch_stride, p.ldvt = a->ldvt, p.vtbs = a->vt_batch_stride;
    p.ld_ksh = a->ld_ksh, p.kshbs = a->ksh_batch_stride, p.ld_vtsh = a->ld_vtsh, p.vtshbs = a->vtsh_batch_stride, p.sbs = a->stats_batch_stride;
    p.q_stats = a->q_stats, p.k_stats = a->k_stats, p.scale = a->scale, p.eps = a->eps;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((a->C / epc + SA_CT - 1) / SA_CT, (a->L + SA_ROWS - 1) / SA_ROWS, a->B);
    const bool vec = al16(a->vt) && al16(a->vt_sh) && a->L % epc == 0 && a->ldvt % epc == 0 && a->vt_batch_stride % epc == 0 && a->ld_vtsh % epc == 0 &&
                     a->vtsh_batch_stride % epc == 0;
    const int64_t vt_work = (int64_t)a->C * a->B * (vec ? a->L / epc : a->L);
    if (a->dtype == MI355X_F32) {
        hipLaunchKernelGGL((style_aligned_qk_kernel<float>), grid, dim3(256), 0, st, p);
        if (vec) hipLaunchKernelGGL((style_aligned_vt_kernel<float>), dim3(grid_for(vt_work)), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((style_aligned_vt_scalar_kernel<float>), dim3(grid_for(vt_work)), dim3(256), 0, st, p);
    } else {
        hipLaunchKernelGGL((style_aligned_qk_kernel<bf16_t>), grid, dim3(256), 0, st, p);
        if (vec) hipLaunchKernelGGL((style_aligned_vt_kernel<bf16_t>), dim3(grid_for(vt_work)), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((style_aligned_vt_scalar_kernel<bf16_t>), dim3(grid_for(vt_work)), dim3(256), 0, st, p);
    }
    return LAUNCH_OK();
}
