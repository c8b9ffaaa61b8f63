// Swin Transformer window attention (src/refiners/foundationals/swin/swin_transformer.py:42-66, 148-203): softmax(scale Q K^T + relative
// position bias + shift mask) V per (window, head), N = ws^2 <= 144 tokens, head dim 32.  float32 arithmetic (f32 MFMA for float32
// storage, bf16 MFMA with float32 accumulation and softmax for bfloat16); every output is written by exactly one lane, no atomics.
#include "common.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_swin.h"

namespace {

constexpr int WA_D = 32;             // head dim
constexpr int WA_NMAX = 144;         // tokens per window (ws <= 12)
constexpr int WA_NB = WA_NMAX / 16;  // 16-token blocks
constexpr int WA_TMAX = 23 * 23;     // (2 ws - 1)^2 table rows
constexpr int WA_INFO = 160;         // per-token words, padded to the bf16 key count

template <typename T> struct WA;
template <> struct WA<float> {
    static constexpr int NWAVE = 2;   // heads per workgroup
    static constexpr int KP = 144;    // key positions of a V^T row
    static constexpr int VROW = 592;  // bytes per V^T row: 576 + 16, an ODD number of 16-byte slots (16 rows at one chunk: 16 distinct slots)
    static constexpr int KS = 2;      // MMA steps over the 32 channels
};
template <> struct WA<bf16_t> {
    static constexpr int NWAVE = 4;
    static constexpr int KP = 160;    // 5 MFMA steps of 32 keys
    static constexpr int VROW = 336;  // 320 + 16
    static constexpr int KS = 1;
};

// Position of key `key` in a V^T row.  float32: natural order (MMA step t = keys 16 t .. 16 t + 15, lane group g takes 4 g .. 4 g + 3, which
// are exactly the keys whose probabilities it holds after S^T = K Q^T).  bfloat16: one step spans the key blocks 2 s and 2 s + 1 and lane
// group g holds keys 4 g + r of BOTH, so those eight are made consecutive: position 32 s + 8 g + 4 (block & 1) + r.
template <typename T> MI_DEV int key_pos(int key) {
    if constexpr (sizeof(T) == 4) return key;
    else return (key & ~31) + 8 * ((key >> 2) & 3) + 4 * ((key >> 4) & 1) + (key & 3);
}

// grid (nW, ceil(H / NWAVE)), NWAVE waves: wave v serves head blockIdx.y * NWAVE + v of window blockIdx.x.
//   prologue  the bias-table columns of the workgroup's heads and one word per token (y (2 ws - 1) + x | region id << 16) into LDS; each wave
//             transposes its head's V into LDS (zeros for keys >= N) and keeps its head's K fragments in registers
//   per 16-query block: S^T = K Q^T (lane: query c16, keys 16 t + 4 g + r), + bias + mask, two-pass softmax over the lane's 36 scores and the
//             four lane groups, O^T = V^T P^T (lane: query c16, channels 4 g + r and 16 + 4 g + r), one vector store per half
template <typename T>
__global__ __launch_bounds__(WA<T>::NWAVE * 64) void window_attention_kernel(mi355x_window_attention_args a) {
    using W = WA<T>;
    constexpr int EPC = DT<T>::EPC;
    __shared__ __attribute__((aligned(16))) char vt[W::NWAVE * WA_D * W::VROW];
    __shared__ float tbl[W::NWAVE][WA_TMAX + 3];
    __shared__ __attribute__((aligned(16))) int info[WA_INFO];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int w = blockIdx.x, h0 = blockIdx.y * W::NWAVE, h = h0 + wv;
    const int ws = a.ws, N = ws * ws, R = 2 * ws - 1, TT = R * R;
    for (int i = tid; i < W::NWAVE * TT; i += W::NWAVE * 64) {
        const int hl = i % W::NWAVE, idx = i / W::NWAVE;
        tbl[hl][idx] = h0 + hl < a.H ? a.table[(int64_t)idx * a.H + h0 + hl] : 0.f;
    }
    for (int k = tid; k < WA_INFO; k += W::NWAVE * 64) {
        const int y = k / ws, x = k - y * ws;
        int reg = 0;
        if (a.shift > 0) {
            const int wi = w % (a.nw * a.nw), wy = wi / a.nw, wx = wi - wy * a.nw;
            const int ry = wy == a.nw - 1 ? (y < ws - a.shift ? 1 : 2) : 0;
            const int rx = wx == a.nw - 1 ? (x < ws - a.shift ? 1 : 2) : 0;
            reg = 3 * ry + rx;
        }
        info[k] = k < N ? ((y * R + x) | (reg << 16)) : 0;
    }
    char* myvt = vt + wv * WA_D * W::VROW;
    if (h < a.H) {
        const T* vb = static_cast<const T*>(a.v) + (int64_t)w * a.v_win_stride + (int64_t)h * WA_D;
        for (int key = lane; key < W::KP; key += 64) {
            T* dst = reinterpret_cast<T*>(myvt) + key_pos<T>(key);
#pragma unroll
            for (int c = 0; c < WA_D / EPC; ++c) {
                Vec16<T> x{};
                if (key < N) x = load16(vb + (int64_t)key * a.ldv + c * EPC);
#pragma unroll
                for (int e = 0; e < EPC; ++e) dst[(c * EPC + e) * (W::VROW / (int)sizeof(T))] = key < N ? from_f32<T>(x.get(e)) : from_f32<T>(0.f);
            }
        }
    }
    __syncthreads();
    if (h >= a.H) return;

    const int nb = (N + 15) >> 4;  // 16-token blocks in use
    const T* kb = static_cast<const T*>(a.k) + (int64_t)w * a.k_win_stride + (int64_t)h * WA_D;
    const T* qb = static_cast<const T*>(a.q) + (int64_t)w * a.q_win_stride + (int64_t)h * WA_D;
    T* ob = static_cast<T*>(a.out) + (int64_t)w * a.o_win_stride + (int64_t)h * WA_D;
    const frag_t zero = {0, 0, 0, 0};
    frag_t kf[WA_NB][W::KS];
#pragma unroll
    for (int t = 0; t < WA_NB; ++t) {
        const int key = 16 * t + c16;
#pragma unroll
        for (int u = 0; u < W::KS; ++u)
            kf[t][u] = key < N ? *reinterpret_cast<const frag_t*>(kb + (int64_t)key * a.ldk + (4 * u + g) * EPC) : zero;
    }
    const float* tb = tbl[wv];
    const float scale = a.scale;
    for (int qblk = 0; qblk < nb; ++qblk) {
        const int qi = 16 * qblk + c16;
        frag_t qf[W::KS];
#pragma unroll
        for (int u = 0; u < W::KS; ++u) qf[u] = qi < N ? *reinterpret_cast<const frag_t*>(qb + (int64_t)qi * a.ldq + (4 * u + g) * EPC) : zero;
        const int qinfo = info[qi];
        const int qterm = (qinfo & 0xffff) + (ws - 1) * R + (ws - 1), qreg = qinfo >> 16;
        f32x4 s[WA_NB];
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < WA_NB; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t < nb) {
#pragma unroll
                for (int u = 0; u < W::KS; ++u) mma_step<T>(s[t], kf[t][u], qf[u]);
                const int4 ki = *reinterpret_cast<const int4*>(&info[16 * t + 4 * g]);
                const int kis[4] = {ki.x, ki.y, ki.z, ki.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float val = fmaf(s[t][r], scale, tb[qterm - (kis[r] & 0xffff)]) + ((kis[r] >> 16) != qreg ? -100.f : 0.f);
                    val = 16 * t + 4 * g + r < N ? val : -INFINITY;
                    s[t][r] = val;
                    m = fmaxf(m, val);
                }
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float l = 0.f;
#pragma unroll
        for (int t = 0; t < WA_NB; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = t < nb ? __expf(s[t][r] - m) : 0.f;  // (a key >= N: exp(-inf) = 0)
                s[t][r] = p;
                l += p;
            }
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int t = 0; t < WA_NB; ++t) {
                if (t < nb) {
                    const frag_t p = __builtin_bit_cast(frag_t, s[t]);
                    mma_step<T>(o0, lds_read_frag(myvt, c16 * W::VROW + (4 * t + g) * 16), p);
                    mma_step<T>(o1, lds_read_frag(myvt, (16 + c16) * W::VROW + (4 * t + g) * 16), p);
                }
            }
        } else {
#pragma unroll
            for (int st = 0; st < (WA_NB + 1) / 2; ++st) {
                if (2 * st < nb) {
                    bf16x8 pv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pv[r] = (bf16_t)s[2 * st][r];
                        pv[4 + r] = 2 * st + 1 < WA_NB ? (bf16_t)s[2 * st + 1 < WA_NB ? 2 * st + 1 : 0][r] : (bf16_t)0.f;
                    }
                    const frag_t p = __builtin_bit_cast(frag_t, pv);
                    mma_step<T>(o0, lds_read_frag(myvt, c16 * W::VROW + (4 * st + g) * 16), p);
                    mma_step<T>(o1, lds_read_frag(myvt, (16 + c16) * W::VROW + (4 * st + g) * 16), p);
                }
            }
        }
        if (qi < N) {
            const float inv = 1.f / l;
            T* orow = ob + (int64_t)qi * a.ldo + 4 * g;
            if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<f32x4*>(orow) = o0 * inv;
                *reinterpret_cast<f32x4*>(orow + 16) = o1 * inv;
            } else {
                bf16x4 v0, v1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v0[r] = (bf16_t)(o0[r] * inv);
                    v1[r] = (bf16_t)(o1[r] * inv);
                }
                *reinterpret_cast<bf16x4*>(orow) = v0;
                *reinterpret_cast<bf16x4*>(orow + 16) = v1;
            }
        }
    }
}

inline bool wa_aligned(const void* p, int64_t ld_elems, int64_t win_elems, int es, int bytes) {
    return reinterpret_cast<uintptr_t>(p) % bytes == 0 && (ld_elems * es) % bytes == 0 && (win_elems * es) % bytes == 0;
}

}  // namespace

extern "C" int mi355x_window_attention(const mi355x_window_attention_args* a, void* stream) {
    if (!a || !a->q || !a->k || !a->v || !a->table || !a->out || a->nW <= 0 || a->H <= 0) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->ws < 1 || a->ws * a->ws > WA_NMAX || a->shift < 0 || a->shift >= a->ws) return MI355X_ESHAPE;
    if (a->shift > 0 && (a->nw < 1 || a->nw > 32768 || a->nW % (a->nw * a->nw))) return MI355X_ESHAPE;
    const int64_t hd = (int64_t)a->H * WA_D;
    if (a->ldq < hd || a->ldk < hd || a->ldv < hd || a->ldo < hd) return MI355X_ESHAPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (!wa_aligned(a->q, a->ldq, a->q_win_stride, es, 16) || !wa_aligned(a->k, a->ldk, a->k_win_stride, es, 16) || !wa_aligned(a->v, a->ldv, a->v_win_stride, es, 16) ||
        !wa_aligned(a->out, a->ldo, a->o_win_stride, es, 4 * es))
        return MI355X_ESHAPE;
    const int nwave = a->dtype == MI355X_F32 ? WA<float>::NWAVE : WA<bf16_t>::NWAVE;
    const int groups = (a->H + nwave - 1) / nwave;
    if (groups > 65535) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(a->nW, groups);
    if (a->dtype == MI355X_F32) hipLaunchKernelGGL((window_attention_kernel<float>), grid, dim3(nwave * 64), 0, st, *a);
    else hipLaunchKernelGGL((window_attention_kernel<bf16_t>), grid, dim3(nwave * 64), 0, st, *a);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}
