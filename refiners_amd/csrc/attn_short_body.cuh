// attn_short_body.cuh: the short-K/V attention of mi355x_attention's bf16 LDS-DMA kernel (attn_short_dma_kernel, attention.hip) as pieces that a second
// kernel can run: the launch parameters, the loader of one 64-key tile (K rows + V^T rows by LDS-DMA, half-tile rule, zeros beyond Lk) and the tile
// body (Q K^T, base-2 softmax, P V, the close of a stream with its out_scale, the store).  Two kernels include it: attn_short_dma_kernel, which reads Q
// from memory, and the cross-attention form of the 4-wave GEMM (gemm_kernel.cuh, XATTN), whose workgroup has just computed the Q tile it attends with.
// Conventions as in attention.hip: "swapped" orientation (S^T = K Q^T, a lane owns query c16 and 16 of a tile's 64 keys), K rows in k_row_key order,
// V^T rows in the order R = 16 j + 4 a + b <-> d = 16 a + 4 j + b, every tile = 8 KB of K rows followed by 8 KB of V^T rows, 128-byte swizzled rows.
#pragma once
#include <type_traits>

#include "../../include/mi355x_refiners.h"
#include "common.cuh"

namespace mi355x_attn {

struct KvP {
    const char* k;
    const char* vt;
    int64_t ldkb, kbsb;    // bytes
    int64_t ldvtb, vtbsb;  // bytes
    int Lk;
    float out_scale;
};

struct AttnP {
    int B, H, Lq, nstream;
    const char* q;
    int64_t ldqb, qbsb;
    char* out;
    int64_t ldob, obsb;
    float c;  // scale * log2(e)
    float thr;  // OPT bit 2: a tile leaves the running maximum alone while no score exceeds it by more than thr (= 8 / c: P <= 2^8)
    KvP kv[2];
    int qtiles;
    int xcd;  // 1 = XCD-aware block order
};

// mi355x_attn_args -> AttnP with the checks every head-dim-64 entry point makes (0, or the MI355X_E* code of the refusal).  need_q = false: the caller
// produces Q itself (mi355x_gemm_attention), a->q is not looked at.
inline int attn_params(const mi355x_attn_args* a, AttnP& p, bool need_q = true) {
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!a || (need_q && !a->q) || !a->out) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->D != 64 || a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->nstream < 1 || a->nstream > 2) return MI355X_ESHAPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (need_q && (!al16(a->q) || (a->ldq * es) % 16 || (a->q_batch_stride * es) % 16)) return MI355X_ESHAPE;
    if (!al16(a->out) || (a->ldo * es) % 16 || (a->o_batch_stride * es) % 16) return MI355X_ESHAPE;
    p.B = a->B;
    p.H = a->H;
    p.Lq = a->Lq;
    p.nstream = a->nstream;
    p.q = need_q ? static_cast<const char*>(a->q) : nullptr;
    p.ldqb = a->ldq * es;
    p.qbsb = a->q_batch_stride * es;
    p.out = static_cast<char*>(a->out);
    p.ldob = a->ldo * es;
    p.obsb = a->o_batch_stride * es;
    p.c = a->scale * 1.44269504088896340736f;
    p.thr = p.c > 0.f ? 8.0f / p.c : 0.f;
    for (int s = 0; s < a->nstream; ++s) {
        const mi355x_kv_stream& k = a->kv[s];
        if (!k.k || !k.vt || k.Lk <= 0) return MI355X_ESHAPE;
        if (!al16(k.k) || !al16(k.vt) || (k.ldk * es) % 16 || (k.ldvt * es) % 16 || (k.k_batch_stride * es) % 16 || (k.vt_batch_stride * es) % 16) return MI355X_ESHAPE;
        p.kv[s].k = static_cast<const char*>(k.k);
        p.kv[s].vt = static_cast<const char*>(k.vt);
        p.kv[s].ldkb = k.ldk * es;
        p.kv[s].kbsb = k.k_batch_stride * es;
        p.kv[s].ldvtb = k.ldvt * es;
        p.kv[s].vtbsb = k.vt_batch_stride * es;
        p.kv[s].Lk = k.Lk;
        p.kv[s].out_scale = k.out_scale;
    }
    return MI355X_OK;
}

// lane <-> lane ^ 16 and lane <-> lane ^ 32 exchanges as row / half swaps (gfx950): after swap(a = x, b = x), a and b hold the two partners'
// values in every lane.  Inline asm (the builtin form folds the combine of its two results away when both inputs are the same value);
// s_nop 1 = the two wait states a VALU write of an operand needs before the swap reads it.
MI_DEV void xswap16(float& a, float& b) { asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
MI_DEV void xswap32(float& a, float& b) { asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
template <bool PL> MI_DEV float group_max(float x) {
    if constexpr (PL) {
        float a = x, b = x;
        xswap16(a, b);
        a = fmaxf(a, b), b = a;
        xswap32(a, b);
        return fmaxf(a, b);
    } else {
        x = fmaxf(x, __shfl_xor(x, 16));
        return fmaxf(x, __shfl_xor(x, 32));
    }
}
template <bool PL> MI_DEV float group_sum(float x) {
    if constexpr (PL) {
        float a = x, b = x;
        xswap16(a, b);
        a = a + b, b = a;
        xswap32(a, b);
        return a + b;
    } else {
        x += __shfl_xor(x, 16);
        return x + __shfl_xor(x, 32);
    }
}

typedef __amdgpu_buffer_rsrc_t rsrc_t;
MI_DEV rsrc_t make_rsrc(const char* base, int64_t bytes) {  // wave-uniform by construction; readfirstlane makes that provable (otherwise every load sits in a waterfall loop)
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    const int64_t nb = bytes < 0x7ffffff0 ? bytes : 0x7ffffff0;
    const int n = __builtin_amdgcn_readfirstlane((int)nb);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), (short)0, n, 0x00020000);
}
// 16 bytes per lane, global -> LDS: lane i lands at lds_wave_base + 16 i; source = descriptor base + voff (per lane) + soff (scalar); bytes beyond the descriptor's range read as zero
MI_DEV void blds16(rsrc_t rs, char* lds_wave_base, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lptr_t)lds_wave_base, 16, (int)voff, (int)soff, 0, 0);
}

// Geometry of the short kernel: head dim 64, 64-key tiles, bf16, 4 waves
constexpr int SHORT_D = 64, SHORT_BKV = 64, SHORT_ES = 2, SHORT_ROWB = SHORT_D * SHORT_ES, SHORT_CPR = SHORT_ROWB / 16, SHORT_NTHR = 256;
constexpr int SHORT_TILEB = 64 * SHORT_ROWB;    // bytes of a tile's K rows; its V^T rows follow
constexpr int SHORT_SLOTB = 2 * SHORT_TILEB;    // bytes of a whole tile
constexpr int SHORT_SLOTS = 3;                  // tiles over all streams

// NSTREAM: 1 or 2 = the launch's stream count as a constant, 0 = read it from p.nstream
template <int NSTREAM> MI_DEV int short_nstream(const AttnP& p) { return NSTREAM ? NSTREAM : p.nstream; }

// Tile `sl` (counted over all streams; nt0 = tiles of stream 0) of (batch b, head h): LDS-DMA of its K rows to ks and its V^T rows to ks + SHORT_TILEB, issued by
// all 256 threads; the caller waits (vmcnt) and synchronises.  Lanes whose keys lie beyond Lk carry the out-of-range offset, for which the hardware writes zeros
// (K rows, whole 8-key chunks of V^T): nothing beyond Lk is read from memory.  A tile with at most 32 valid keys is a HALF tile: K rows 32 .. 63 are not requested.
template <int NSTREAM>
MI_DEV void attn_short_load_slot(const AttnP& p, int sl, int nt0, char* ks, int b, int h, int tid, int wid) {
    constexpr int D = SHORT_D, BKV = SHORT_BKV, ES = SHORT_ES, ROWB = SHORT_ROWB, CPR = SHORT_CPR, NTHR = SHORT_NTHR, TILEB = SHORT_TILEB;
    constexpr int LI = 64 * CPR / NTHR;
    const int sidx = (short_nstream<NSTREAM>(p) > 1 && sl >= nt0) ? 1 : 0;
    const KvP& kv = p.kv[sidx];
    const int kv0 = (sidx ? sl - nt0 : sl) * BKV;
    const bool half = kv.Lk - kv0 <= 32;
    const rsrc_t krs = make_rsrc(kv.k + (int64_t)b * kv.kbsb + (int64_t)h * ROWB + (int64_t)kv0 * kv.ldkb, (int64_t)63 * kv.ldkb + ROWB);
    const rsrc_t vrs = make_rsrc(kv.vt + (int64_t)h * D * kv.ldvtb + (int64_t)b * kv.vtbsb + (int64_t)kv0 * ES, (int64_t)(D - 1) * kv.ldvtb + BKV * ES);
#pragma unroll
    for (int it = 0; it < LI; ++it) {
        const int q = it * NTHR + tid, row = q / CPR, pch = q % CPR;
        const int cl = pch ^ swz<ROWB>(row);  // the logical chunk this lane's physical slot holds
        const int key = k_row_key(row);       // LDS rows 0 .. 31 hold keys 0 .. 31 of the tile
        if (!(half && it * NTHR >= 32 * CPR)) {  // wave-uniform: a half tile has no second K iteration
            const uint32_t ko = kv0 + key < kv.Lk ? (uint32_t)(key * (int)kv.ldkb + cl * 16) : 0x80000000u;
            blds16(krs, ks + (it * NTHR + wid * 64) * 16, ko, 0);
        }
        const int j = row >> 4, a = (row >> 2) & 3, bb = row & 3;
        const int vrow = 16 * a + 4 * j + bb;
        const uint32_t vo = kv0 + cl * 8 < kv.Lk ? (uint32_t)(vrow * (int)kv.ldvtb + cl * 16) : 0x80000000u;
        blds16(vrs, ks + TILEB + (it * NTHR + wid * 64) * 16, vo, 0);
    }
}

// The wave's 16 NJQ queries q0 .. of (batch b, head h) against every tile of every stream, then the store.  qf: the queries' fragments (chunk 4 s + g of row
// 16 jq + c16); slot(sl): the LDS address tile sl was loaded to.  The tiles must have landed and be visible to the wave.
template <int NSTREAM, int NJQ, typename SlotFn>
MI_DEV void attn_short_tiles(const AttnP& p, SlotFn slot, const frag_t (&qf)[NJQ][2], int b, int h, int q0, int lane) {
    using T = bf16_t;
    constexpr int BKV = SHORT_BKV, ROWB = SHORT_ROWB, TILEB = SHORT_TILEB, SLOTS = SHORT_SLOTS, NS = 2;
    const int g = lane >> 4, c16 = lane & 15;
    const int nstream = short_nstream<NSTREAM>(p);
    const int nt0 = (p.kv[0].Lk + BKV - 1) / BKV;
    const int nt1 = nstream > 1 ? (p.kv[1].Lk + BKV - 1) / BKV : 0;
    const int ntot = nt0 + nt1;  // <= SLOTS (checked by the host)

    f32x4 res[4][NJQ], o[4][NJQ];
    float mrun[NJQ], lsum[NJQ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jq = 0; jq < NJQ; ++jq) res[i][jq] = f32x4{0.f, 0.f, 0.f, 0.f}, o[i][jq] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jq = 0; jq < NJQ; ++jq) mrun[jq] = -INFINITY, lsum[jq] = 0.f;

    auto finish = [&](float out_scale) {
#pragma unroll
        for (int jq = 0; jq < NJQ; ++jq) {
            const float l = group_sum<true>(lsum[jq]);
            const float inv = out_scale / l;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                res[i][jq] += o[i][jq] * inv;
                o[i][jq] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            mrun[jq] = -INFINITY, lsum[jq] = 0.f;
        }
    };

    auto tile = [&](const char* ks, int kv0, int Lk, auto halfc) {
        constexpr int TT = decltype(halfc)::value ? 2 : 4;  // 16-key blocks of the tile that hold valid keys
        const char* vs = ks + TILEB;
        f32x4 st[TT][NJQ];
#pragma unroll
        for (int t = 0; t < TT; ++t) {
#pragma unroll
            for (int jq = 0; jq < NJQ; ++jq) st[t][jq] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const frag_t kf = lds_read_frag(ks, tile_off<ROWB>(16 * t + c16, 4 * s + g));
#pragma unroll
                for (int jq = 0; jq < NJQ; ++jq) mma_step<T>(st[t][jq], kf, qf[jq][s]);
            }
        }
        if (kv0 + BKV > Lk) {
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (kv0 + k_row_key(16 * t + 4 * g + r) >= Lk) {
#pragma unroll
                        for (int jq = 0; jq < NJQ; ++jq) st[t][jq][r] = -INFINITY;
                    }
                }
        }
#pragma unroll
        for (int jq = 0; jq < NJQ; ++jq) {
            float mx = st[0][jq][0];
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[t][jq][r]);
            mx = group_max<true>(mx);
            const float mnew = fmaxf(mrun[jq], mx);
            const float alpha = fast_exp2((mrun[jq] - mnew) * p.c);
            const float mc = mnew * p.c;
            float ps = 0.f;
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = fast_exp2(st[t][jq][r] * p.c - mc);
                    st[t][jq][r] = e;
                    ps += e;
                }
            lsum[jq] = lsum[jq] * alpha + ps;
            mrun[jq] = mnew;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i][jq] *= alpha;
        }
#pragma unroll
        for (int s2 = 0; s2 < TT / 2; ++s2) {
            frag_t pb[NJQ];
#pragma unroll
            for (int jq = 0; jq < NJQ; ++jq) {
                bf16x8 pk;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pk[r] = (bf16_t)st[2 * s2][jq][r];
                    pk[4 + r] = (bf16_t)st[2 * s2 + 1][jq][r];
                }
                pb[jq] = __builtin_bit_cast(frag_t, pk);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const frag_t vf = lds_read_frag(vs, tile_off<ROWB>(16 * i + c16, 4 * s2 + g));
#pragma unroll
                for (int jq = 0; jq < NJQ; ++jq) mma_step<T>(o[i][jq], vf, pb[jq]);
            }
        }
    };

#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        if (sl < ntot) {
            const int sidx = (nstream > 1 && sl >= nt0) ? 1 : 0;
            if (nstream > 1 && sl == nt0) finish(p.kv[0].out_scale);  // first tile of the second stream: close the first
            const int Lk = p.kv[sidx].Lk;
            const int kv0 = (sidx ? sl - nt0 : sl) * BKV;
            if (Lk - kv0 <= 32) tile(slot(sl), kv0, Lk, std::true_type{});
            else tile(slot(sl), kv0, Lk, std::false_type{});
        }
    }
    finish(nstream > 1 ? p.kv[1].out_scale : p.kv[0].out_scale);

    // ---- store: lane owns d = 16 g .. 16 g + 15 of query 16 jq + c16 ----
#pragma unroll
    for (int jq = 0; jq < NJQ; ++jq) {
        const int qr = q0 + 16 * jq + c16;
        if (qr >= p.Lq) continue;
        T* op = reinterpret_cast<T*>(p.out + (int64_t)b * p.obsb + (int64_t)qr * p.ldob + (int64_t)h * ROWB) + 16 * g;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            Vec16<T> ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov.set(e, res[(c * 8 + e) >> 2][jq][e & 3]);
            store16<T>(op + c * 8, ov);
        }
    }
}

}  // namespace mi355x_attn
