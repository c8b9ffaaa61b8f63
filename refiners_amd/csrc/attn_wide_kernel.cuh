// attn_wide_kernel.cuh: softmax(scale * Q K^T [causal]) V for head widths up to 512 in one launch -- the shapes attn_general_kernel.cuh cannot be
// instantiated for (32 queries x 512 columns of O per wave are 256 accumulator registers, two LDS stages of a 512-wide K / V^T tile are 256 KB).
// The one user today is the autoencoder's mid-block SelfAttention2d: one head of 512 channels over all H * W latent tokens
// (latent_diffusion/auto_encoder.py:221-225), 16 384 tokens for a 1024 x 1024 image.  attn_wide.hip includes it; mi355x_attention_general
// reaches it for every (Dqk, Dv) <= (512, 512) that no attn_general instance serves.  Same contract as that kernel (mi355x_attn_general_args).
//
// Work split (one workgroup = 4 waves = 64 queries of one (sample, head); key tiles of BKV = 64 keys in bf16, 32 in float32):
//   * S^T = K Q^T is split over QUERIES: wave w owns queries 16 w .. 16 w + 15 against the whole key tile and the whole Dqk.  Its Q fragments
//     stay in registers for the kernel's lifetime (NS = 16 fragments in bf16, 32 in float32), so the online softmax (base 2, c = scale * log2(e),
//     exact running maximum) is the wave's own business exactly as in attn_general_kernel: no partial sums to reduce, no maximum to exchange.
//     The other choice, splitting Dqk over the waves, costs 16 KB of float32 partials per wave per tile through LDS plus a cross-wave maximum.
//   * O^T += V^T P^T is split over Dv: wave w owns V^T rows w * dvw .. + dvw - 1 (dvw = Dv / 4 rounded up to 16: 128 at Dv = 512, 80 at 320) for ALL
//     64 queries, 8 x 4 accumulator blocks = 128 registers.  Every wave therefore needs the tile's full P^T: each wave writes its 16 queries'
//     P^T fragments (already in B-operand layout, bf16: with the k_row_key key order) into an 8 KB LDS buffer, lane-linear, once per tile, together
//     with its 16 rescale factors alpha; after one barrier all four waves read the 8 fragments back.  O is rescaled only in tiles where some
//     query's maximum moved (alpha != 1 somewhere: a ballot), which after the first few tiles of a long row is rare.
//   * K and V^T tiles are register-staged through ONE LDS stage each, half a tile apart: V^T(t) is committed and K(t + 1) issued before
//     S^T(t); after the P^T barrier K(t + 1) is committed and V^T(t + 1) issued before the P V of tile t.  Two barriers per tile.
//   * columns beyond Dqk and V^T rows beyond Dv are zero-filled by the loaders' predicated 16-byte loads; whole groups of 4 MMA steps / 2 V^T
//     blocks past the valid width are skipped (wave-uniform).  FULL = true is the (512, 512) instance with those tests folded away.
// LDS: K tile NS planes of [BKV keys][64 bytes] = 64 KB (planes and swizzle as in attn_general_kernel), V^T tile 512 rows x 128 bytes = 64 KB
//   (tile_off<128>), P^T 8 KB, alpha / 1 / l 256 bytes: 139 520 bytes of the 160 KB, one workgroup = 4 waves per CU, one wave per SIMD.
// Registers per lane (512 available at one wave per SIMD): O 128, Q 64 (float32: 128), K staging 64, V^T staging 64, S^T 16 (8), P^T fragments 16.
// MFMA : LDS reads per wave and tile (bf16): S^T 64 : 64 (every K fragment feeds one 16-query block), P V 64 : 24 (16 V^T + 8 P^T fragments),
//   128 : 88 overall; plus 2 P^T fragment writes.  LDS reads of all four waves (88 x 4 x 8 cycles) are about 1.4 x the MFMA cycles of one SIMD
//   (128 x 16), so the loop is LDS-bound on the S^T half; the measured rates are in docs/MEASUREMENTS_attn_wide.md.
// float32 (the parity mode) runs the same loop on 32-key tiles with v_mfma_f32_16x16x4_f32.
#pragma once
#include "attn_general_kernel.cuh"

namespace {

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void attn_wide_kernel(const GAttnP p) {
    constexpr int ES = sizeof(T);
    constexpr bool IS_BF16 = (ES == 2);
    constexpr int NW = 4, NTHR = 256, BQ = 64, BKV = IS_BF16 ? 64 : 32, DMAX = 512;
    constexpr int NS = DMAX / DT<T>::KSTEP;   // MMA steps over Dqk: 16 / 32
    constexpr int NSG = NS / 4;               // ... in groups of four
    constexpr int NT = BKV / 16;              // S^T blocks of 16 keys: 4 / 2
    constexpr int NPF = 2;                    // P^T fragments per query block and tile: bf16 2 x 32 keys, float32 2 x 16 keys
    constexpr int KPLANE = BKV * 64;          // one K plane: BKV keys x 64 bytes
    constexpr int KBYTES = NS * KPLANE;       // 64 KB
    constexpr int VROWB = BKV * ES;           // V^T tile row: 128 bytes
    constexpr int VBYTES = DMAX * VROWB;      // 64 KB
    constexpr int PBYTES = NW * NPF * 64 * 16;
    constexpr int PP = 64 / BKV;              // K planes one pass of the 256 loader threads covers
    constexpr int KLI = NS / PP;              // 16
    constexpr int VCPR = VROWB / 16;          // 8
    constexpr int VLI = DMAX * VCPR / NTHR;   // 16
    constexpr int NDB = DMAX / NW / 16;       // V^T blocks of 16 rows per wave: 8
    static_assert(VROWB == 128 && KBYTES == 65536 && VBYTES == 65536, "tile plan");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const ks = smem;
    char* const vs = smem + KBYTES;
    char* const ps = vs + VBYTES;
    float* const as = reinterpret_cast<float*>(ps + PBYTES);  // [64 queries]: alpha of the tile; 1 / l at the end

    const int tid = threadIdx.x, lane = tid & 63, wid = wave_id();
    const int g = lane >> 4, c16 = lane & 15;
    int bid = blockIdx.x;
    const int qt = bid % p.qtiles;
    bid /= p.qtiles;
    const int h = bid % p.H;
    const int b = bid / p.H;
    const int qw0 = qt * BQ;         // the workgroup's first query
    const int q0 = qw0 + wid * 16;   // the wave's first S^T query
    const int Dv = FULL ? DMAX : p.Dv;
    const bool causal = p.causal;
    const int qk_chunks = FULL ? DMAX * ES / 16 : (p.Dqk * ES + 15) / 16;
    const int nsg = FULL ? NSG : (qk_chunks + 15) / 16;     // groups of 4 MMA steps = 16 chunks that hold valid columns
    const int dvw = FULL ? DMAX / NW : ((Dv + 15) / 16 + NW - 1) / NW * 16;  // V^T rows per wave
    const int ndg = FULL ? NDB / 2 : (dvw + 31) / 32;       // pairs of V^T blocks the wave runs
    const int vrow0 = wid * dvw;
    const frag_t zero = frag_t{0, 0, 0, 0};

    int ntile = (p.seg[0].Lk + BKV - 1) / BKV;
    if (causal) {  // keys beyond the last query of this workgroup never contribute
        const int last_q = min(qw0 + BQ - 1, p.Lq - 1);
        ntile = min(ntile, last_q / BKV + 1);
    }
    const int Lk = p.seg[0].Lk;

    // ---- Q fragments (B operand) of the wave's 16 queries, predicated on the valid width ----
    frag_t qf[NS];
    {
        int qr = q0 + c16;
        qr = qr < p.Lq ? qr : p.Lq - 1;
        const char* qp = p.q + (int64_t)b * p.qbsb + (int64_t)qr * p.ldqb + (int64_t)h * p.Dqk * ES;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ch = 4 * s + g;
            qf[s] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(qp + ch * 16) : zero;
        }
    }

    const char* kbase = p.seg[0].k + (int64_t)b * p.seg[0].kbsb + (int64_t)h * p.Dqk * ES;
    const char* vbase = p.seg[0].vt + (int64_t)h * Dv * p.seg[0].ldvtb + (int64_t)b * p.seg[0].vtbsb;
    const int64_t ldkb = p.seg[0].ldkb, ldvtb = p.seg[0].ldvtb;
    // K loader: one 16-byte chunk of one key row per plane; a pass of the 256 threads covers PP planes
    const int krow = (tid >> 2) % BKV, ksub = (tid >> 2) / BKV, kg = tid & 3;
    const int koff = krow * 64 + ((kg ^ ((krow >> 2) & 3)) << 4);
    frag_t kr[KLI], vr[VLI];

    auto issue_k = [&](int tile) {
        int key = tile * BKV + (IS_BF16 ? k_row_key(krow) : krow);  // bf16: permuted key order (k_row_key, common.cuh)
        key = key < Lk ? key : Lk - 1;
        const char* kp = kbase + (int64_t)key * ldkb;
#pragma unroll
        for (int it = 0; it < KLI; ++it) {
            const int ch = 4 * (it * PP + ksub) + kg;
            kr[it] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(kp + ch * 16) : zero;
        }
    };
    auto commit_k = [&]() {
#pragma unroll
        for (int it = 0; it < KLI; ++it) *reinterpret_cast<frag_t*>(ks + (it * PP + ksub) * KPLANE + koff) = kr[it];
    };
    auto issue_v = [&](int tile) {  // (rows are readable up to the next multiple of 64 keys: whole chunks, no key predicate)
        const char* vp = vbase + (int64_t)tile * BKV * ES;
#pragma unroll
        for (int it = 0; it < VLI; ++it) {
            const int q = it * NTHR + tid, row = q / VCPR, pch = q % VCPR;
            vr[it] = row < Dv ? *reinterpret_cast<const frag_t*>(vp + (int64_t)row * ldvtb + pch * 16) : zero;
        }
    };
    auto commit_v = [&]() {
#pragma unroll
        for (int it = 0; it < VLI; ++it) {
            const int q = it * NTHR + tid, row = q / VCPR, pch = q % VCPR;
            *reinterpret_cast<frag_t*>(vs + tile_off<VROWB>(row, pch)) = vr[it];
        }
    };

    f32x4 o[NDB][NW];  // O^T blocks: V^T rows vrow0 + 16 i + 4 g + r of query 16 jq + c16
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int jq = 0; jq < NW; ++jq) o[i][jq] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrun = -INFINITY, lsum = 0.f;

    issue_k(0);
    commit_k();
    issue_v(0);
    __syncthreads();

    for (int tile = 0; tile < ntile; ++tile) {
        const bool more = tile + 1 < ntile;
        const int kv0 = tile * BKV;
        commit_v();  // (every wave left the P V of the previous tile at the barrier that ended it)
        if (more) issue_k(tile + 1);

        // ---- S^T = K Q^T: 16 queries x BKV keys ----
        f32x4 st[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sg = 0; sg < NSG; ++sg) {
            if (!FULL && sg >= nsg) continue;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int row = 16 * t + c16;
                    const int off = row * 64 + ((g ^ ((row >> 2) & 3)) << 4);
                    mma_step<T>(st[t], lds_read_frag(ks, (4 * sg + s4) * KPLANE + off), qf[4 * sg + s4]);
                }
        }
        // ---- masks: keys past Lk, and (causal) keys after the query ----
        if (kv0 + BKV > Lk || (causal && kv0 + BKV - 1 > q0)) {
            const int qi = q0 + c16;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + (IS_BF16 ? k_row_key(16 * t + 4 * g + r) : 16 * t + 4 * g + r);
                    if (key >= Lk || (causal && key > qi)) st[t][r] = -INFINITY;
                }
        }
        // ---- online softmax of the wave's 16 queries ----
        {
            float mx = st[0][0];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[t][r]);
            const float mnew = fmaxf(mrun, group_max4(mx));
            // a fully masked prefix keeps mnew = -inf: use 0 as the reference point so that exp2(-inf - 0) = 0, not NaN
            const float mref = mnew == -INFINITY ? 0.f : mnew;
            const float alpha = fast_exp2((mrun - mref) * p.c);
            const float mc = mref * p.c;
            float psum = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = fast_exp2(st[t][r] * p.c - mc);
                    st[t][r] = e;
                    psum += e;
                }
            lsum = lsum * alpha + psum;  // (the lane's share; the four lane groups are summed once, at the end)
            mrun = mnew;
            if (g == 0) as[wid * 16 + c16] = alpha;
        }
        // ---- the wave's P^T fragments, B-operand layout, lane-linear: fragment f of query block w at ps + ((w NPF + f) 64 + lane) 16 ----
#pragma unroll
        for (int f = 0; f < NPF; ++f) {
            frag_t pf;
            if constexpr (IS_BF16) {
                bf16x8 pk;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pk[r] = (bf16_t)st[2 * f][r];
                    pk[4 + r] = (bf16_t)st[2 * f + 1][r];
                }
                pf = __builtin_bit_cast(frag_t, pk);
            } else {
                pf = __builtin_bit_cast(frag_t, st[f]);
            }
            *reinterpret_cast<frag_t*>(ps + ((wid * NPF + f) * 64 + lane) * 16) = pf;
        }
        __syncthreads();  // P^T, alpha and V^T(tile) are in LDS; nobody reads K(tile) any more

        if (more) {
            commit_k();
            issue_v(tile + 1);
        }
        // ---- rescale: only where some query's maximum moved ----
        {
            float al[NW];
            bool need = false;
#pragma unroll
            for (int jq = 0; jq < NW; ++jq) {
                al[jq] = as[16 * jq + c16];
                need |= al[jq] != 1.f;
            }
            if (__builtin_amdgcn_ballot_w64(need) != 0) {  // wave-uniform
#pragma unroll
                for (int i = 0; i < NDB; ++i)
#pragma unroll
                    for (int jq = 0; jq < NW; ++jq) o[i][jq] *= al[jq];
            }
        }
        // ---- O^T += V^T P^T over the wave's V^T rows, all 64 queries ----
#pragma unroll
        for (int f = 0; f < NPF; ++f) {
            frag_t pb[NW];
#pragma unroll
            for (int jq = 0; jq < NW; ++jq) pb[jq] = lds_read_frag(ps, ((jq * NPF + f) * 64 + lane) * 16);
#pragma unroll
            for (int ig = 0; ig < NDB / 2; ++ig) {
                if (!FULL && ig >= ndg) continue;
#pragma unroll
                for (int i2 = 0; i2 < 2; ++i2) {
                    const int i = 2 * ig + i2;
                    const frag_t vf = lds_read_frag(vs, tile_off<VROWB>(vrow0 + 16 * i + c16, 4 * f + g));  // one chunk = the lane's 8 (4) consecutive keys
#pragma unroll
                    for (int jq = 0; jq < NW; ++jq) mma_step<T>(o[i][jq], vf, pb[jq]);
                }
            }
        }
        __syncthreads();  // K(tile + 1) is in LDS; nobody reads V^T(tile), P^T or alpha any more
    }

    // ---- out_scale / l of every query, through LDS like alpha ----
    {
        float l = lsum;
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (g == 0) as[wid * 16 + c16] = p.out_scale / l;
    }
    __syncthreads();
#pragma unroll
    for (int jq = 0; jq < NW; ++jq) {
        const int qi = qw0 + 16 * jq + c16;
        if (qi >= p.Lq) continue;
        const float inv = as[16 * jq + c16];
        T* op = reinterpret_cast<T*>(p.out + (int64_t)b * p.obsb + (int64_t)qi * p.ldob) + (int64_t)h * Dv;
#pragma unroll
        for (int i = 0; i < NDB; ++i) {
            const int d0 = vrow0 + 16 * i + 4 * g;
            if (16 * i >= dvw || d0 + 4 > Dv) continue;  // (rows past the wave's share belong to the next wave; Dv is a multiple of 4)
            if constexpr (IS_BF16) {
                bf16x4 v4;
#pragma unroll
                for (int r = 0; r < 4; ++r) v4[r] = (bf16_t)(o[i][jq][r] * inv);
                *reinterpret_cast<bf16x4*>(op + d0) = v4;
            } else {
                *reinterpret_cast<f32x4*>(op + d0) = o[i][jq] * inv;
            }
        }
    }
}

template <typename T, bool FULL>
int attn_wide_launch(const GAttnP& p0, hipStream_t stream) {
    constexpr int LDS = 65536 + 65536 + 4 * 2 * 64 * 16 + 64 * 4;  // K tile, V^T tile, P^T, alpha
    auto kfn = attn_wide_kernel<T, FULL>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_set = true;
    }
    GAttnP p = p0;
    p.qtiles = (p.Lq + 63) / 64;
    hipLaunchKernelGGL(kfn, dim3(p.qtiles * p.H * p.B), dim3(256), LDS, stream, p);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

template <typename T>
int attn_wide_dispatch(const GAttnP& p, hipStream_t st) {
    if (p.Dqk > 512 || p.Dv > 512) return MI355X_ESHAPE;
    return p.Dqk == 512 && p.Dv == 512 ? attn_wide_launch<T, true>(p, st) : attn_wide_launch<T, false>(p, st);
}

}  // namespace
