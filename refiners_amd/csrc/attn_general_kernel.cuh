// attn_general_kernel.cuh: the tile loop of the general-head-shape attentions, once.  Two translation units include it:
//   attention_general.hip  JOINT = false: softmax(scale * Q K^T [causal]) V over one key segment, Dqk != Dv allowed, out_scale / l in the store;
//   reference_only.hip     JOINT = true:  mix * softmax(scale * Q [K0 ; K1]^T) [V0 ; V1] + (1 - mix) * softmax(scale * Q K0^T) V0 over two segments.
//
// Same wave-level scheme as attention.hip (S^T = K Q^T so a lane owns one query column, P^T already in B-operand layout,
// base-2 online softmax on raw v_exp_f32, 32 queries per wave, 4 waves, 64-key tiles, register-staged double-buffered LDS),
// generalised along the head dimension:
//   * QK^T runs over NS = ceil(Dqk / KSTEP) MMA steps; the K tile lives in LDS as NS planes of [64 keys][64 bytes]
//     (one MMA step's worth of columns per plane), 16-byte chunks XOR-swizzled by (row >> 2) & 3 so that a 16-row fragment
//     read touches 16 distinct 16-byte slots of a 256-byte bank row;
//   * P V runs over ND = ceil(Dv / 16) independent 16-row blocks of V^T, so Dv = 80 costs exactly 5 blocks (no padding to 128);
//   * columns / rows beyond Dqk / Dv are zero-filled by the loaders (predicated 16-byte loads), nothing is padded in HBM;
//   * `causal` (JOINT = false): key j contributes to query i only if j <= i (both indices within the sample); tiles entirely above the
//     diagonal are skipped.
// What JOINT adds, all of it behind `if constexpr (JOINT)` or folded by it:
//   * the key loop runs over segment 0's tiles, then segment 1's; each segment has its own pointers and strides, and its last tile is
//     masked by its own Lk (both segments may be a fraction of one tile);
//   * where segment 1 begins, a sample with 0 != mix != 1 writes (1 - mix) * O / l into the lane's own `out` elements and reads them
//     back in the final store.  The same lane writes and reads, so program order is all the ordering it needs; keeping the term in
//     registers would double the accumulator (80 more VGPRs at D = 160).  O and l share the reference maximum on the lazy path too,
//     so the quotient is exact there;
//   * mix is read from device memory per sample: mix == 1 skips the snapshot, mix == 0 skips segment 1 altogether.
#pragma once
#include "common.cuh"
#include "../../include/mi355x_refiners.h"

namespace {

struct GAttnSeg {
    const char* k;
    const char* vt;
    int64_t ldkb, kbsb, ldvtb, vtbsb;  // bytes
    int Lk;
};

struct GAttnP {
    int B, H, Lq, Dqk, Dv, causal;  // JOINT: Dqk is the one head width, Dv and causal are not read
    const char* q;
    char* out;
    int64_t ldqb, qbsb, ldob, obsb;  // bytes
    float c;          // scale * log2(e)
    float thr;        // FAST: a tile leaves the running maximum alone while no score exceeds it by more than thr = 8 / c
    float out_scale;  // (JOINT = false)
    int qtiles;
    GAttnSeg seg[2];   // key segments; JOINT = false reads seg[0] only
    const float* mix;  // JOINT: per-sample blend weight on the device, or NULL (all ones)
};

// lane <-> lane ^ 16 / lane ^ 32 as row / half swaps (gfx950; see attention.hip): the maximum over a query's four lane groups without an LDS round trip
MI_DEV float group_max4(float x) {
    float a = x, b = x;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    a = fmaxf(a, b), b = a;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}

// FAST (bf16, round 6; the measures of attention.hip's self-attention loop that do not depend on its pipelining): lazy running maximum (cross-lane maximum and the
// O / l rescale only when some lane of the wave sees a score above reference + thr: P <= 2^8 otherwise, exact in the quotient), row sums l from the matrix pipe
// (one more MFMA per P^T fragment against a fragment of ones: l = sum of the ROUNDED P), permlane reductions instead of ds_bpermute.
template <typename T, int NS, int ND, bool FAST, bool JOINT>
__global__ __launch_bounds__(256) void attn_general_kernel(const GAttnP p) {
    static_assert(!FAST || sizeof(T) == 2, "FAST is the bf16 path");
    constexpr int ES = sizeof(T);
    constexpr int NW = 4, NTHR = 256, BQW = 32, BKV = 64;
    constexpr int VROWB = BKV * ES;           // V^T tile row: 64 keys
    constexpr int KPLANE = 64 * 64;           // one K plane: 64 keys x 64 bytes
    constexpr int KBYTES = NS * KPLANE;
    constexpr int VBYTES = ND * 16 * VROWB;
    constexpr int STAGE = KBYTES + VBYTES;
    constexpr int VCPR = VROWB / 16;          // 16-byte chunks per V^T row
    constexpr int VLI = (ND * 16 * VCPR + NTHR - 1) / NTHR;
    constexpr bool IS_BF16 = (ES == 2);
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = wave_id();
    const int g = lane >> 4, c16 = lane & 15;
    int bid = blockIdx.x;
    const int qt = bid % p.qtiles;
    bid /= p.qtiles;
    const int h = bid % p.H;
    const int b = bid / p.H;
    const int q0 = qt * (BQW * NW) + wid * BQW;
    const int Dv = JOINT ? p.Dqk : p.Dv;
    const bool causal = !JOINT && p.causal;
    const int qk_chunks = (p.Dqk * ES + 15) / 16;  // valid 16-byte chunks of a Q / K row of this head
    const frag_t zero = frag_t{0, 0, 0, 0};

    // ---- tiles: segment 0's, then (JOINT) segment 1's ----
    const int nt0 = (p.seg[0].Lk + BKV - 1) / BKV;
    int ntile = nt0;
    float mixb = 1.f;   // JOINT: the sample's blend weight, uniform over the workgroup
    bool snap = false;  // JOINT: the sample parks its segment-0 term at the boundary
    if constexpr (JOINT) {
        mixb = p.mix ? p.mix[b] : 1.f;
        ntile = nt0 + (mixb == 0.f ? 0 : (p.seg[1].Lk + BKV - 1) / BKV);  // mix == 0: the plain attention over segment 0
        snap = mixb != 1.f && mixb != 0.f;
    } else if (causal) {  // keys beyond the last query of this workgroup never contribute
        const int last_q = min(qt * (BQW * NW) + BQW * NW - 1, p.Lq - 1);
        ntile = min(ntile, last_q / BKV + 1);
    }

    // ---- Q fragments (B operand), predicated on the valid width ----
    frag_t qf[2][NS];
#pragma unroll
    for (int jq = 0; jq < 2; ++jq) {
        int qr = q0 + 16 * jq + c16;
        qr = qr < p.Lq ? qr : p.Lq - 1;
        const char* qp = p.q + (int64_t)b * p.qbsb + (int64_t)qr * p.ldqb + (int64_t)h * p.Dqk * ES;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ch = 4 * s + g;
            qf[jq][s] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(qp + ch * 16) : zero;
        }
    }

    const char* kbase0 = p.seg[0].k + (int64_t)b * p.seg[0].kbsb + (int64_t)h * p.Dqk * ES;
    const char* vbase0 = p.seg[0].vt + (int64_t)h * Dv * p.seg[0].ldvtb + (int64_t)b * p.seg[0].vtbsb;
    const char* kbase1 = nullptr;
    const char* vbase1 = nullptr;
    if constexpr (JOINT) {
        kbase1 = p.seg[1].k + (int64_t)b * p.seg[1].kbsb + (int64_t)h * p.Dqk * ES;
        vbase1 = p.seg[1].vt + (int64_t)h * Dv * p.seg[1].ldvtb + (int64_t)b * p.seg[1].vtbsb;
    }
    const int krow = tid >> 2, kg = tid & 3;  // K loader: one 16-byte chunk of one key row per plane
    const int koff = krow * 64 + ((kg ^ ((krow >> 2) & 3)) << 4);
    frag_t kr[NS], vr[VLI];

    auto issue = [&](int tile) {
        const bool s1 = JOINT && tile >= nt0;  // which segment the tile belongs to, and where it starts there
        const int kv0 = (s1 ? tile - nt0 : tile) * BKV;
        const int Lk = s1 ? p.seg[1].Lk : p.seg[0].Lk;
        const char* kbase = s1 ? kbase1 : kbase0;
        const char* vbase = s1 ? vbase1 : vbase0;
        const int64_t ldkb = s1 ? p.seg[1].ldkb : p.seg[0].ldkb, ldvtb = s1 ? p.seg[1].ldvtb : p.seg[0].ldvtb;
        int key = kv0 + (IS_BF16 ? k_row_key(krow) : krow);  // bf16: permuted key order (k_row_key, common.cuh)
        key = key < Lk ? key : Lk - 1;
        const char* kp = kbase + (int64_t)key * ldkb;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ch = 4 * s + kg;
            kr[s] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(kp + ch * 16) : zero;
        }
#pragma unroll
        for (int it = 0; it < VLI; ++it) {
            const int q = it * NTHR + tid, row = q / VCPR, pch = q % VCPR;
            vr[it] = (row < Dv) ? *reinterpret_cast<const frag_t*>(vbase + (int64_t)row * ldvtb + (int64_t)kv0 * ES + pch * 16) : zero;
        }
    };
    auto commit = [&](int buf) {
        char* ks = smem + buf * STAGE;
        char* vs = ks + KBYTES;
#pragma unroll
        for (int s = 0; s < NS; ++s) *reinterpret_cast<frag_t*>(ks + s * KPLANE + koff) = kr[s];
#pragma unroll
        for (int it = 0; it < VLI; ++it) {
            const int q = it * NTHR + tid, row = q / VCPR, pch = q % VCPR;
            if (row < ND * 16) *reinterpret_cast<frag_t*>(vs + tile_off<VROWB>(row, pch)) = vr[it];
        }
    };

    f32x4 o[ND][2];
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int jq = 0; jq < 2; ++jq) o[i][jq] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrun[2] = {-INFINITY, -INFINITY};
    float lsum[2] = {0.f, 0.f};
    f32x4 lacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};  // FAST: row sums as an MFMA accumulator (its four rows are equal)
    const frag_t ones = frag_t{0x3f803f80, 0x3f803f80, 0x3f803f80, 0x3f803f80};

    auto row_sum = [&](int jq) {  // (every lane calls it: the non-FAST form shuffles)
        if constexpr (FAST) {
            return lacc[jq][0];
        } else {
            float l = lsum[jq];
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            return l;
        }
    };
    // the lane's output elements: d = 16 i + 4 g + r of query 16 jq + c16
    auto out_row = [&](int jq) { return reinterpret_cast<T*>(p.out + (int64_t)b * p.obsb + (int64_t)(q0 + 16 * jq + c16) * p.ldob) + (int64_t)h * Dv; };

    issue(0);
    commit(0);
    __syncthreads();

    for (int tile = 0; tile < ntile; ++tile) {
        const int cur = tile & 1;
        const bool more = tile + 1 < ntile;
        if (more) issue(tile + 1);
        const char* ks = smem + cur * STAGE;
        const char* vs = ks + KBYTES;
        const bool s1 = JOINT && tile >= nt0;
        const int kv0 = (s1 ? tile - nt0 : tile) * BKV;
        const int Lk = s1 ? p.seg[1].Lk : p.seg[0].Lk;

        // ---- segment boundary: park (1 - mix) * softmax(Q K0^T) V0 in the lane's own output elements ----
        // (Written out here and again after the loop, not as one row-store helper: with the store behind a lambda or a device function the
        //  float32 (6, 5) JOINT instance needs 263 registers for the 252 it has this way, and loses its second wave per SIMD.)
        if constexpr (JOINT) {
            if (snap && tile == nt0) {
#pragma unroll
                for (int jq = 0; jq < 2; ++jq) {
                    const float w = (1.f - mixb) / row_sum(jq);  // (every lane: row_sum shuffles)
                    if (q0 + 16 * jq + c16 >= p.Lq) continue;
                    T* op = out_row(jq);
#pragma unroll
                    for (int i = 0; i < ND; ++i) {
                        const int d0 = 16 * i + 4 * g;
                        if (d0 + 4 > Dv) continue;  // (Dv is a multiple of 4)
                        if constexpr (IS_BF16) {
                            bf16x4 v4;
#pragma unroll
                            for (int r = 0; r < 4; ++r) v4[r] = (bf16_t)(o[i][jq][r] * w);
                            *reinterpret_cast<bf16x4*>(op + d0) = v4;
                        } else {
                            *reinterpret_cast<f32x4*>(op + d0) = o[i][jq] * w;
                        }
                    }
                }
            }
        }

        // ---- S^T = K Q^T ----
        f32x4 st[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            st[t][0] = f32x4{0.f, 0.f, 0.f, 0.f};
            st[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int row = 16 * t + c16;
            const int off = row * 64 + ((g ^ ((row >> 2) & 3)) << 4);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const frag_t kf = lds_read_frag(ks, s * KPLANE + off);
                mma_step<T>(st[t][0], kf, qf[0][s]);
                mma_step<T>(st[t][1], kf, qf[1][s]);
            }
        }
        // ---- masks: keys past the segment's own Lk, and (causal) keys after the query ----
        if (kv0 + BKV > Lk || (causal && kv0 + BKV - 1 > q0)) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + (IS_BF16 ? k_row_key(16 * t + 4 * g + r) : 16 * t + 4 * g + r);
#pragma unroll
                    for (int jq = 0; jq < 2; ++jq) {
                        const int qi = q0 + 16 * jq + c16;
                        if (key >= Lk || (causal && key > qi)) st[t][jq][r] = -INFINITY;
                    }
                }
        }
        // ---- online softmax ----
        if constexpr (FAST) {
            float mloc[2];
            bool need = false;
#pragma unroll
            for (int jq = 0; jq < 2; ++jq) {
                float mx = st[0][jq][0];
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[t][jq][r]);
                mloc[jq] = mx;
                need |= mx > mrun[jq] + p.thr;  // (reference still -inf: any finite score)
            }
            if (__builtin_amdgcn_ballot_w64(need) != 0) {  // wave-uniform
#pragma unroll
                for (int jq = 0; jq < 2; ++jq) {
                    const float mnew = fmaxf(mrun[jq], group_max4(mloc[jq]));
                    const float mref = mnew == -INFINITY ? 0.f : mnew;  // (a fully masked prefix: see below)
                    const float alpha = fast_exp2((mrun[jq] - mref) * p.c);
                    mrun[jq] = mnew;
                    lacc[jq] *= alpha;
#pragma unroll
                    for (int i = 0; i < ND; ++i) o[i][jq] *= alpha;
                }
            }
#pragma unroll
            for (int jq = 0; jq < 2; ++jq) {
                const float mc = (mrun[jq] == -INFINITY ? 0.f : mrun[jq]) * p.c;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) st[t][jq][r] = fast_exp2(st[t][jq][r] * p.c - mc);
            }
        }
#pragma unroll
        for (int jq = 0; jq < (FAST ? 0 : 2); ++jq) {
            float mx = st[0][jq][0];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[t][jq][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mnew = fmaxf(mrun[jq], mx);
            // a fully masked prefix keeps mnew = -inf: use 0 as the reference point so that exp2(-inf - 0) = 0, not NaN
            const float mref = mnew == -INFINITY ? 0.f : mnew;
            const float alpha = fast_exp2((mrun[jq] - mref) * p.c);
            const float mc = mref * p.c;
            float ps = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = fast_exp2(st[t][jq][r] * p.c - mc);
                    st[t][jq][r] = e;
                    ps += e;
                }
            lsum[jq] = lsum[jq] * alpha + ps;
            mrun[jq] = mnew;
#pragma unroll
            for (int i = 0; i < ND; ++i) o[i][jq] *= alpha;
        }
        // ---- O^T += V^T P^T ----
        if constexpr (IS_BF16) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                frag_t pb[2];
#pragma unroll
                for (int jq = 0; jq < 2; ++jq) {
                    bf16x8 pk;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pk[r] = (bf16_t)st[2 * s2][jq][r];
                        pk[4 + r] = (bf16_t)st[2 * s2 + 1][jq][r];
                    }
                    pb[jq] = __builtin_bit_cast(frag_t, pk);
                }
                if constexpr (FAST) {
                    mma_step<T>(lacc[0], ones, pb[0]);
                    mma_step<T>(lacc[1], ones, pb[1]);
                }
#pragma unroll
                for (int i = 0; i < ND; ++i) {
                    const frag_t vf = lds_read_frag(vs, tile_off<VROWB>(16 * i + c16, 4 * s2 + g));  // one chunk = the lane's 8 consecutive keys
                    mma_step<T>(o[i][0], vf, pb[0]);
                    mma_step<T>(o[i][1], vf, pb[1]);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const frag_t p0 = __builtin_bit_cast(frag_t, st[t][0]);
                const frag_t p1 = __builtin_bit_cast(frag_t, st[t][1]);
#pragma unroll
                for (int i = 0; i < ND; ++i) {
                    const frag_t vf = lds_read_frag(vs, tile_off<VROWB>(16 * i + c16, 4 * t + g));
                    mma_step<T>(o[i][0], vf, p0);
                    mma_step<T>(o[i][1], vf, p1);
                }
            }
        }
        if (more) commit(cur ^ 1);
        __syncthreads();
    }

    // ---- store: out_scale * O / l; JOINT: mix * O / l, plus the parked term where one was kept ----
#pragma unroll
    for (int jq = 0; jq < 2; ++jq) {
        // (the order and the spelling of these lines are the two kernels' own, each to its instance: an idle row leaves before the row sum with one
        //  segment and after it with two, and l is not taken through row_sum() -- either change moves the register allocation of an instance)
        if (!JOINT && q0 + 16 * jq + c16 >= p.Lq) continue;
        float l = lsum[jq];
        if constexpr (FAST) {
            l = lacc[jq][0];
        } else {
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
        }
        if (JOINT && q0 + 16 * jq + c16 >= p.Lq) continue;
        const float inv = (JOINT ? (snap ? mixb : 1.f) : p.out_scale) / l;
        T* op = out_row(jq);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int d0 = 16 * i + 4 * g;
            if (d0 + 4 > Dv) continue;  // (Dv is a multiple of 4: the entry points refuse any other)
            if constexpr (IS_BF16) {
                bf16x4 v4;
                if (JOINT && snap) {
                    const bf16x4 kept = *reinterpret_cast<const bf16x4*>(op + d0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v4[r] = (bf16_t)((float)kept[r] + o[i][jq][r] * inv);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v4[r] = (bf16_t)(o[i][jq][r] * inv);
                }
                *reinterpret_cast<bf16x4*>(op + d0) = v4;
            } else {
                f32x4 v = o[i][jq] * inv;
                if (JOINT && snap) v += *reinterpret_cast<const f32x4*>(op + d0);
                *reinterpret_cast<f32x4*>(op + d0) = v;
            }
        }
    }
}

template <typename T, int NS, int ND, bool FAST, bool JOINT>
int attn_general_launch(const GAttnP& p0, hipStream_t stream) {
    constexpr int LDS = 2 * (NS * 64 * 64 + ND * 16 * 64 * (int)sizeof(T));  // two stages of NS K planes + ND V^T blocks
    auto kfn = attn_general_kernel<T, NS, ND, FAST, JOINT>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_set = true;
    }
    GAttnP p = p0;
    p.qtiles = (p.Lq + 127) / 128;
    hipLaunchKernelGGL(kfn, dim3(p.qtiles * p.H * p.B), dim3(256), LDS, stream, p);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

// (QK steps of 32 bf16 / 2 x 16 f32 columns, PV blocks of 16 V^T rows, instantiated for JOINT too): the smallest pair that covers the request is used.
#define ATTN_GENERAL_INSTANCES(X)                                                  \
    X(2, 3, true)   /* head dim 40 (SD1.5 at 320 channels) */                      \
    X(2, 4, true)   /* head dim 64; with causal masking, CLIP */                   \
    X(3, 5, true)   /* head dim 80 (SD1.5 at 640 channels) */                      \
    X(4, 5, false)  /* SAM windowed: 80 + 14 + 14 bias columns, V 80 */            \
    X(4, 8, true)   /* head dim 128 (MVANet's single-head attentions) */           \
    X(5, 10, true)  /* head dim 160 (SD1.5 at 1280 channels) */                    \
    X(7, 5, false)  /* SAM global: 80 + 64 + 64 bias columns, V 80 */

// float32 has the plain softmax only.  bfloat16 takes the FAST instance unless the one-segment caller passes fast = false (A/B and tests);
// JOINT has no other bfloat16 instance, and its caller passes nothing.
template <typename T, bool JOINT>
int attn_general_dispatch(const GAttnP& p, hipStream_t st, bool fast = true) {
    constexpr int KSTEP = DT<T>::KSTEP;
    const int ns = (p.Dqk + KSTEP - 1) / KSTEP, nd = ((JOINT ? p.Dqk : p.Dv) + 15) / 16;
#define TRY(NS_, ND_, JOINT_TOO_)                                                                                                  \
    if constexpr (!JOINT || JOINT_TOO_) {                                                                                          \
        if (ns <= (NS_ * 32 / KSTEP) && nd <= ND_) {                                                                               \
            if constexpr (sizeof(T) == 2) {                                                                                        \
                if (JOINT || fast) return attn_general_launch<T, NS_ * 32 / KSTEP, ND_, true, JOINT>(p, st);                       \
            }                                                                                                                      \
            if constexpr (sizeof(T) == 4 || !JOINT) return attn_general_launch<T, NS_ * 32 / KSTEP, ND_, false, JOINT>(p, st);     \
        }                                                                                                                          \
    }
    ATTN_GENERAL_INSTANCES(TRY)
#undef TRY
    return MI355X_ESHAPE;
}

}  // namespace
