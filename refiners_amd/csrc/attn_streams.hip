// mi355x_attention_streams: out = sum_s out_scale_s * softmax(scale * Q K_s^T) V_s over one or two K/V streams that together have at most
// three 64-key tiles, at the head widths of mi355x_attention_general with Dqk == Dv (SD1.5: 40 / 80 / 160).  The cross-attention of an
// IP-Adapter on SD1.5 -- 77 text keys + 4 or 16 image keys -- as ONE launch, where the tile loop of attn_general_kernel.cuh takes a launch per
// stream and an axpby.  It is the general-width sibling of attn_short_dma_kernel (attention.hip, head width 64) and shares that kernel's
// buffer-descriptor LDS-DMA helpers (attn_short_body.cuh); the kernel itself is its own:
//
//   * Work split.  A workgroup is 4 waves on consecutive queries of one (sample, head); a wave owns 16 JQ queries, JQ = 2 (128 queries per
//     workgroup) or, where that grid would not give each of the GPU's 256 CUs a workgroup, JQ = 1 (64 queries per workgroup).  These launches
//     are latency-bound chains (load, Q K^T, softmax, P V, store) and every workgroup loads the whole K / V^T of its (sample, head); the
//     16-query wave halves the MFMA and softmax chain of a wave and doubles the number of CUs at work, while the four waves of a workgroup
//     still share one copy of the keys (SD1.5's mid block, 64 queries x 8 heads x 2 samples: 16 workgroups of four busy waves, not 16 of two).
//   * Wave-level scheme of the other attention kernels: S^T = K Q^T, so a lane owns query column c16 and P^T is already in B-operand
//     layout; v_mfma_f32_16x16x32_bf16 (bfloat16) / 4 x v_mfma_f32_16x16x4_f32 (float32) through mma_step.
//   * Residency (bfloat16).  All K tiles and all V^T tiles of all streams are brought into LDS ONCE per workgroup by LDS-DMA
//     (raw_ptr_buffer_load_lds, 16 bytes per lane), then one wait and one barrier: no key loop over HBM, no double buffering.  A tile is NS K
//     planes of [64 keys][64 bytes] followed by 16 ND V^T rows of 128 bytes: at D = 160, 3 x (5 x 4 KB + 160 x 128 B) = 120 KB of gfx950's 160 KB.
//     float32 (the parity mode) does not fit at D = 160: it walks ONE stage -- every tile's K planes in turn while the scores are formed, then
//     every tile's V^T rows in turn for P V -- with a barrier pair per refill.
//   * LDS layouts.  K: the swizzled planes of attn_general_kernel.cuh (one MMA step's columns per plane, 16-byte chunks XOR-ed with
//     (row >> 2) & 3: a 16-row fragment read touches 16 distinct slots), bfloat16 rows in k_row_key order so that a P^T fragment is eight
//     consecutive keys.  V^T: tile_off rows (common.cuh).  LDS-DMA lands lane i at base + 16 i, so the swizzle and the key order are applied
//     to each lane's SOURCE offset.
//   * Predication is the buffer descriptor's: a lane whose chunk lies beyond D (K columns, V^T rows), or whose key lies at or beyond the
//     stream's Lk (K rows; V^T chunks that hold no valid key), carries an out-of-range offset, for which the hardware writes zeros.  Nothing is
//     padded in HBM, no K row at or beyond Lk is read.  A tile with at most 32 valid keys (the image tokens) is a HALF tile: its K rows
//     32 .. 63 are not requested and its key blocks 2, 3 are neither multiplied nor exponentiated.
//   * Softmax.  The whole score row of a query -- at most 192 scores, 48 per lane and query -- stays in registers.  Per stream: the true maximum
//     over its valid keys (masked keys are -inf), base-2 exponentials, the row sum; no online softmax, no running maximum, no threshold.  In
//     bfloat16 the exponentials are rounded to bfloat16 BEFORE they are summed, so the row sum is the sum of what P V multiplies.  Each
//     stream's P is then scaled by out_scale_s / l_s, and both streams accumulate into one O: no second accumulator, no rescale, one store.
//   * A stream with out_scale == 0 is skipped altogether (no load, no scores, no P V): an exact zero whatever its scores would have been.
#include "attn_short_body.cuh"
#include "../../include/mi355x_refiners_attn_streams.h"

namespace {

using mi355x_attn::blds16;
using mi355x_attn::group_max;
using mi355x_attn::group_sum;
using mi355x_attn::make_rsrc;
using mi355x_attn::rsrc_t;

struct StreamsKv {
    const char* k;
    const char* vt;
    int64_t ldkb, kbsb, ldvtb, vtbsb;  // bytes
    int Lk;
    float out_scale;
};

struct StreamsP {
    int B, H, Lq, D, nstream;
    const char* q;
    char* out;
    int64_t ldqb, qbsb, ldob, obsb;  // bytes
    float c;                         // scale * log2(e)
    int qtiles;
    StreamsKv kv[2];
};

constexpr int STREAMS_SLOTS = 3;           // key tiles over all streams
constexpr uint32_t STREAMS_OOR = 0x80000000u;  // beyond every descriptor's range: the load writes zeros
constexpr int STREAMS_CUS = 256;           // MI355X

// NS: K planes (64 bytes of every key row each); ND: 16-row blocks of V^T; JQ: 16-query blocks per wave; RESIDENT: every tile has LDS of its own
template <typename T, int NS, int ND, int JQ, bool RESIDENT>
__global__ __launch_bounds__(256) void attn_streams_kernel(const StreamsP p) {
    constexpr int ES = sizeof(T), EPC = 16 / ES;
    constexpr int NW = 4, NTHR = 256, BKV = 64, SLOTS = STREAMS_SLOTS;
    constexpr int KPLANE = 64 * 64, KBYTES = NS * KPLANE;
    constexpr int VROWB = BKV * ES, VCPR = VROWB / 16, VROWS = ND * 16, VBYTES = VROWS * VROWB;
    constexpr int VLI = (VROWS * VCPR + NTHR - 1) / NTHR;
    constexpr int SLOT = KBYTES + VBYTES;
    constexpr bool IS_BF16 = (ES == 2);
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = wave_id();
    const int g = lane >> 4, c16 = lane & 15;
    int bid = blockIdx.x;
    const int qt = bid % p.qtiles;
    bid /= p.qtiles;
    const int h = bid % p.H;
    const int b = bid / p.H;
    const int q0 = qt * (16 * JQ * NW) + wid * 16 * JQ;
    const int qk_chunks = p.D * ES / 16;  // 16-byte chunks of a Q / K row of this head (D * ES % 16 == 0)
    const frag_t zero = frag_t{0, 0, 0, 0};

    // ---- tiles: stream 0's, then stream 1's; everything below is uniform over the workgroup ----
    const int nt0 = (p.kv[0].Lk + BKV - 1) / BKV;
    const int ntot = nt0 + (p.nstream > 1 ? (p.kv[1].Lk + BKV - 1) / BKV : 0);  // <= SLOTS (checked by the host)
    auto stream_of = [&](int sl) { return sl >= nt0 ? 1 : 0; };
    auto first_key = [&](int sl) { return (sl >= nt0 ? sl - nt0 : sl) * BKV; };
    auto used = [&](int sl) { return sl < ntot && p.kv[stream_of(sl)].out_scale != 0.f; };
    auto is_half = [&](int sl) { return p.kv[stream_of(sl)].Lk - first_key(sl) <= 32; };

    // ---- loaders: LDS-DMA by all 256 threads; the caller waits (vmcnt) and synchronises ----
    auto load_k = [&](int sl, char* ks) {
        const StreamsKv& kv = p.kv[stream_of(sl)];
        const int kv0 = first_key(sl);
        const int valid = min(kv.Lk - kv0, BKV);
        if (valid <= 32 && wid >= 2) return;  // a half tile has no rows 32 .. 63 (a wave loads 16 rows of every plane)
        const rsrc_t rs = make_rsrc(kv.k + (int64_t)b * kv.kbsb + (int64_t)h * p.D * ES + (int64_t)kv0 * kv.ldkb, (int64_t)(valid - 1) * kv.ldkb + p.D * ES);
        const int row = tid >> 2;
        const int kg = (tid & 3) ^ ((row >> 2) & 3);      // the logical chunk this lane's physical slot holds
        const int key = IS_BF16 ? k_row_key(row) : row;  // bf16: permuted key order (common.cuh)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ch = 4 * s + kg;
            const uint32_t off = (key < valid && ch < qk_chunks) ? (uint32_t)(key * (int)kv.ldkb + ch * 16) : STREAMS_OOR;
            blds16(rs, ks + s * KPLANE + wid * 1024, off, 0);
        }
    };
    auto load_v = [&](int sl, char* vs) {
        const StreamsKv& kv = p.kv[stream_of(sl)];
        const int kv0 = first_key(sl);
        const rsrc_t rs = make_rsrc(kv.vt + (int64_t)h * p.D * kv.ldvtb + (int64_t)b * kv.vtbsb + (int64_t)kv0 * ES, (int64_t)(p.D - 1) * kv.ldvtb + VROWB);
#pragma unroll
        for (int it = 0; it < VLI; ++it) {
            const int base = it * NTHR + wid * 64;  // a wave's 64 chunks are whole rows: the guard is wave-uniform
            if (base >= VROWS * VCPR) continue;
            const int q = base + lane, row = q / VCPR, cl = (q % VCPR) ^ swz<VROWB>(row);
            const uint32_t off = (row < p.D && kv0 + cl * EPC < kv.Lk) ? (uint32_t)(row * (int)kv.ldvtb + cl * 16) : STREAMS_OOR;
            blds16(rs, vs + base * 16, off, 0);
        }
    };

    if constexpr (RESIDENT) {  // K of every tile first: the scores need nothing else
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl)
            if (used(sl)) load_k(sl, smem + sl * SLOT);
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl)
            if (used(sl)) load_v(sl, smem + sl * SLOT + KBYTES);
    }

    // ---- Q fragments (B operand), predicated on the valid width ----
    frag_t qf[JQ][NS];
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq) {
        int qr = q0 + 16 * jq + c16;
        qr = qr < p.Lq ? qr : p.Lq - 1;
        const char* qp = p.q + (int64_t)b * p.qbsb + (int64_t)qr * p.ldqb + (int64_t)h * p.D * ES;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ch = 4 * s + g;
            qf[jq][s] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(qp + ch * 16) : zero;
        }
    }
    if constexpr (RESIDENT) {
        wait_vm0();
        __syncthreads();
    }

    // ---- S^T = K Q^T of every tile, masked by its stream's Lk ----
    f32x4 st[SLOTS][4][JQ];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        if (!used(sl)) continue;
        const char* ks = smem + (RESIDENT ? sl * SLOT : 0);
        if constexpr (!RESIDENT) {
            __syncthreads();  // the stage's previous tile has been read by every wave
            load_k(sl, smem);
            wait_vm0();
            __syncthreads();
        }
        const int kv0 = first_key(sl), Lk = p.kv[stream_of(sl)].Lk;
        const int nblk = is_half(sl) ? 2 : 4;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= nblk) {
#pragma unroll
                for (int jq = 0; jq < JQ; ++jq) st[sl][t][jq] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                continue;
            }
#pragma unroll
            for (int jq = 0; jq < JQ; ++jq) st[sl][t][jq] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int row = 16 * t + c16;
            const int off = row * 64 + ((g ^ ((row >> 2) & 3)) << 4);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const frag_t kf = lds_read_frag(ks, s * KPLANE + off);
#pragma unroll
                for (int jq = 0; jq < JQ; ++jq) mma_step<T>(st[sl][t][jq], kf, qf[jq][s]);
            }
        }
        if (kv0 + BKV > Lk) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + (IS_BF16 ? k_row_key(16 * t + 4 * g + r) : 16 * t + 4 * g + r);
                    if (key >= Lk) {
#pragma unroll
                        for (int jq = 0; jq < JQ; ++jq) st[sl][t][jq][r] = -INFINITY;
                    }
                }
        }
    }

    // ---- one exact softmax per stream: maximum, exponentials, row sum; P *= out_scale / l ----
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq) {
        float mx[2] = {-INFINITY, -INFINITY};
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            if (!used(sl)) continue;
            float m = st[sl][0][jq][0];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) m = fmaxf(m, st[sl][t][jq][r]);
            const bool s1 = stream_of(sl) != 0;
            mx[0] = s1 ? mx[0] : fmaxf(mx[0], m);
            mx[1] = s1 ? fmaxf(mx[1], m) : mx[1];
        }
        // (every used stream has a valid key in each of its tiles, so its maximum is finite; an unused stream's stays -inf and is not read)
        mx[0] = group_max<true>(mx[0]) * p.c;
        mx[1] = group_max<true>(mx[1]) * p.c;
        float ls[2] = {0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            if (!used(sl)) continue;
            const bool s1 = stream_of(sl) != 0;
            const float mc = s1 ? mx[1] : mx[0];
            float ps = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float e = fast_exp2(st[sl][t][jq][r] * p.c - mc);
                    if constexpr (IS_BF16) e = (float)(bf16_t)e;  // the value P V multiplies is what the row sum counts
                    st[sl][t][jq][r] = e;
                    ps += e;
                }
            ls[0] += s1 ? 0.f : ps;
            ls[1] += s1 ? ps : 0.f;
        }
        const float w0 = p.kv[0].out_scale / group_sum<true>(ls[0]);
        const float w1 = p.kv[1].out_scale / group_sum<true>(ls[1]);  // (one stream, or a skipped one: never multiplied)
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            if (!used(sl)) continue;
            const float w = stream_of(sl) ? w1 : w0;
#pragma unroll
            for (int t = 0; t < 4; ++t) st[sl][t][jq] *= w;
        }
    }

    // ---- O^T = sum over tiles of V^T P^T: both streams into one accumulator ----
    f32x4 o[ND][JQ];
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int jq = 0; jq < JQ; ++jq) o[i][jq] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        if (!used(sl)) continue;
        const char* vs = smem + (RESIDENT ? sl * SLOT + KBYTES : 0);
        if constexpr (!RESIDENT) {
            __syncthreads();
            load_v(sl, smem);
            wait_vm0();
            __syncthreads();
        }
        const int nblk = is_half(sl) ? 2 : 4;
        if constexpr (IS_BF16) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                if (2 * s2 >= nblk) continue;
                frag_t pb[JQ];
#pragma unroll
                for (int jq = 0; jq < JQ; ++jq) {
                    bf16x8 pk;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pk[r] = (bf16_t)st[sl][2 * s2][jq][r];
                        pk[4 + r] = (bf16_t)st[sl][2 * s2 + 1][jq][r];
                    }
                    pb[jq] = __builtin_bit_cast(frag_t, pk);
                }
#pragma unroll
                for (int i = 0; i < ND; ++i) {
                    const frag_t vf = lds_read_frag(vs, tile_off<VROWB>(16 * i + c16, 4 * s2 + g));  // one chunk = the lane's 8 consecutive keys
#pragma unroll
                    for (int jq = 0; jq < JQ; ++jq) mma_step<T>(o[i][jq], vf, pb[jq]);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t >= nblk) continue;
#pragma unroll
                for (int i = 0; i < ND; ++i) {
                    const frag_t vf = lds_read_frag(vs, tile_off<VROWB>(16 * i + c16, 4 * t + g));
#pragma unroll
                    for (int jq = 0; jq < JQ; ++jq) mma_step<T>(o[i][jq], vf, __builtin_bit_cast(frag_t, st[sl][t][jq]));
                }
            }
        }
    }

    // ---- store: the lane's elements d = 16 i + 4 g + r of query 16 jq + c16 ----
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq) {
        const int qr = q0 + 16 * jq + c16;
        if (qr >= p.Lq) continue;
        T* op = reinterpret_cast<T*>(p.out + (int64_t)b * p.obsb + (int64_t)qr * p.ldob) + (int64_t)h * p.D;
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int d0 = 16 * i + 4 * g;
            if (d0 + 4 > p.D) continue;  // (D is a multiple of 4)
            if constexpr (IS_BF16) {
                bf16x4 v4;
#pragma unroll
                for (int r = 0; r < 4; ++r) v4[r] = (bf16_t)o[i][jq][r];
                *reinterpret_cast<bf16x4*>(op + d0) = v4;
            } else {
                *reinterpret_cast<f32x4*>(op + d0) = o[i][jq];
            }
        }
    }
}

template <typename T, int NS, int ND, int JQ>
int streams_launch(const StreamsP& p0, int ntot, hipStream_t stream) {
    constexpr bool RESIDENT = sizeof(T) == 2;
    constexpr int KBYTES = NS * 64 * 64, VBYTES = ND * 16 * 64 * (int)sizeof(T);
    constexpr int LDS_MAX = RESIDENT ? STREAMS_SLOTS * (KBYTES + VBYTES) : (KBYTES > VBYTES ? KBYTES : VBYTES);
    static_assert(LDS_MAX <= 160 * 1024, "the tiles do not fit gfx950's LDS");
    auto kfn = attn_streams_kernel<T, NS, ND, JQ, RESIDENT>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        attr_set = true;
    }
    StreamsP p = p0;
    p.qtiles = (p.Lq + 64 * JQ - 1) / (64 * JQ);
    const int lds = RESIDENT ? ntot * (KBYTES + VBYTES) : LDS_MAX;
    hipLaunchKernelGGL(kfn, dim3((unsigned)((int64_t)p.qtiles * p.H * p.B)), dim3(256), lds, stream, p);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

// (K planes in 64-byte units of bfloat16 -- float32 takes twice as many --, 16-row blocks of V^T): the smallest pair that covers D is used
#define ATTN_STREAMS_INSTANCES(X)                    \
    X(2, 3)  /* head dim 40 (SD1.5 at 320 channels) */  \
    X(2, 4)  /* head dim 64 */                        \
    X(3, 5)  /* head dim 80 (SD1.5 at 640 channels) */  \
    X(4, 8)  /* head dim 128 */                       \
    X(5, 10) /* head dim 160 (SD1.5 at 1280 channels) */

template <typename T>
int streams_dispatch(const StreamsP& p, int ntot, hipStream_t st) {
    constexpr int PER = sizeof(T) == 2 ? 1 : 2;  // K planes per 32 columns
    const int ns = (p.D * (int)sizeof(T) + 63) / 64, nd = (p.D + 15) / 16;
    // 16-query waves where 128-query workgroups would leave CUs without one
    const bool narrow = (int64_t)((p.Lq + 127) / 128) * p.H * p.B < STREAMS_CUS;
#define TRY(NS_, ND_)                                                             \
    if (ns <= NS_ * PER && nd <= ND_)                                             \
        return narrow ? streams_launch<T, NS_ * PER, ND_, 1>(p, ntot, st) : streams_launch<T, NS_ * PER, ND_, 2>(p, ntot, st);
    ATTN_STREAMS_INSTANCES(TRY)
#undef TRY
    return MI355X_ESHAPE;
}

}  // namespace

extern "C" int mi355x_attention_streams(const mi355x_attn_args* a, void* stream) {
    if (!a || !a->q || !a->out) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->D <= 0 || a->nstream < 1 || a->nstream > 2) return MI355X_ESHAPE;
    if (a->D > 160 || (a->D * es) % 16 || a->D % 4) return MI355X_ESHAPE;
    if (!al16(a->q) || (a->ldq * es) % 16 || (a->q_batch_stride * es) % 16) return MI355X_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(a->out) & (4 * es - 1)) || a->ldo % 4 || a->o_batch_stride % 4) return MI355X_ESHAPE;
    if ((int64_t)((a->Lq + 63) / 64) * a->H * a->B > 0x7fffffff) return MI355X_ESHAPE;
    StreamsP p{};
    p.B = a->B, p.H = a->H, p.Lq = a->Lq, p.D = a->D, p.nstream = a->nstream;
    p.q = static_cast<const char*>(a->q), p.out = static_cast<char*>(a->out);
    p.ldqb = a->ldq * es, p.qbsb = a->q_batch_stride * es, p.ldob = a->ldo * es, p.obsb = a->o_batch_stride * es;
    p.c = a->scale * 1.44269504088896340736f;
    int ntot = 0;
    for (int s = 0; s < a->nstream; ++s) {
        const mi355x_kv_stream& k = a->kv[s];
        if (!k.k || !k.vt) return MI355X_EARG;
        if (k.Lk <= 0) return MI355X_ESHAPE;
        if (!al16(k.k) || !al16(k.vt) || (k.ldk * es) % 16 || (k.ldvt * es) % 16 || (k.k_batch_stride * es) % 16 || (k.vt_batch_stride * es) % 16) return MI355X_ESHAPE;
        // the loaders address a (batch, head) slice of a tile through a buffer descriptor with 32-bit offsets
        if (k.ldk < 0 || k.ldvt < 0 || 63 * k.ldk * es + a->D * es >= 0x7ffffff0LL || (int64_t)(a->D - 1) * k.ldvt * es + 64 * es >= 0x7ffffff0LL) return MI355X_ESHAPE;
        ntot += (k.Lk + 63) / 64;
        StreamsKv& d = p.kv[s];
        d.k = static_cast<const char*>(k.k), d.vt = static_cast<const char*>(k.vt);
        d.ldkb = k.ldk * es, d.kbsb = k.k_batch_stride * es, d.ldvtb = k.ldvt * es, d.vtbsb = k.vt_batch_stride * es;
        d.Lk = k.Lk, d.out_scale = k.out_scale;
    }
    if (ntot > STREAMS_SLOTS) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return a->dtype == MI355X_F32 ? streams_dispatch<float>(p, ntot, st) : streams_dispatch<bf16_t>(p, ntot, st);
}
