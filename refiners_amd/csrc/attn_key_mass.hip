// mi355x_attention_key_mass: mass[b][j] = 1 / H * sum_h sum_i softmax_j(scale * q_i . k_j) -- the column sums of the attention matrix, which is all
// the Self-Attention Guidance tap reads (LoweredBlocks.sag_attention_mass).  The L x L matrix is never stored: two dependent launches form the
// scores twice on the matrix pipe and keep them in registers.  A column sum needs every row's normaliser before the first probability can be
// added, so the work splits at exactly that point:
//
//   Pass A (key_mass_rows_kernel): the row statistics.  A workgroup is (64-query tile, head, sample), four waves of 16 queries.  The wave's Q
//     fragments stay in registers; K tiles of 64 keys go through a double-buffered LDS ring, register-staged and laid out as the K planes of
//     attn_general_kernel.cuh (one MMA step's columns per plane, 16-byte chunks XOR-ed with (row >> 2) & 3), keys in natural order: there is no
//     P V here, so nothing wants the k_row_key permutation.  S^T = K Q^T (a lane owns query column c16), keys at or beyond L masked to -inf,
//     online softmax with the true running maximum and base-2 exponentials.  Lane group 0 stores lse2 = c * m + log2(l) for its 16 queries.
//   Pass B (key_mass_cols_kernel): the column mass.  A workgroup is (tile of 16 KB keys, sample); its four waves SPLIT THE HEADS (wave w takes
//     heads w, w + 4, ...), so a wave's loop has no workgroup barrier in it and a head count that is no multiple of four only shortens some
//     waves' loops.  Per head the wave holds the key tile's K fragments in registers as the A operand and walks all queries: the MFMA gives
//     S^T, in whose accumulator layout a lane holds four keys (4 g + r) of ONE query column (c16), so p = 2^(c s - lse2[query]) takes one lse2
//     value per lane and query block, and the per-key sums are plain register adds over every query block and every head of the wave.
//     Q streams through a ring of the wave's own in LDS, two stages of 16 QB queries, filled by LDS-DMA through a buffer descriptor
//     (raw_ptr_buffer_load_lds, attn_short_body.cuh): no staging registers, and a chunk beyond D or a query row at or beyond L carries an
//     out-of-range offset, for which the hardware writes zeros.  Such a query also gets lse2 = +inf and contributes an exact 0.
//     At the end: one reduction across the 16 lanes of a key row, one fixed-order sum of the four waves through LDS, times 1 / H, one store per key.
//   D is zero-padded to the MMA step in registers (the predicated fragment loads) and in LDS (the loaders), nothing is padded in HBM.
#include "attn_short_body.cuh"
#include "../../include/mi355x_refiners_key_mass.h"

namespace {

using mi355x_attn::blds16;
using mi355x_attn::make_rsrc;
using mi355x_attn::rsrc_t;

struct KeyMassP {
    int B, H, L, D;
    const char* q;
    const char* k;
    int64_t ldqb, qbsb, ldkb, kbsb;  // bytes
    float* lse;
    float* mass;
    int64_t ldl, ldm;  // floats
    float c;           // scale * log2(e)
    float inv_h;
    int tiles;         // pass A: query tiles per (sample, head); pass B: key tiles per sample
};

constexpr uint32_t KEY_MASS_OOR = 0x80000000u;  // beyond every descriptor's range: the load writes zeros
int g_key_tile = 0;                              // probing: 32 / 64 forces pass B's key-tile height, anything else = 16

// ---- pass A: lse2[b][h][i] of every score row ----
template <typename T, int NS>
__global__ __launch_bounds__(256) void key_mass_rows_kernel(const KeyMassP p) {
    constexpr int ES = sizeof(T);
    constexpr int BKV = 64, KPLANE = 64 * 64, STAGE = NS * KPLANE;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = wave_id();
    const int g = lane >> 4, c16 = lane & 15;
    int bid = blockIdx.x;
    const int qt = bid % p.tiles;
    bid /= p.tiles;
    const int h = bid % p.H;
    const int b = bid / p.H;
    const int q0 = qt * 64 + wid * 16;
    const int qk_chunks = p.D * ES / 16;  // 16-byte chunks of a Q / K row of this head (D * ES % 16 == 0)
    const frag_t zero = frag_t{0, 0, 0, 0};

    // Q fragments (B operand): chunk 4 s + g of query q0 + c16; a query at or beyond L reads the last row and stores nothing
    frag_t qf[NS];
    {
        const int qr = min(q0 + c16, p.L - 1);
        const char* qp = p.q + (int64_t)b * p.qbsb + (int64_t)qr * p.ldqb + (int64_t)h * p.D * ES;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ch = 4 * s + g;
            qf[s] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(qp + ch * 16) : zero;
        }
    }

    const char* kbase = p.k + (int64_t)b * p.kbsb + (int64_t)h * p.D * ES;
    const int krow = tid >> 2, kg = tid & 3;  // K loader: one 16-byte chunk of one key row per plane
    const int koff = krow * 64 + ((kg ^ ((krow >> 2) & 3)) << 4);
    frag_t kr[NS];
    auto issue = [&](int tile) {
        const int key = min(tile * BKV + krow, p.L - 1);  // (a key at or beyond L is masked below)
        const char* kp = kbase + (int64_t)key * p.ldkb;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ch = 4 * s + kg;
            kr[s] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(kp + ch * 16) : zero;
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int s = 0; s < NS; ++s) *reinterpret_cast<frag_t*>(smem + buf * STAGE + s * KPLANE + koff) = kr[s];
    };

    float mrun = -INFINITY, lsum = 0.f;  // the running maximum in score units, the lane group's share of the row sum
    const int ntile = (p.L + BKV - 1) / BKV;
    issue(0);
    commit(0);
    __syncthreads();
    for (int tile = 0; tile < ntile; ++tile) {
        const int cur = tile & 1;
        const bool more = tile + 1 < ntile;
        if (more) issue(tile + 1);
        const char* ks = smem + cur * STAGE;
        const int kv0 = tile * BKV;

        f32x4 st[4];  // S^T: keys kv0 + 16 t + 4 g + r of query c16
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int row = 16 * t + c16;
            const int off = row * 64 + ((g ^ ((row >> 2) & 3)) << 4);
#pragma unroll
            for (int s = 0; s < NS; ++s) mma_step<T>(st[t], lds_read_frag(ks, s * KPLANE + off), qf[s]);
        }
        if (kv0 + BKV > p.L) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kv0 + 16 * t + 4 * g + r >= p.L) st[t][r] = -INFINITY;
        }
        float mx = st[0][0];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[t][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mnew = fmaxf(mrun, mx);  // finite: every tile has a valid key
        const float alpha = fast_exp2((mrun - mnew) * p.c);
        const float mc = mnew * p.c;
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) ps += fast_exp2(st[t][r] * p.c - mc);
        lsum = lsum * alpha + ps;
        mrun = mnew;

        if (more) commit(cur ^ 1);
        __syncthreads();
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (g == 0 && q0 + c16 < p.L) p.lse[((int64_t)b * p.H + h) * p.ldl + q0 + c16] = mrun * p.c + __log2f(lsum);
}

// ---- pass B: the mass of the 16 KB keys of a tile, over every head and every query ----
// queries per ring stage: a wave's two stages stay at or below 20 KB, the workgroup's four rings at or below 80 KB
template <int NS> constexpr int key_mass_qb() { return NS <= 2 ? 4 : NS <= 5 ? 2 : 1; }

template <typename T, int NS, int KB>
__global__ __launch_bounds__(256) void key_mass_cols_kernel(const KeyMassP p) {
    constexpr int ES = sizeof(T);
    constexpr int QB = key_mass_qb<NS>(), QT = 16 * QB, KT = 16 * KB;
    constexpr int BLK = 16 * 64;  // one 16-query block of one plane: what one DMA instruction of a wave fills
    constexpr int STAGE = NS * QB * BLK, RING = 2 * STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = wave_id();
    const int g = lane >> 4, c16 = lane & 15;
    const int kt = blockIdx.x % p.tiles, b = blockIdx.x / p.tiles;
    const int k0 = kt * KT;
    const int qk_chunks = p.D * ES / 16;
    const int nqt = (p.L + QT - 1) / QT;
    const frag_t zero = frag_t{0, 0, 0, 0};
    char* ring = smem + wid * RING;
    float* red = reinterpret_cast<float*>(smem + 4 * RING);  // [4 waves][KT]

    // loader lane -> (row lane >> 2 of a 16-query block, physical slot lane & 3): the logical chunk that slot holds, and where a fragment read finds its own
    const int lrow = lane >> 2, lkg = (lane & 3) ^ ((lrow >> 2) & 3);
    const int roff = c16 * 64 + ((g ^ ((c16 >> 2) & 3)) << 4);

    f32x4 col[KB];  // keys k0 + 16 j + 4 g + r, summed over the queries c16, c16 + 16, ... of this wave's heads
#pragma unroll
    for (int j = 0; j < KB; ++j) col[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int h = wid; h < p.H; h += 4) {  // (wave-uniform)
        frag_t kf[KB][NS];  // A operand: chunk 4 s + g of key k0 + 16 j + c16; a key at or beyond L reads the last row and is not stored
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const int key = min(k0 + 16 * j + c16, p.L - 1);
            const char* kp = p.k + (int64_t)b * p.kbsb + (int64_t)key * p.ldkb + (int64_t)h * p.D * ES;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int ch = 4 * s + g;
                kf[j][s] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(kp + ch * 16) : zero;
            }
        }
        const rsrc_t rs = make_rsrc(p.q + (int64_t)b * p.qbsb + (int64_t)h * p.D * ES, (int64_t)(p.L - 1) * p.ldqb + p.D * ES);
        const float* lse = p.lse + ((int64_t)b * p.H + h) * p.ldl;
        auto issue = [&](int qt, char* stage) {  // NS * QB DMA instructions
#pragma unroll
            for (int jb = 0; jb < QB; ++jb) {
                const int row = qt * QT + 16 * jb + lrow;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int ch = 4 * s + lkg;
                    const uint32_t off = (row < p.L && ch < qk_chunks) ? (uint32_t)(row * (int)p.ldqb + ch * 16) : KEY_MASS_OOR;
                    blds16(rs, stage + (s * QB + jb) * BLK, off, 0);
                }
            }
        };

        // (the stage written here was last read by MFMAs that have been issued: the ring is the wave's own, program order is all it needs)
        issue(0, ring);
        for (int qt = 0; qt < nqt; ++qt) {
            const char* cur = ring + (qt & 1) * STAGE;
            float ls[QB];
#pragma unroll
            for (int jb = 0; jb < QB; ++jb) {
                const int qi = qt * QT + 16 * jb + c16;
                ls[jb] = qi < p.L ? lse[qi] : INFINITY;
            }
            if (qt + 1 < nqt) {
                issue(qt + 1, ring + ((qt + 1) & 1) * STAGE);
                wait_vm<NS * QB>();  // all but the newest NS * QB vector-memory operations: this tile has landed, the next may be in flight
            } else {
                wait_vm0();
            }
#pragma unroll
            for (int jb = 0; jb < QB; ++jb) {
                f32x4 st[KB];
#pragma unroll
                for (int j = 0; j < KB; ++j) st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const frag_t qf = lds_read_frag(cur, (s * QB + jb) * BLK + roff);
#pragma unroll
                    for (int j = 0; j < KB; ++j) mma_step<T>(st[j], kf[j][s], qf);
                }
#pragma unroll
                for (int j = 0; j < KB; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) col[j][r] += fast_exp2(st[j][r] * p.c - ls[jb]);
            }
        }
    }

    // ---- the 16 query lanes of a key row, then the four waves in a fixed order ----
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = col[j][r];
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            v += __shfl_xor(v, 8);
            if (c16 == 0) red[wid * KT + 16 * j + 4 * g + r] = v;
        }
    __syncthreads();
    if (tid < KT && k0 + tid < p.L)
        p.mass[(int64_t)b * p.ldm + k0 + tid] = (((red[tid] + red[KT + tid]) + red[2 * KT + tid]) + red[3 * KT + tid]) * p.inv_h;
}

template <typename T, int NS>
int key_mass_rows_launch(const KeyMassP& p0, hipStream_t stream) {
    constexpr int LDS = 2 * NS * 64 * 64;
    auto kfn = key_mass_rows_kernel<T, NS>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_set = true;
    }
    KeyMassP p = p0;
    p.tiles = (p.L + 63) / 64;
    hipLaunchKernelGGL(kfn, dim3((unsigned)((int64_t)p.tiles * p.H * p.B)), dim3(256), LDS, stream, p);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

template <typename T, int NS, int KB>
int key_mass_cols_launch(const KeyMassP& p0, hipStream_t stream) {
    constexpr int LDS = 4 * 2 * NS * key_mass_qb<NS>() * 16 * 64 + 4 * 16 * KB * (int)sizeof(float);
    static_assert(LDS <= 160 * 1024, "the rings do not fit gfx950's LDS");
    auto kfn = key_mass_cols_kernel<T, NS, KB>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_set = true;
    }
    KeyMassP p = p0;
    p.tiles = (p.L + 16 * KB - 1) / (16 * KB);
    hipLaunchKernelGGL(kfn, dim3((unsigned)((int64_t)p.tiles * p.B)), dim3(256), LDS, stream, p);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

// Key-tile height of pass B.  A workgroup walks every head and every query of its sample, so the grid is ceil(L / height) * B workgroups for 256 CUs
// and a wave's walk is one dependent chain per Q tile.  The 16-key tile gives the most workgroups and was the fastest at every shape measured
// (SDXL's and SD1.5's middle blocks, one and four samples, both dtypes: docs/MEASUREMENTS_sag_mass.md), so it is the one taken; the 32- and 64-key
// instances re-read Q less often and stay reachable for measurements at shapes not yet taken.
int key_mass_tile() { return (g_key_tile == 32 || g_key_tile == 64) ? g_key_tile : 16; }

// MMA steps of 32 bfloat16 columns (float32 takes twice as many steps of 16): the smallest that covers D
#define KEY_MASS_INSTANCES(X) \
    X(2) /* head dim 40, 64 */ \
    X(3) /* head dim 80, 96 */ \
    X(4) /* head dim 128 */    \
    X(5) /* head dim 160 */

template <typename T>
int key_mass_dispatch(const KeyMassP& p, hipStream_t st) {
    constexpr int PER = sizeof(T) == 2 ? 1 : 2;
    const int ns = (p.D + DT<T>::KSTEP - 1) / DT<T>::KSTEP;
    const int kt = key_mass_tile();
#define TRY(NS_)                                                                                              \
    if (ns <= NS_ * PER) {                                                                                    \
        const int rc = key_mass_rows_launch<T, NS_ * PER>(p, st);                                             \
        if (rc != MI355X_OK) return rc;                                                                       \
        return kt == 64 ? key_mass_cols_launch<T, NS_ * PER, 4>(p, st)                                        \
             : kt == 32 ? key_mass_cols_launch<T, NS_ * PER, 2>(p, st) : key_mass_cols_launch<T, NS_ * PER, 1>(p, st); \
    }
    KEY_MASS_INSTANCES(TRY)
#undef TRY
    return MI355X_ESHAPE;
}

}  // namespace

// probing and A/B runs (native.UNSTABLE, not in the header): 32 / 64 keys per pass-B workgroup, anything else = the default 16
extern "C" int mi355x_key_mass_set_tile(int keys) {
    g_key_tile = keys;
    return MI355X_OK;
}

extern "C" int mi355x_attention_key_mass(const mi355x_key_mass_args* a, const void* q, int64_t ldq, int64_t q_batch_stride, const void* k, int64_t ldk,
                                         int64_t k_batch_stride, float* lse, int64_t ldl, float* mass, int64_t ldm, void* stream) {
    if (!a || !q || !k || !lse || !mass) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B <= 0 || a->H <= 0 || a->L <= 0 || a->D <= 0) return MI355X_ESHAPE;
    if (a->D > 160 || (a->D * es) % 16) return MI355X_ESHAPE;
    if (ldl < a->L || ldm < a->L || !(a->scale > 0.f) || !(a->scale < INFINITY)) return MI355X_ESHAPE;
    if (!al16(q) || !al16(k) || (ldq * es) % 16 || (ldk * es) % 16 || (q_batch_stride * es) % 16 || (k_batch_stride * es) % 16) return MI355X_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(lse) & 3) || (reinterpret_cast<uintptr_t>(mass) & 3)) return MI355X_ESHAPE;
    // pass B addresses a (batch, head) slice of Q through a buffer descriptor with 32-bit offsets; K keeps the same rule
    if (ldq < 0 || ldk < 0 || ldq > 0x7fffffff || ldk > 0x7fffffff) return MI355X_ESHAPE;
    if (((int64_t)(a->L - 1) * ldq + a->D) * es >= 0x7ffffff0LL || ((int64_t)(a->L - 1) * ldk + a->D) * es >= 0x7ffffff0LL) return MI355X_ESHAPE;
    if ((int64_t)((a->L + 63) / 64) * a->H * a->B > 0x7fffffff || (int64_t)((a->L + 15) / 16) * a->B > 0x7fffffff) return MI355X_ESHAPE;
    KeyMassP p{};
    p.B = a->B, p.H = a->H, p.L = a->L, p.D = a->D;
    p.q = static_cast<const char*>(q), p.k = static_cast<const char*>(k);
    p.ldqb = ldq * es, p.qbsb = q_batch_stride * es, p.ldkb = ldk * es, p.kbsb = k_batch_stride * es;
    p.lse = lse, p.mass = mass, p.ldl = ldl, p.ldm = ldm;
    p.c = a->scale * 1.44269504088896340736f;
    p.inv_h = 1.f / (float)a->H;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return a->dtype == MI355X_F32 ? key_mass_dispatch<float>(p, st) : key_mass_dispatch<bf16_t>(p, st);
}
