// mi355x_attention_joint: the self-attention of reference-only control (foundationals/latent_diffusion/reference_only_control.py of the
// reference, SelfAttentionInjectionAdapter) as one launch:
//   out[b] = mix[b] * softmax(scale * Q [K0 ; K1]^T) [V0 ; V1] + (1 - mix[b]) * softmax(scale * Q K0^T) V0
// Segment 0 is the sample's own keys, segment 1 the keys the guide pass projected at the same site.  The second term is the online
// softmax's own state at the moment segment 0 ends (O / l over the keys seen so far), so neither attention reads a key twice.
//
// The wave-level scheme is attention_general.hip's, copied (that file's instances are pinned by its kernel tests): S^T = K Q^T so a lane
// owns one query column, 32 queries per wave, 4 waves, 64-key tiles, register-staged double-buffered LDS, base-2 online softmax, for
// bf16 the lazy running maximum with row sums from the matrix pipe.  What differs:
//   * the key loop runs over segment 0's tiles, then segment 1's; each segment has its own pointers and strides, and its last tile is
//     masked by its own Lk (both segments may be a fraction of one tile);
//   * where segment 1 begins, a sample with 0 != mix != 1 writes (1 - mix) * O / l into the lane's own `out` elements and reads them
//     back in the final store.  The same lane writes and reads, so program order is all the ordering it needs; keeping the term in
//     registers would double the accumulator (80 more VGPRs at D = 160).  O and l share the reference maximum on the lazy path too,
//     so the quotient is exact there;
//   * mix is read from device memory per sample: mix == 1 skips the snapshot, mix == 0 skips segment 1 altogether.
#include "common.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_reference_only.h"

namespace {

struct JAttnP {
    int B, H, Lq, D, Lk0, Lk1;
    const char* q;
    const char* k0;
    const char* vt0;
    const char* k1;
    const char* vt1;
    const float* mix;
    char* out;
    int64_t ldqb, qbsb, ldk0b, k0bsb, ldvt0b, vt0bsb, ldk1b, k1bsb, ldvt1b, vt1bsb, ldob, obsb;  // bytes
    float c;    // scale * log2(e)
    float thr;  // FAST: a tile leaves the running maximum alone while no score exceeds it by more than thr = 8 / c
    int qtiles;
};

// lane <-> lane ^ 16 / lane ^ 32 as row / half swaps (gfx950): the maximum over a query's four lane groups without an LDS round trip
MI_DEV float group_max4(float x) {
    float a = x, b = x;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    a = fmaxf(a, b), b = a;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}

template <typename T, int NS, int ND, bool FAST>
__global__ __launch_bounds__(256) void attn_joint_kernel(const JAttnP p) {
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
    const int qk_chunks = (p.D * ES + 15) / 16;  // valid 16-byte chunks of a Q / K row of this head
    const frag_t zero = frag_t{0, 0, 0, 0};

    // ---- the sample's blend weight: uniform over the workgroup ----
    const float mixb = p.mix ? p.mix[b] : 1.f;
    const int nt0 = (p.Lk0 + BKV - 1) / BKV;
    const int ntile = nt0 + (mixb == 0.f ? 0 : (p.Lk1 + BKV - 1) / BKV);  // mix == 0: the plain attention over segment 0
    const bool snap = mixb != 1.f && mixb != 0.f;

    // ---- Q fragments (B operand), predicated on the valid width ----
    frag_t qf[2][NS];
#pragma unroll
    for (int jq = 0; jq < 2; ++jq) {
        int qr = q0 + 16 * jq + c16;
        qr = qr < p.Lq ? qr : p.Lq - 1;
        const char* qp = p.q + (int64_t)b * p.qbsb + (int64_t)qr * p.ldqb + (int64_t)h * p.D * ES;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ch = 4 * s + g;
            qf[jq][s] = ch < qk_chunks ? *reinterpret_cast<const frag_t*>(qp + ch * 16) : zero;
        }
    }

    const char* kbase0 = p.k0 + (int64_t)b * p.k0bsb + (int64_t)h * p.D * ES;
    const char* vbase0 = p.vt0 + (int64_t)h * p.D * p.ldvt0b + (int64_t)b * p.vt0bsb;
    const char* kbase1 = p.k1 + (int64_t)b * p.k1bsb + (int64_t)h * p.D * ES;
    const char* vbase1 = p.vt1 + (int64_t)h * p.D * p.ldvt1b + (int64_t)b * p.vt1bsb;
    const int krow = tid >> 2, kg = tid & 3;  // K loader: one 16-byte chunk of one key row per plane
    const int koff = krow * 64 + ((kg ^ ((krow >> 2) & 3)) << 4);
    frag_t kr[NS], vr[VLI];

    auto issue = [&](int tile) {
        const bool s1 = tile >= nt0;  // which segment the tile belongs to, and where it starts there
        const int kv0 = (s1 ? tile - nt0 : tile) * BKV;
        const int Lk = s1 ? p.Lk1 : p.Lk0;
        const char* kbase = s1 ? kbase1 : kbase0;
        const char* vbase = s1 ? vbase1 : vbase0;
        const int64_t ldkb = s1 ? p.ldk1b : p.ldk0b, ldvtb = s1 ? p.ldvt1b : p.ldvt0b;
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
            vr[it] = (row < p.D) ? *reinterpret_cast<const frag_t*>(vbase + (int64_t)row * ldvtb + (int64_t)kv0 * ES + pch * 16) : zero;
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

    // the lane's output elements: d = 16 i + 4 g + r of query 16 jq + c16
    auto out_row = [&](int jq) { return reinterpret_cast<T*>(p.out + (int64_t)b * p.obsb + (int64_t)(q0 + 16 * jq + c16) * p.ldob) + (int64_t)h * p.D; };
    auto row_sum = [&](int jq) {
        if constexpr (FAST) {
            return lacc[jq][0];
        } else {
            float l = lsum[jq];
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            return l;
        }
    };

    issue(0);
    commit(0);
    __syncthreads();

    for (int tile = 0; tile < ntile; ++tile) {
        const int cur = tile & 1;
        const bool more = tile + 1 < ntile;
        if (more) issue(tile + 1);
        const char* ks = smem + cur * STAGE;
        const char* vs = ks + KBYTES;
        const bool s1 = tile >= nt0;
        const int kv0 = (s1 ? tile - nt0 : tile) * BKV;
        const int Lk = s1 ? p.Lk1 : p.Lk0;

        // ---- segment boundary: park (1 - mix) * softmax(Q K0^T) V0 in the lane's own output elements ----
        if (snap && tile == nt0) {
#pragma unroll
            for (int jq = 0; jq < 2; ++jq) {
                const float w = (1.f - mixb) / row_sum(jq);  // (every lane: row_sum shuffles)
                if (q0 + 16 * jq + c16 >= p.Lq) continue;
                T* op = out_row(jq);
#pragma unroll
                for (int i = 0; i < ND; ++i) {
                    const int d0 = 16 * i + 4 * g;
                    if (d0 + 4 > p.D) continue;  // (D is a multiple of 4)
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
        // ---- mask: keys past the segment's own Lk ----
        if (kv0 + BKV > Lk) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + (IS_BF16 ? k_row_key(16 * t + 4 * g + r) : 16 * t + 4 * g + r);
                    if (key >= Lk) st[t][0][r] = -INFINITY, st[t][1][r] = -INFINITY;
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
                    const float mref = mnew == -INFINITY ? 0.f : mnew;
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

    // ---- store: mix * O / l, plus the parked term where one was kept ----
#pragma unroll
    for (int jq = 0; jq < 2; ++jq) {
        const float l = row_sum(jq);
        if (q0 + 16 * jq + c16 >= p.Lq) continue;
        const float inv = (snap ? mixb : 1.f) / l;
        T* op = out_row(jq);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int d0 = 16 * i + 4 * g;
            if (d0 + 4 > p.D) continue;
            if constexpr (IS_BF16) {
                bf16x4 v4;
                if (snap) {
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
                if (snap) v += *reinterpret_cast<const f32x4*>(op + d0);
                *reinterpret_cast<f32x4*>(op + d0) = v;
            }
        }
    }
}

template <typename T, int NS, int ND>
int launch_joint(const JAttnP& p0, hipStream_t stream) {
    constexpr int ES = sizeof(T);
    constexpr int LDS = 2 * (NS * 64 * 64 + ND * 16 * 64 * ES);
    auto kfn = attn_joint_kernel<T, NS, ND, ES == 2>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
        attr_set = true;
    }
    JAttnP p = p0;
    p.qtiles = (p.Lq + 127) / 128;
    hipLaunchKernelGGL(kfn, dim3(p.qtiles * p.H * p.B), dim3(256), LDS, stream, p);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

// (QK steps, PV blocks) instantiated: the smallest pair that covers D is used.  bf16: step = 32 columns; f32: step = 16 columns.
template <typename T>
int dispatch_joint(const JAttnP& p, hipStream_t st) {
    constexpr int KSTEP = DT<T>::KSTEP;
    const int ns = (p.D + KSTEP - 1) / KSTEP, nd = (p.D + 15) / 16;
#define TRY(NS_, ND_) \
    if (ns <= (NS_ * 32 / KSTEP) && nd <= ND_) return launch_joint<T, NS_ * 32 / KSTEP, ND_>(p, st);
    TRY(2, 3)    // head dim 40 (SD1.5 at 320 channels)
    TRY(2, 4)    // head dim 64
    TRY(3, 5)    // head dim 80 (SD1.5 at 640 channels)
    TRY(4, 8)    // head dim 128
    TRY(5, 10)   // head dim 160 (SD1.5 at 1280 channels)
#undef TRY
    return MI355X_ESHAPE;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// [p, p + n) and [q, q + m) (bytes) share a byte
inline bool overlap(const void* p, int64_t n, const void* q, int64_t m) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}
// bytes spanned by B batch rows of `rows` rows of `cols` elements
inline int64_t span(int64_t B, int64_t bs, int64_t rows, int64_t ld, int64_t cols, int es) { return ((B - 1) * bs + (rows - 1) * ld + cols) * es; }

}  // namespace

extern "C" int mi355x_attention_joint(const mi355x_attn_joint_args* a, void* stream) {
    if (!a || !a->q || !a->k0 || !a->vt0 || !a->k1 || !a->vt1 || !a->out) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->D <= 0 || a->Lk0 <= 0 || a->Lk1 <= 0 || a->D > 160) return MI355X_ESHAPE;
    // every head's Q / K row segment and every V^T row must start on a 16-byte boundary
    if ((a->D * es) % 16 || (a->ldq * es) % 16 || (a->ldk0 * es) % 16 || (a->ldvt0 * es) % 16 || (a->ldk1 * es) % 16 || (a->ldvt1 * es) % 16 || a->ldo % 4) return MI355X_ESHAPE;
    if ((a->q_batch_stride * es) % 16 || (a->k0_batch_stride * es) % 16 || (a->vt0_batch_stride * es) % 16 || (a->k1_batch_stride * es) % 16 ||
        (a->vt1_batch_stride * es) % 16 || a->o_batch_stride % 4)
        return MI355X_ESHAPE;
    if (!al16(a->q) || !al16(a->k0) || !al16(a->vt0) || !al16(a->k1) || !al16(a->vt1) || (reinterpret_cast<uintptr_t>(a->out) & (4 * es - 1)) ||
        (reinterpret_cast<uintptr_t>(a->mix) & 3))
        return MI355X_ESHAPE;
    const int64_t HD = (int64_t)a->H * a->D;
    const int64_t obytes = span(a->B, a->o_batch_stride, a->Lq, a->ldo, HD, es);
    const int64_t lp0 = ((int64_t)a->Lk0 + 63) / 64 * 64, lp1 = ((int64_t)a->Lk1 + 63) / 64 * 64;
    if (overlap(a->q, span(a->B, a->q_batch_stride, a->Lq, a->ldq, HD, es), a->out, obytes) ||
        overlap(a->k0, span(a->B, a->k0_batch_stride, a->Lk0, a->ldk0, HD, es), a->out, obytes) ||
        overlap(a->k1, span(a->B, a->k1_batch_stride, a->Lk1, a->ldk1, HD, es), a->out, obytes) ||
        overlap(a->vt0, span(a->B, a->vt0_batch_stride, HD, a->ldvt0, lp0, es), a->out, obytes) ||
        overlap(a->vt1, span(a->B, a->vt1_batch_stride, HD, a->ldvt1, lp1, es), a->out, obytes))
        return MI355X_EARG;
    JAttnP p{};
    p.B = a->B, p.H = a->H, p.Lq = a->Lq, p.D = a->D, p.Lk0 = a->Lk0, p.Lk1 = a->Lk1;
    p.q = static_cast<const char*>(a->q), p.out = static_cast<char*>(a->out), p.mix = static_cast<const float*>(a->mix);
    p.k0 = static_cast<const char*>(a->k0), p.vt0 = static_cast<const char*>(a->vt0), p.k1 = static_cast<const char*>(a->k1), p.vt1 = static_cast<const char*>(a->vt1);
    p.ldqb = a->ldq * es, p.qbsb = a->q_batch_stride * es, p.ldob = a->ldo * es, p.obsb = a->o_batch_stride * es;
    p.ldk0b = a->ldk0 * es, p.k0bsb = a->k0_batch_stride * es, p.ldvt0b = a->ldvt0 * es, p.vt0bsb = a->vt0_batch_stride * es;
    p.ldk1b = a->ldk1 * es, p.k1bsb = a->k1_batch_stride * es, p.ldvt1b = a->ldvt1 * es, p.vt1bsb = a->vt1_batch_stride * es;
    p.c = a->scale * 1.44269504088896340736f;
    p.thr = p.c > 0.f ? 8.0f / p.c : 0.f;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return a->dtype == MI355X_F32 ? dispatch_joint<float>(p, st) : dispatch_joint<bf16_t>(p, st);
}
