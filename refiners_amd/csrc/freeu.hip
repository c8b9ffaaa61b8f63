// mi355x_freeu_filter: FreeU's residual concatenator (reference latent_diffusion/freeu.py) in one launch.
//
// fourier_filter(x, scale, threshold) scales a small centred box of the 2-D spectrum and keeps the real part: per (image, channel) plane
// out = x + (scale - 1) P x with P real, symmetric and of rank 7 at threshold 1.  The host factors (scale - 1) P = S^T A into two tables of at
// most 16 rows (engine/freeu.py), and on token rows [B * HW][C] the filter is two skinny GEMMs with the pixels as the contraction:
//   moments  M[r][c] = sum_p A[r][p] x[p][c]          16 x C per image
//   update   out[p][c] = x[p][c] + sum_r S[r][p] M[r][c]
//
// Work split.  A workgroup of four waves owns one image and one slab of CS channels (CS = 16, 32 or 64, a compile-time choice: the slab
// width is what decides the number of workgroups -- SDXL's sites are 2 images x 1024 pixels x 1280 channels).
//   Phase 1: the slab's pixel rows in blocks of 128, wave w takes pixels 32 w .. 32 w + 31 of every block.  Table rows are the MFMA's M,
//     pixels its K, channels its N, so a wave keeps CS / 16 accumulator tiles of 16 x 16 moments.
//       bfloat16: rows are loaded with 16-byte vectors (8 channels of one pixel) into a tile of the wave's own in LDS and read back as B
//         fragments of 8 pixels of one channel -- the transpose the channels-last layout asks for; the next block's rows are in flight in
//         registers meanwhile.  The table fragment (8 floats of row c16) is split in registers into hi = bf16(a) and lo = bf16(a - hi):
//         two v_mfma_f32_16x16x32_bf16 per tile keep the table at float32-level accuracy (|a - hi - lo| <= 2^-16 |a|).
//       float32: v_mfma_f32_16x16x4_f32 takes one element per lane, so both operands come straight from memory, no LDS.
//     Pixels at or beyond HW are loaded as zeros (never the next image's rows); the table's columns there are zeros as well.
//     The four waves' partial moments meet in LDS and are summed in wave order: no atomics, bit-equal replays.
//   Phase 2: the workgroup walks the same rows again (its own phase 1 just pulled them through L2), a thread owns one 16-byte chunk of
//     channels and holds its moments in registers: RR fused multiply-adds per element (RR = 8 when the rank fits, else 16), one rounding.
// Workgroups behind the skip part scale the first half of the backbone rows in place, 16 bytes per lane; the other half is not touched.
#include "common.cuh"
#include "../../include/mi355x_refiners_freeu.h"

namespace {

struct FreeuP {
    int B, HW, C, nslab, nskip;  // nskip = B * nslab workgroups filter, the rest scale the backbone
    const char* skip;
    char* out;
    char* bb;
    int64_t ldsb, ldob, ldbb;  // row strides in bytes
    const float* ta;
    const float* ts;
    int64_t ldt;  // floats
    int rank8;    // the tables use at most 8 rows
    float bscale;
    int hchunks;        // 16-byte chunks of the scaled half of a backbone row
    int64_t bb_chunks;  // ... of all rows
};

// 32 channels: at SDXL's sites (2 x 1024 pixels x 1280 channels, 80 workgroups) 11.1 us in bfloat16 against 12.2 us at 16 (160 workgroups, half the
// bytes per row segment) and 16.8 us at 64 (40 workgroups); float32 25.1 / 28.9 / 46.5 us (docs/MEASUREMENTS_freeu.md)
constexpr int FREEU_DEFAULT_SLAB = 32;
int g_slab = 0;  // probing: 16 / 32 / 64 forces the slab width, anything else = the default

template <typename T, int CS, int RR>
MI_DEV void freeu_update(const FreeuP& p, const char* xin, char* xout, const float* mom, int c0, int tid) {
    constexpr int EPC = DT<T>::EPC, CPR = CS / EPC, RPI = 256 / CPR;
    const int ch = tid % CPR;
    if (c0 + ch * EPC + EPC > p.C) return;  // (the tail slab's chunks beyond C; no barrier follows)
    float m[RR][EPC];
#pragma unroll
    for (int r = 0; r < RR; ++r)
#pragma unroll
        for (int e = 0; e < EPC; ++e) m[r][e] = mom[r * CS + ch * EPC + e];
    for (int pix = tid / CPR; pix < p.HW; pix += RPI) {
        Vec16<T> v = load16(reinterpret_cast<const T*>(xin + (int64_t)pix * p.ldsb + ch * 16));
        float s[RR];
#pragma unroll
        for (int r = 0; r < RR; ++r) s[r] = p.ts[r * p.ldt + pix];
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            float a = v.get(e);
#pragma unroll
            for (int r = 0; r < RR; ++r) a = fmaf(s[r], m[r][e], a);
            v.set(e, a);
        }
        store16(reinterpret_cast<T*>(xout + (int64_t)pix * p.ldob + ch * 16), v);
    }
}

template <typename T, int CS>
__global__ __launch_bounds__(256) void freeu_kernel(const FreeuP p) {
    constexpr int ES = sizeof(T), NB = CS / 16;
    constexpr int PITCH = CS * 2 + 16;  // bfloat16 tile row: CS channels and one chunk of padding
    __shared__ __attribute__((aligned(16))) char tile[ES == 2 ? 4 * 32 * PITCH : 16];
    __shared__ float red[4 * 16 * CS];
    __shared__ float mom[16 * CS];

    const int tid = threadIdx.x, lane = tid & 63, wid = wave_id();
    const int g = lane >> 4, c16 = lane & 15;

    if ((int)blockIdx.x >= p.nskip) {  // ---- backbone[:, : C_b / 2] *= backbone_scale
        const int64_t step = (int64_t)(gridDim.x - p.nskip) * 256;
        for (int64_t i = (int64_t)(blockIdx.x - p.nskip) * 256 + tid; i < p.bb_chunks; i += step) {
            T* q = reinterpret_cast<T*>(p.bb + (i / p.hchunks) * p.ldbb + (i % p.hchunks) * 16);
            Vec16<T> v = load16(q);
#pragma unroll
            for (int e = 0; e < Vec16<T>::N; ++e) v.set(e, v.get(e) * p.bscale);
            store16(q, v);
        }
        return;
    }

    const int slab = blockIdx.x % p.nslab, b = blockIdx.x / p.nslab;
    const int c0 = slab * CS;
    const char* xin = p.skip + (int64_t)b * p.HW * p.ldsb + (int64_t)c0 * ES;
    char* xout = p.out + (int64_t)b * p.HW * p.ldob + (int64_t)c0 * ES;
    const int nit = (p.HW + 127) / 128;

    // ---- phase 1: M[r][c] = sum_p A[r][p] x[p][c]; acc[nb][i] = M[4 g + i][c0 + 16 nb + c16], this wave's pixels only
    f32x4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (ES == 2) {
        constexpr int CPR = CS / 8, NCH = CS / 16;  // chunks per tile row, chunks per lane (32 rows x CPR chunks over 64 lanes)
        char* mine = tile + wid * 32 * PITCH;
        const frag_t zero = frag_t{0, 0, 0, 0};
        frag_t stage[NCH];
        auto issue = [&](int it) {
            const int p0 = it * 128 + wid * 32;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int idx = j * 64 + lane, row = idx / CPR, ch = idx % CPR;
                const bool ok = p0 + row < p.HW && c0 + ch * 8 + 8 <= p.C;
                stage[j] = ok ? *reinterpret_cast<const frag_t*>(xin + (int64_t)(p0 + row) * p.ldsb + ch * 16) : zero;
            }
        };
        issue(0);
        for (int it = 0; it < nit; ++it) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int idx = j * 64 + lane;
                *reinterpret_cast<frag_t*>(mine + (idx / CPR) * PITCH + (idx % CPR) * 16) = stage[j];
            }
            if (it + 1 < nit) issue(it + 1);
            __syncthreads();
            // table fragment: columns it * 128 + wid * 32 + 8 g .. + 7 of row c16, as hi + lo
            const float* ap = p.ta + (int64_t)c16 * p.ldt + it * 128 + wid * 32 + 8 * g;
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap), a1 = *reinterpret_cast<const f32x4*>(ap + 4);
            bf16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = e < 4 ? a0[e] : a1[e - 4];
                const bf16_t h = (bf16_t)a;
                hi[e] = h;
                lo[e] = (bf16_t)(a - (float)h);
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const char* src = mine + 8 * g * PITCH + (nb * 16 + c16) * 2;  // pixels 8 g .. 8 g + 7 of channel 16 nb + c16
                bf16x8 x;
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const bf16_t*>(src + j * PITCH);
                acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, x, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, x, acc[nb], 0, 0, 0);
            }
            __syncthreads();  // (the tile is rewritten at the top of the next round)
        }
    } else {
        for (int it = 0; it < nit; ++it) {
            const int p0 = it * 128 + wid * 32;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int pix = p0 + 4 * s + g;  // K index g of this step
                const float a = p.ta[(int64_t)c16 * p.ldt + pix];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int c = nb * 16 + c16;
                    const float x = (pix < p.HW && c0 + c < p.C) ? *reinterpret_cast<const float*>(xin + (int64_t)pix * p.ldsb + c * 4) : 0.f;
                    acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x, acc[nb], 0, 0, 0);
                }
            }
        }
    }

    // ---- the four waves' partial moments, summed in wave order
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[(wid * 16 + 4 * g + i) * CS + nb * 16 + c16] = acc[nb][i];
    __syncthreads();
    for (int i = tid; i < 16 * CS; i += 256) mom[i] = ((red[i] + red[16 * CS + i]) + red[2 * 16 * CS + i]) + red[3 * 16 * CS + i];
    __syncthreads();

    // ---- phase 2: out[p][c] = x[p][c] + sum_r S[r][p] M[r][c]
    if (p.rank8) freeu_update<T, CS, 8>(p, xin, xout, mom, c0, tid);
    else freeu_update<T, CS, 16>(p, xin, xout, mom, c0, tid);
}

template <typename T, int CS>
int freeu_launch(const FreeuP& p0, hipStream_t stream) {
    FreeuP p = p0;
    p.nslab = (p.C + CS - 1) / CS;
    const int64_t nskip = (int64_t)p.B * p.nslab;
    const int64_t nbb = p.bb_chunks < 2048 ? 1 : p.bb_chunks / 2048 > 256 ? 256 : p.bb_chunks / 2048;  // about eight chunks per lane, at most one workgroup per CU
    if (nskip + nbb > 0x7fffffff) return MI355X_ESHAPE;
    p.nskip = (int)nskip;
    hipLaunchKernelGGL((freeu_kernel<T, CS>), dim3((unsigned)(nskip + nbb)), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

template <typename T>
int freeu_dispatch(const FreeuP& p, hipStream_t st) {
    const int cs = (g_slab == 16 || g_slab == 32 || g_slab == 64) ? g_slab : FREEU_DEFAULT_SLAB;
    return cs == 64 ? freeu_launch<T, 64>(p, st) : cs == 32 ? freeu_launch<T, 32>(p, st) : freeu_launch<T, 16>(p, st);
}

}  // namespace

// probing and A/B runs (native.UNSTABLE, not in the header): 16 / 32 / 64 channels per workgroup, anything else = the default
extern "C" int mi355x_freeu_set_slab(int channels) {
    g_slab = channels;
    return MI355X_OK;
}

extern "C" int mi355x_freeu_filter(const mi355x_freeu_args* a, const void* skip, int64_t ld_skip, void* skip_out, int64_t ld_out, void* backbone,
                                   int64_t ld_backbone, const float* analysis, const float* synthesis, int64_t ld_table, void* stream) {
    if (!a || !skip || !skip_out || !backbone || !analysis || !synthesis) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B < 1 || a->HW < 1 || a->C_skip < 1 || a->R < 1 || a->R > 16) return MI355X_ESHAPE;
    if (a->C_skip % 8 || a->C_b < 2 || a->C_b % 2 || (a->C_b / 2) % 8) return MI355X_ESHAPE;
    if (ld_skip < a->C_skip || ld_out < a->C_skip || ld_backbone < a->C_b) return MI355X_ESHAPE;
    if (ld_table % 128 || ld_table < a->HW || !(a->backbone_scale - a->backbone_scale == 0.f)) return MI355X_ESHAPE;
    if (!al16(skip) || !al16(skip_out) || !al16(backbone) || !al16(analysis) || !al16(synthesis)) return MI355X_ESHAPE;
    if ((ld_skip * es) % 16 || (ld_out * es) % 16 || (ld_backbone * es) % 16) return MI355X_ESHAPE;
    const int64_t rows = (int64_t)a->B * a->HW;
    const int64_t nskip = ((rows - 1) * ld_skip + a->C_skip) * es, nout = ((rows - 1) * ld_out + a->C_skip) * es, nbb = ((rows - 1) * ld_backbone + a->C_b) * es;
    if (overlap(skip, nskip, skip_out, nout) && !(skip == skip_out && ld_skip == ld_out)) return MI355X_ESHAPE;
    if (overlap(backbone, nbb, skip, nskip) || overlap(backbone, nbb, skip_out, nout)) return MI355X_ESHAPE;
    FreeuP p{};
    p.B = a->B, p.HW = a->HW, p.C = a->C_skip;
    p.skip = static_cast<const char*>(skip), p.out = static_cast<char*>(skip_out), p.bb = static_cast<char*>(backbone);
    p.ldsb = ld_skip * es, p.ldob = ld_out * es, p.ldbb = ld_backbone * es;
    p.ta = analysis, p.ts = synthesis, p.ldt = ld_table;
    p.rank8 = a->R <= 8;
    p.bscale = a->backbone_scale;
    p.hchunks = a->C_b / 2 * es / 16;
    p.bb_chunks = rows * p.hchunks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return a->dtype == MI355X_F32 ? freeu_dispatch<float>(p, st) : freeu_dispatch<bf16_t>(p, st);
}
