// The T2I-Adapter condition encoder's own kernels (reference latent_diffusion/t2i_adapter.py): mi355x_t2i_stem and mi355x_t2i_pool.
//
// mi355x_t2i_stem fuses PixelUnshuffle(r) with the 3 x 3 convolution behind it: an implicit GEMM straight off the NCHW picture,
//   out[pixel][n] = bias[n] + sum_k W[n][k] X[pixel][k],  k = (c, ky, dy | kx, dx).
// With K in that order the 3 r values over (kx, dx) of output pixel (oy, ox) are picture pixels (ox - 1) r .. (ox + 2) r - 1 of picture row
// (oy + ky - 1) r + dy, channel c: ONE contiguous run, and neighbouring output pixels' runs are r pixels apart.  So a strip of S output pixels
// of one output row needs, per (c, ky, dy), one run of (S + 2) r picture pixels, and every operand fragment is a 16-byte read of it.
//
// Work split.  A workgroup of four waves owns a strip of S = 16 MB consecutive output pixels of one output row and a chunk of 64 NB output
// channels.  The waves split the CHANNELS only: each holds all S pixels of its 16 NB channels (MB x NB accumulator tiles of 16 x 16), so a weight
// fragment is fetched by one wave of the workgroup and feeds MB MFMAs; the pixel fragments, which every wave reads, come from LDS.  Channels are
// the MFMA's rows and pixels its columns, so a lane ends up with four consecutive channels of one pixel: one 8- or 16-byte store.
// K loop.  One step = 8 picture rows of one (c, ky) (r = 8: all of dy; r = 16: half of it), K = 8 * 3 r.  A (c, ky) whose picture rows lie
// outside the picture is not a step at all (the top and bottom output rows run two of the three ky); columns outside it are zeros in the slab.
//   * the slab [8][(S + 2) r] goes global -> registers (16 bytes of float32 or 8 of bfloat16 per load, converted to the compute type) -> LDS,
//     two slabs: the loads of step s + 1 are issued before the MFMAs of step s and stored behind them, one barrier per step.
//   * pixel fragments: ds_read_b128 at column m r + j of row dy (j = kx r + dx, a multiple of the chunk).  In bfloat16 the 16 lanes of a group
//     are r * 2 = 16 or 32 bytes apart and the four groups fill the gaps or repeat a neighbour's chunk (a broadcast), so the reads do not
//     serialise on banks; rows are padded by one chunk so that fragments that straddle two dy do not collide.  float32 (twice the stride)
//     runs at a 2- to 4-way conflict: it is the accuracy mode.
//   * weight fragments come straight from global memory / L2: the host stores the weight chunk-major, [K / E][C0][E], so the 16 lanes of a
//     group read 256 contiguous bytes and the four groups four consecutive such runs.
// bfloat16 computes on v_mfma_f32_16x16x32_bf16, float32 on 4 x v_mfma_f32_16x16x4_f32 (common.cuh mma_step), accumulation in float32.
//
// mi355x_t2i_pool: AvgPool2d(2, 2) on channels-last rows, one 16-byte chunk per lane, float32 sum.
#include "common.cuh"
#include "../../include/mi355x_refiners_t2i.h"

namespace {

struct StemP {
    int B, cin, h, w, C0, nstrip, nchunk, pic_f32;
    const char* pic;
    const char* wgt;
    const char* bias;
    char* out;
    int64_t ldob;  // bytes
};

constexpr int STEM_ROWS = 8;  // picture rows per K step

template <typename T, int R, int MB, int NB>
struct StemCfg {
    static constexpr int ES = sizeof(T), EPC = DT<T>::EPC, KS = DT<T>::KSTEP;
    static constexpr int S = 16 * MB, CHUNK = 64 * NB;
    static constexpr int WS = (S + 2) * R;        // slab pixels per picture row
    static constexpr int PITCH = WS * ES + 16;    // bytes
    static constexpr int SLAB = STEM_ROWS * PITCH;
    static constexpr int UPR = WS / 4, UNITS = STEM_ROWS * UPR, NU = (UNITS + 255) / 256;  // 4-pixel load units
    static constexpr int NKK = STEM_ROWS * 3 * R / KS;  // MMA steps per K step
    static constexpr int HALVES = R / STEM_ROWS;
    static constexpr int LDS = 2 * SLAB;
};

template <typename T, int R, int MB, int NB>
__global__ __launch_bounds__(256) void t2i_stem_kernel(const StemP p) {
    using Cf = StemCfg<T, R, MB, NB>;
    constexpr int ES = Cf::ES, EPC = Cf::EPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = wave_id();
    const int g = lane >> 4, c16 = lane & 15;
    int bid = blockIdx.x;
    const int chunk = bid % p.nchunk;
    bid /= p.nchunk;
    const int strip = bid % p.nstrip;
    bid /= p.nstrip;
    const int oy = bid % p.h, b = bid / p.h;
    const int ox0 = strip * Cf::S, x0 = (ox0 - 1) * R;
    const int Hp = p.h * R, Wp = p.w * R;
    const int ky_lo = oy == 0 ? 1 : 0, nky = (oy == p.h - 1 ? 1 : 2) - ky_lo + 1;
    const int nsteps = p.cin * nky * Cf::HALVES;
    const int n0 = chunk * Cf::CHUNK + wid * NB * 16;

    f32x4 stage[Cf::NU];
    auto issue = [&](int s) {  // global -> registers: the slab of step s, as float32
        const int half = s % Cf::HALVES, t = s / Cf::HALVES;
        const int ky = ky_lo + t % nky, c = t / nky;
        const int64_t row0 = ((int64_t)(b * p.cin + c) * Hp + (oy + ky - 1) * R + half * STEM_ROWS) * Wp;
#pragma unroll
        for (int j = 0; j < Cf::NU; ++j) {
            const int u = j * 256 + tid, row = u / Cf::UPR, x = x0 + (u % Cf::UPR) * 4;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < Cf::UNITS && x >= 0 && x < Wp) {  // (x and Wp are multiples of 4: a unit is inside the picture or outside it)
                const int64_t e = row0 + (int64_t)row * Wp + x;
                if (p.pic_f32) {
                    v = *reinterpret_cast<const f32x4*>(p.pic + e * 4);
                } else {
                    const bf16x4 q = *reinterpret_cast<const bf16x4*>(p.pic + e * 2);
                    v = f32x4{(float)q[0], (float)q[1], (float)q[2], (float)q[3]};
                }
            }
            stage[j] = v;
        }
    };
    auto commit = [&](int buf) {  // registers -> LDS, in the compute type
        char* slab = smem + buf * Cf::SLAB;
#pragma unroll
        for (int j = 0; j < Cf::NU; ++j) {
            const int u = j * 256 + tid;
            if (u < Cf::UNITS) {
                char* dst = slab + (u / Cf::UPR) * Cf::PITCH + (u % Cf::UPR) * 4 * ES;
                if constexpr (ES == 4) {
                    *reinterpret_cast<f32x4*>(dst) = stage[j];
                } else {
                    *reinterpret_cast<bf16x4*>(dst) = bf16x4{(bf16_t)stage[j][0], (bf16_t)stage[j][1], (bf16_t)stage[j][2], (bf16_t)stage[j][3]};
                }
            }
        }
    };

    f32x4 acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    issue(0);
    commit(0);
    __syncthreads();
    const frag_t zero = frag_t{0, 0, 0, 0};
    for (int s = 0; s < nsteps; ++s) {
        if (s + 1 < nsteps) issue(s + 1);
        const char* slab = smem + (s & 1) * Cf::SLAB;
        const int half = s % Cf::HALVES, t = s / Cf::HALVES;
        const int ky = ky_lo + t % nky, c = t / nky;
        const int64_t kch0 = (int64_t)(((c * 3 + ky) * R + half * STEM_ROWS) * 3 * R) / EPC;  // first 16-byte K chunk of the step
#pragma unroll
        for (int kk = 0; kk < Cf::NKK; ++kk) {
            const int k = kk * Cf::KS + g * EPC, dy = k / (3 * R), j = k % (3 * R);  // this lane's chunk: k .. k + EPC - 1 of the step
            frag_t xf[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) xf[mb] = lds_read_frag(slab, dy * Cf::PITCH + ((mb * 16 + c16) * R + j) * ES);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int n16 = n0 + nb * 16;
                const frag_t wf = n16 < p.C0 ? *reinterpret_cast<const frag_t*>(p.wgt + ((kch0 + kk * 4 + g) * p.C0 + n16 + c16) * 16) : zero;
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) mma_step<T>(acc[mb][nb], wf, xf[mb]);
            }
        }
        if (s + 1 < nsteps) commit((s + 1) & 1);
        __syncthreads();
    }

    // acc[mb][nb][i] = channel n0 + 16 nb + 4 g + i of pixel ox0 + 16 mb + c16
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int ox = ox0 + mb * 16 + c16;
        if (ox >= p.w) continue;
        char* orow = p.out + ((int64_t)(b * p.h + oy) * p.w + ox) * p.ldob;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int n = n0 + nb * 16 + 4 * g;
            if (n >= p.C0) continue;
            f32x4 v = acc[mb][nb];
            if (p.bias) {
                const T* bp = reinterpret_cast<const T*>(p.bias) + n;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += to_f32(bp[i]);
            }
            if constexpr (ES == 4) {
                *reinterpret_cast<f32x4*>(orow + n * 4) = v;
            } else {
                *reinterpret_cast<bf16x4*>(orow + n * 2) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
            }
        }
    }
}

// 32 pixels x 64 channels: SDXL's 64 x 64 x 320 stem (r = 16) is 640 workgroups and takes 103 us in bfloat16, against 121 us at 64 x 64, 168 us at
// 32 x 128 and 195 us at 64 x 128; SD1.5's (r = 8) 19.2 / 22.1 / 24.6 / 28.3 us (docs/MEASUREMENTS_t2i.md): more, smaller workgroups hide the latency of
// the weight fragments, which come from L2
constexpr int T2I_DEFAULT_STRIP = 32, T2I_DEFAULT_CHUNK = 64;
int g_strip = 0, g_chunk = 0;  // probing: 32 / 64 pixels, 64 / 128 channels; anything else = the default

template <typename T, int R, int MB, int NB>
int stem_launch(const StemP& p0, hipStream_t stream) {
    using Cf = StemCfg<T, R, MB, NB>;
    auto kfn = t2i_stem_kernel<T, R, MB, NB>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, Cf::LDS);
        attr_set = true;
    }
    StemP p = p0;
    p.nstrip = (p.w + Cf::S - 1) / Cf::S;
    p.nchunk = (p.C0 + Cf::CHUNK - 1) / Cf::CHUNK;
    const int64_t grid = (int64_t)p.B * p.h * p.nstrip * p.nchunk;
    if (grid > 0x7fffffff) return MI355X_ESHAPE;
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(256), Cf::LDS, stream, p);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}

template <typename T, int R>
int stem_dispatch(const StemP& p, hipStream_t st) {
    const int strip = (g_strip == 32 || g_strip == 64) ? g_strip : T2I_DEFAULT_STRIP;
    const int chunk = (g_chunk == 64 || g_chunk == 128) ? g_chunk : T2I_DEFAULT_CHUNK;
    if (strip == 32) return chunk == 64 ? stem_launch<T, R, 2, 1>(p, st) : stem_launch<T, R, 2, 2>(p, st);
    return chunk == 64 ? stem_launch<T, R, 4, 1>(p, st) : stem_launch<T, R, 4, 2>(p, st);
}

template <typename T>
__global__ __launch_bounds__(256) void t2i_pool_kernel(const char* __restrict__ in, char* __restrict__ out, int H, int W, int cpr, int64_t total,
                                                       int64_t ldib, int64_t ldob) {
    const int OH = H / 2, OW = W / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ch = (int)(i % cpr);
        int64_t r = i / cpr;
        const int x = (int)(r % OW);
        r /= OW;
        const int y = (int)(r % OH);
        const int64_t b = r / OH;
        const char* src = in + ((b * H + 2 * y) * W + 2 * x) * ldib + ch * 16;
        const Vec16<T> a = load16(reinterpret_cast<const T*>(src)), bq = load16(reinterpret_cast<const T*>(src + ldib));
        const Vec16<T> c = load16(reinterpret_cast<const T*>(src + W * ldib)), d = load16(reinterpret_cast<const T*>(src + (W + 1) * ldib));
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < Vec16<T>::N; ++e) o.set(e, (((a.get(e) + bq.get(e)) + c.get(e)) + d.get(e)) * 0.25f);
        store16(reinterpret_cast<T*>(out + ((b * OH + y) * OW + x) * ldob + ch * 16), o);
    }
}

}  // namespace

// probing and A/B runs (native.UNSTABLE, not in the header): strip = 32 / 64 output pixels, chunk = 64 / 128 output channels per workgroup,
// anything else = the default
extern "C" int mi355x_t2i_set_strip(int strip, int chunk) {
    g_strip = strip, g_chunk = chunk;
    return MI355X_OK;
}

extern "C" int mi355x_t2i_stem(const mi355x_t2i_stem_args* a, const void* picture, const void* weight, const void* bias, void* out, int64_t ld_out,
                               void* stream) {
    if (!a || !picture || !weight || !out) return MI355X_EARG;
    if ((a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) || (a->pic_dtype != MI355X_F32 && a->pic_dtype != MI355X_BF16)) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2, pes = a->pic_dtype == MI355X_F32 ? 4 : 2;
    if ((a->r != 8 && a->r != 16) || (a->cin != 1 && a->cin != 3) || a->B < 1 || a->h < 1 || a->w < 1) return MI355X_ESHAPE;
    if (a->C0 < 16 || a->C0 % 16 || ld_out < a->C0) return MI355X_ESHAPE;
    if ((int64_t)a->h * a->r > 0x7fffffff / 64 || (int64_t)a->w * a->r > 0x7fffffff / 64 || (int64_t)a->B * a->cin > 0x7fffffff / 64) return MI355X_ESHAPE;
    if (!al16(picture) || !al16(weight) || !al16(out) || (ld_out * es) % 16) return MI355X_ESHAPE;
    const int64_t npic = (int64_t)a->B * a->cin * a->h * a->r * a->w * a->r * pes, nw = (int64_t)a->C0 * a->cin * 9 * a->r * a->r * es;
    const int64_t nout = (((int64_t)a->B * a->h * a->w - 1) * ld_out + a->C0) * es;
    if (overlap(out, nout, picture, npic) || overlap(out, nout, weight, nw) || overlap(out, nout, bias, (int64_t)a->C0 * es)) return MI355X_ESHAPE;
    StemP p{};
    p.B = a->B, p.cin = a->cin, p.h = a->h, p.w = a->w, p.C0 = a->C0, p.pic_f32 = a->pic_dtype == MI355X_F32;
    p.pic = static_cast<const char*>(picture), p.wgt = static_cast<const char*>(weight), p.bias = static_cast<const char*>(bias);
    p.out = static_cast<char*>(out), p.ldob = ld_out * es;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->dtype == MI355X_F32) return a->r == 8 ? stem_dispatch<float, 8>(p, st) : stem_dispatch<float, 16>(p, st);
    return a->r == 8 ? stem_dispatch<bf16_t, 8>(p, st) : stem_dispatch<bf16_t, 16>(p, st);
}

extern "C" int mi355x_t2i_pool(const mi355x_t2i_pool_args* a, const void* in, int64_t ld_in, void* out, int64_t ld_out, void* stream) {
    if (!a || !in || !out) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B < 1 || a->H < 2 || a->W < 2 || a->C < 1 || (a->C * es) % 16 || ld_in < a->C || ld_out < a->C) return MI355X_ESHAPE;
    if (!al16(in) || !al16(out) || (ld_in * es) % 16 || (ld_out * es) % 16) return MI355X_ESHAPE;
    const int OH = a->H / 2, OW = a->W / 2;
    const int64_t nin = (((int64_t)a->B * a->H * a->W - 1) * ld_in + a->C) * es, nout = (((int64_t)a->B * OH * OW - 1) * ld_out + a->C) * es;
    if (overlap(in, nin, out, nout)) return MI355X_ESHAPE;
    const int cpr = a->C * es / 16;
    const int64_t total = (int64_t)a->B * OH * OW * cpr;
    const int64_t want = (total + 255) / 256;
    const int grid = (int)(want < 1 ? 1 : want > 4096 ? 4096 : want);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->dtype == MI355X_F32)
        hipLaunchKernelGGL((t2i_pool_kernel<float>), dim3(grid), dim3(256), 0, st, static_cast<const char*>(in), static_cast<char*>(out), a->H, a->W, cpr, total, ld_in * es, ld_out * es);
    else
        hipLaunchKernelGGL((t2i_pool_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, static_cast<const char*>(in), static_cast<char*>(out), a->H, a->W, cpr, total, ld_in * es, ld_out * es);
    return hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH;
}
