// InformativeDrawings, the lineart preprocessor (src/refiners/foundationals/latent_diffusion/preprocessors/informative_drawings.py:8-107): the
// reflect-padded 7x7 stem, InstanceNorm2d statistics and apply over the three activation layouts of include/mi355x_refiners_lineart.h, and the
// head that normalises its halo tile on the way into LDS.  The 3x3 convolutions in between are mi355x_gemm's.  float32 arithmetic, float32 or
// bfloat16 storage; every output is written by exactly one lane and every reduction has a fixed order (no atomics: replays are bit-equal).
#include "common.cuh"
#include "../../include/mi355x_refiners.h"
#include "../../include/mi355x_refiners_lineart.h"

namespace {

#define LA_LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)

// 4 consecutive elements as float32 (16-byte load for float, 8-byte for bfloat16) and back
MI_DEV f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
MI_DEV f32x4 load4(const bf16_t* p) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
MI_DEV void store4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
MI_DEV void store4(bf16_t* p, f32x4 v) { *reinterpret_cast<bf16x4*>(p) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]}; }

// ReflectionPad2d's source index of padded index i - pad, for |overhang| < n; positions of a ragged tile further out are clamped (their
// values are never stored)
MI_DEV int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// Where logical pixel (b, y, x) of an H x W activation lives: (row, first column of its C channels).
struct Src {
    int layout, pad, H, W, C;
    MI_DEV int64_t row(int b, int y, int x) const {
        if (layout == MI355X_LINEART_PADDED) return ((int64_t)b * (H + 2 * pad) + y + pad) * (W + 2 * pad) + x + pad;
        if (layout == MI355X_LINEART_QUAD) return ((int64_t)b * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1);
        return ((int64_t)b * H + y) * W + x;
    }
    MI_DEV int col(int y, int x) const { return layout == MI355X_LINEART_QUAD ? ((y & 1) * 2 + (x & 1)) * C : 0; }
};

// ---------------------------------------------------------------------------------------------------- stem
constexpr int ST_T = 16;             // output tile: 16 x 16 pixels
constexpr int ST_HALO = ST_T + 6;    // with the 3-pixel halo
constexpr int ST_HPIX = ST_HALO * ST_HALO;

// grid (workgroups walking the tiles of all images round-robin).  LDS: the weights [Cin 49][64], once per workgroup, and per tile the halo
// [Cin][22][22] in float32 (reflected on load).  Wave v owns output channels 16 v .. 16 v + 15 of all 256 pixels (its weight reads are
// wave-uniform: LDS broadcasts); lane l owns pixels (x = l & 15, y = (l >> 4) + 4 j), j = 0 .. 3: 64 accumulators.
template <typename T>
__global__ __launch_bounds__(256) void lineart_stem_kernel(mi355x_lineart_stem_args a) {
    extern __shared__ __attribute__((aligned(16))) float st_lds[];
    const int Cin = a.Cin, H = a.H, W = a.W;
    float* ws = st_lds;                   // [Cin * 49][64]
    float* hs = st_lds + Cin * 49 * 64;   // [Cin][22][22]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < Cin * 49 * 16; i += 256) reinterpret_cast<f32x4*>(ws)[i] = reinterpret_cast<const f32x4*>(a.w)[i];
    f32x4 bv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bv[k] = a.bias ? reinterpret_cast<const f32x4*>(a.bias)[4 * wv + k] : f32x4{0.f, 0.f, 0.f, 0.f};
    const int tiles_x = (W + ST_T - 1) / ST_T, tiles_y = (H + ST_T - 1) / ST_T;
    const int64_t ntiles = (int64_t)a.B * tiles_x * tiles_y;
    const T* img = static_cast<const T*>(a.image);
    T* out = static_cast<T*>(a.out);
    const int px = lane & 15, py0 = lane >> 4;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / (tiles_x * tiles_y)), tt = (int)(tile % (tiles_x * tiles_y));
        const int ty0 = (tt / tiles_x) * ST_T, tx0 = (tt % tiles_x) * ST_T;
        __syncthreads();  // the previous tile's readers are done with hs
        for (int i = tid; i < Cin * ST_HPIX; i += 256) {
            const int ci = i / ST_HPIX, r = i - ci * ST_HPIX;
            const int hy = r / ST_HALO, hx = r - hy * ST_HALO;
            const int gy = reflect(ty0 + hy - 3, H), gx = reflect(tx0 + hx - 3, W);
            hs[i] = to_f32(img[(int64_t)b * a.batch_stride + (int64_t)ci * a.channel_stride + (int64_t)gy * a.row_stride + gx]);
        }
        __syncthreads();
        f32x4 acc[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[j][k] = bv[k];
        for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll 1
            for (int ky = 0; ky < 7; ++ky) {
                const float* hrow = hs + ci * ST_HPIX + (py0 + ky) * ST_HALO + px;
                const f32x4* wrow = reinterpret_cast<const f32x4*>(ws + ((ci * 7 + ky) * 7) * 64 + 16 * wv);
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    f32x4 wk[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) wk[k] = wrow[kx * 16 + k];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xv = hrow[4 * j * ST_HALO + kx];
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[j][k] += xv * wk[k];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gy = ty0 + py0 + 4 * j, gx = tx0 + px;
            if (gy < H && gx < W) {
                T* orow = out + (((int64_t)b * H + gy) * W + gx) * a.ldo + 16 * wv;
#pragma unroll
                for (int k = 0; k < 4; ++k) store4(orow + 4 * k, acc[j][k]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- InstanceNorm2d statistics
// (na, ma, Ma) <- (na, ma, Ma) + (nb, mb, Mb): Chan's pairwise update of (count, mean, M2)
MI_DEV void chan(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
    if (nb == 0.f) return;
    const float n = na + nb, d = mb - ma;
    ma += d * (nb / n);
    Ma += Mb + d * d * (na * nb / n);
    na = n;
}

constexpr int IN_MAX_SLABS = 1024;  // four workgroups per compute unit at full resolution; 128-row slabs below that
// source rows of one image, its columns, slab length and slab count (every slab holds at least one row)
struct Slabs {
    int Ns, Cc, L, S;
};
inline Slabs slabs_of(int H, int W, int C, int layout) {
    Slabs s;
    s.Ns = layout == MI355X_LINEART_QUAD ? (H / 2) * (W / 2) : H * W;
    s.Cc = layout == MI355X_LINEART_QUAD ? 4 * C : C;
    int want = (s.Ns + 127) / 128;
    want = want < 1 ? 1 : (want > IN_MAX_SLABS ? IN_MAX_SLABS : want);
    s.L = (s.Ns + want - 1) / want;
    s.S = (s.Ns + s.L - 1) / s.L;
    return s;
}

// grid (S, B).  Thread (cq, pl) walks rows n0 + pl, n0 + pl + PL, ... of its slab with Welford's update on 4 columns; the PL row lanes of a
// column meet in LDS, combined in lane order by thread (cq, 0).  ws [(b S + s)][Cc][2] = (mean, M2); the count of a slab is known to the reader.
template <typename T>
__global__ __launch_bounds__(256) void lineart_in_partial_kernel(mi355x_lineart_in_stats_args a, Slabs sl) {
    __shared__ __attribute__((aligned(16))) float sm_mean[256 * 4];
    __shared__ __attribute__((aligned(16))) float sm_m2[256 * 4];
    __shared__ float sm_cnt[256];
    const int tid = threadIdx.x, CQ = sl.Cc >> 2, PL = 256 / CQ;
    const int cq = tid % CQ, pl = tid / CQ;
    const int s = blockIdx.x, b = blockIdx.y;
    const int n0 = s * sl.L, n1 = min(sl.Ns, n0 + sl.L);
    const T* x = static_cast<const T*>(a.x) + 4 * cq;
    const int q = a.pad, W = a.W;
    f32x4 mean = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
#pragma unroll 4
    for (int n = n0 + pl; n < n1; n += PL) {  // (unrolled: the loads of four rows are in flight while Welford's chain runs)
        int64_t row;
        if (a.layout == MI355X_LINEART_PADDED) {
            const int y = n / W, xx = n - y * W;
            row = ((int64_t)b * (a.H + 2 * q) + y + q) * (W + 2 * q) + xx + q;
        } else {
            row = (int64_t)b * sl.Ns + n;
        }
        const f32x4 v = load4(x + row * a.ldx);
        cnt += 1;
        const float inv = 1.f / (float)cnt;
        const f32x4 d = v - mean;
        mean += d * inv;
        m2 += d * (v - mean);
    }
    *reinterpret_cast<f32x4*>(&sm_mean[4 * tid]) = mean;
    *reinterpret_cast<f32x4*>(&sm_m2[4 * tid]) = m2;
    sm_cnt[tid] = (float)cnt;
    __syncthreads();
    if (tid < CQ) {
        float n[4], mu[4], M[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) n[j] = (float)cnt, mu[j] = mean[j], M[j] = m2[j];
        for (int k = 1; k < PL; ++k) {
            const int o = k * CQ + tid;
#pragma unroll
            for (int j = 0; j < 4; ++j) chan(n[j], mu[j], M[j], sm_cnt[o], sm_mean[4 * o + j], sm_m2[4 * o + j]);
        }
        float* w = a.ws + (((int64_t)b * sl.S + s) * sl.Cc + 4 * tid) * 2;
        *reinterpret_cast<f32x4*>(w) = f32x4{mu[0], M[0], mu[1], M[1]};
        *reinterpret_cast<f32x4*>(w + 4) = f32x4{mu[2], M[2], mu[3], M[3]};
    }
}

// grid (C / 4, B).  Thread (cl, lane_s) combines slabs lane_s, lane_s + 64, ... (and the G column groups of each) of channel 4 blockIdx.x + cl
// in order (unrolled: the partials' loads do not wait for Chan's chain); the 64 slab lanes meet in LDS, combined in lane order.
__global__ __launch_bounds__(256) void lineart_in_final_kernel(const float* __restrict__ ws, float* __restrict__ stats, int C, int G, Slabs sl, float eps) {
    __shared__ float sn[256], smu[256], sM[256];
    const int tid = threadIdx.x, cl = tid & 3, lane_s = tid >> 2;
    const int c = blockIdx.x * 4 + cl, b = blockIdx.y;
    float n = 0.f, mu = 0.f, M = 0.f;
#pragma unroll 4
    for (int s = lane_s; s < sl.S; s += 64) {
        const float ns = (float)min(sl.L, sl.Ns - s * sl.L);
        for (int g = 0; g < G; ++g) {
            const f32x2 p = *reinterpret_cast<const f32x2*>(ws + (((int64_t)b * sl.S + s) * sl.Cc + g * C + c) * 2);
            chan(n, mu, M, ns, p[0], p[1]);
        }
    }
    sn[tid] = n, smu[tid] = mu, sM[tid] = M;
    __syncthreads();
    if (lane_s == 0) {
        for (int k = 1; k < 64; ++k) chan(n, mu, M, sn[4 * k + cl], smu[4 * k + cl], sM[4 * k + cl]);
        *reinterpret_cast<f32x2*>(stats + ((int64_t)b * C + c) * 2) = f32x2{mu, 1.f / sqrtf(M / n + eps)};
    }
}

// ---------------------------------------------------------------------------------------------------- InstanceNorm2d apply
// one thread per (pixel, 4 channels) of the LOGICAL image, grid-stride; the owner of an interior pixel writes its mirror images into the ring
template <typename T>
__global__ __launch_bounds__(256) void lineart_in_apply_kernel(mi355x_lineart_in_apply_args a) {
    const int H = a.H, W = a.W, C = a.C, CQ = C >> 2, p = a.ring;
    const Src src{a.layout, a.pad, H, W, C};
    const int64_t total = (int64_t)a.B * H * W * CQ;
    const T* x = static_cast<const T*>(a.x);
    const T* res = static_cast<const T*>(a.res);
    T* out = static_cast<T*>(a.out);
    const int OW = W + 2 * p, OH = H + 2 * p;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        const int64_t pix = i / CQ;
        const int xx = (int)(pix % W), yy = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
        const f32x4 v = load4(x + src.row(b, yy, xx) * a.ldx + src.col(yy, xx) + 4 * cq);
        const f32x4* st = reinterpret_cast<const f32x4*>(a.stats + ((int64_t)b * C + 4 * cq) * 2);
        const f32x4 s0 = st[0], s1 = st[1];  // (mean, rstd) of channels 4 cq, 4 cq + 1 | 4 cq + 2, 4 cq + 3
        f32x4 r = {(v[0] - s0[0]) * s0[1], (v[1] - s0[2]) * s0[3], (v[2] - s1[0]) * s1[1], (v[3] - s1[2]) * s1[3]};
        if (a.relu) r = f32x4{fmaxf(r[0], 0.f), fmaxf(r[1], 0.f), fmaxf(r[2], 0.f), fmaxf(r[3], 0.f)};
        if (res) {
            const int rp = a.res_pad;
            r += load4(res + (((int64_t)b * (H + 2 * rp) + yy + rp) * (W + 2 * rp) + xx + rp) * a.ldr + 4 * cq);
        }
        // output rows / columns this pixel lands on: itself, its mirror about the first row / column, its mirror about the last
        const int oy[3] = {yy + p, p - yy, p + 2 * (H - 1) - yy}, ox[3] = {xx + p, p - xx, p + 2 * (W - 1) - xx};
        const bool vy[3] = {true, yy >= 1 && yy <= p, yy <= H - 2 && yy >= H - 1 - p}, vx[3] = {true, xx >= 1 && xx <= p, xx <= W - 2 && xx >= W - 1 - p};
#pragma unroll
        for (int jy = 0; jy < 3; ++jy)
#pragma unroll
            for (int jx = 0; jx < 3; ++jx)
                if (vy[jy] && vx[jx]) store4(out + (((int64_t)b * OH + oy[jy]) * OW + ox[jx]) * a.ldo + 4 * cq, r);
    }
}

// ---------------------------------------------------------------------------------------------------- head
constexpr int HD_TW = 16, HD_TH = 8;                     // output pixels of one tile: four lanes per pair of pixels, 16 channels each
constexpr int HD_HW = HD_TW + 6, HD_HH = HD_TH + 6;      // the tile with its three-pixel halo
constexpr int HD_NPIX = HD_HW * HD_HH;                   // 308
constexpr int HD_ROW = 68;                               // floats per LDS pixel row: 64 + one 16-byte slot, so that consecutive pixels start one slot apart

// grid (tiles of an image taken round-robin, B).  Per tile: 16 lanes per halo pixel stage z = ReLU((x - mean) rstd) into LDS, the pixel found by
// reflection; then lane (pixel pair, channel quarter) sums its 2 x 49 x 16 products and the four quarters of a pair meet in two shuffles.
template <typename T>
__global__ __launch_bounds__(256) void lineart_head_kernel(mi355x_lineart_head_args a) {
    __shared__ __attribute__((aligned(16))) float zs[HD_NPIX * HD_ROW];
    __shared__ __attribute__((aligned(16))) float wl[49 * 64];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int H = a.H, W = a.W;
    const Src src{a.layout, a.pad, H, W, 64};
    for (int i = tid; i < 49 * 16; i += 256) reinterpret_cast<f32x4*>(wl)[i] = reinterpret_cast<const f32x4*>(a.w)[i];
    const int l16 = tid & 15;
    const f32x4* st = reinterpret_cast<const f32x4*>(a.stats + ((int64_t)b * 64 + 4 * l16) * 2);
    const f32x4 s0 = st[0], s1 = st[1];
    const f32x4 mean = {s0[0], s0[2], s1[0], s1[2]}, rstd = {s0[1], s0[3], s1[1], s1[3]};
    const int tiles_x = (W + HD_TW - 1) / HD_TW, tiles_y = (H + HD_TH - 1) / HD_TH;
    const int ntiles = tiles_x * tiles_y;
    const T* x = static_cast<const T*>(a.x);
    T* ob = static_cast<T*>(a.out) + (int64_t)b * a.out_batch_stride;
    // lane (pair, quarter): two horizontally adjacent pixels x 16 channels, so that a staged column serves both pixels and the weights of a tap
    // are read once per pair: 60 LDS reads per kernel row instead of 112
    const int quarter = tid & 3, pair = tid >> 2, px = (pair & 7) * 2, py = pair >> 3;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * HD_TH, tx0 = (tile % tiles_x) * HD_TW;
        __syncthreads();  // the previous tile's readers are done with zs (first tile: wl is written)
        for (int i = tid >> 4; i < HD_NPIX; i += 16) {
            const int hy = i / HD_HW, hx = i - hy * HD_HW;
            const int gy = reflect(ty0 + hy - 3, H), gx = reflect(tx0 + hx - 3, W);
            const f32x4 v = load4(x + src.row(b, gy, gx) * a.ldx + src.col(gy, gx) + 4 * l16);
            f32x4 z = (v - mean) * rstd;
            z = f32x4{fmaxf(z[0], 0.f), fmaxf(z[1], 0.f), fmaxf(z[2], 0.f), fmaxf(z[3], 0.f)};
            *reinterpret_cast<f32x4*>(&zs[i * HD_ROW + 4 * l16]) = z;
        }
        __syncthreads();
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {
            f32x4 wp[4] = {};  // the weights of the previous column's tap: the second pixel's tap at this column
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const f32x4* zr = reinterpret_cast<const f32x4*>(&zs[((py + ky) * HD_HW + px + c) * HD_ROW + quarter * 16]);
                f32x4 wc[4] = {};
                if (c < 7) {
                    const f32x4* wr = reinterpret_cast<const f32x4*>(&wl[(ky * 7 + c) * 64 + quarter * 16]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) wc[k] = wr[k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f32x4 zv = zr[k];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (c < 7) acc0 += zv[j] * wc[k][j];
                        if (c > 0) acc1 += zv[j] * wp[k][j];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) wp[k] = wc[k];
            }
        }
        acc0 += __shfl_xor(acc0, 1);
        acc0 += __shfl_xor(acc0, 2);
        acc1 += __shfl_xor(acc1, 1);
        acc1 += __shfl_xor(acc1, 2);
        const int gy = ty0 + py, gx = tx0 + px + quarter;  // quarter 0 stores the first pixel, quarter 1 the second
        const float v = quarter == 0 ? acc0 : acc1;
        if (quarter < 2 && gy < H && gx < W) ob[(int64_t)gy * W + gx] = from_f32<T>(1.f / (1.f + __expf(-(v + a.bias))));
    }
}

inline bool aligned_to(const void* p, int64_t ld_elems, int dtype, int elems) {  // pointer and leading dimension on `elems` elements
    const int64_t bytes = (int64_t)elems * (dtype == MI355X_F32 ? 4 : 2);
    return (reinterpret_cast<uintptr_t>(p) % bytes) == 0 && ld_elems % elems == 0;
}

// the checks every reader of a layout shares: MI355X_OK, or the code to return
inline int check_src(int dtype, int layout, int pad, int B, int H, int W, int C, const void* x, int64_t ldx) {
    if (!x || B <= 0 || H <= 0 || W <= 0 || layout < MI355X_LINEART_ROWS || layout > MI355X_LINEART_QUAD) return MI355X_EARG;
    if (dtype != MI355X_F32 && dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (pad < 0 || (pad != 0 && layout != MI355X_LINEART_PADDED)) return MI355X_ESHAPE;
    if (layout == MI355X_LINEART_QUAD && ((H & 1) || (W & 1))) return MI355X_ESHAPE;
    if (ldx < (layout == MI355X_LINEART_QUAD ? 4 * (int64_t)C : C) || !aligned_to(x, ldx, dtype, 4)) return MI355X_ESHAPE;
    return MI355X_OK;
}

}  // namespace

extern "C" int mi355x_lineart_stem(const mi355x_lineart_stem_args* a, void* stream) {
    if (!a || !a->image || !a->w || !a->out || a->B <= 0 || a->H <= 0 || a->W <= 0 || a->Cin <= 0) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->H < 4 || a->W < 4 || a->Cin > MI355X_LINEART_MAX_CIN || a->ldo < 64 || (reinterpret_cast<uintptr_t>(a->w) & 15)) return MI355X_ESHAPE;
    if ((a->bias && (reinterpret_cast<uintptr_t>(a->bias) & 15)) || !aligned_to(a->out, a->ldo, a->dtype, 4)) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntiles = (int64_t)a->B * ((a->W + ST_T - 1) / ST_T) * ((a->H + ST_T - 1) / ST_T);
    const dim3 grid((int)(ntiles < 768 ? ntiles : 768));  // three workgroups per compute unit (LDS), each loads the weights once
    const size_t lds = (size_t)a->Cin * (49 * 64 + ST_HPIX) * sizeof(float);
    if (a->dtype == MI355X_F32) hipLaunchKernelGGL((lineart_stem_kernel<float>), grid, dim3(256), lds, st, *a);
    else hipLaunchKernelGGL((lineart_stem_kernel<bf16_t>), grid, dim3(256), lds, st, *a);
    return LA_LAUNCH_OK();
}

extern "C" int64_t mi355x_lineart_in_stats_ws_floats(int32_t B, int32_t H, int32_t W, int32_t C, int32_t layout) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    const Slabs sl = slabs_of(H, W, C, layout);
    return (int64_t)B * sl.S * sl.Cc * 2;
}

extern "C" int mi355x_lineart_in_stats(const mi355x_lineart_in_stats_args* a, void* stream) {
    if (!a || !a->stats || !a->ws) return MI355X_EARG;
    const int st_src = check_src(a->dtype, a->layout, a->pad, a->B, a->H, a->W, a->C, a->x, a->ldx);
    if (st_src != MI355X_OK) return st_src;
    if ((a->C != 64 && a->C != 128 && a->C != 256) || a->B > 65535) return MI355X_ESHAPE;
    if (a->ws_floats < mi355x_lineart_in_stats_ws_floats(a->B, a->H, a->W, a->C, a->layout) || (reinterpret_cast<uintptr_t>(a->ws) & 15) || (reinterpret_cast<uintptr_t>(a->stats) & 7)) return MI355X_ESHAPE;
    const Slabs sl = slabs_of(a->H, a->W, a->C, a->layout);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->dtype == MI355X_F32) hipLaunchKernelGGL((lineart_in_partial_kernel<float>), dim3(sl.S, a->B), dim3(256), 0, st, *a, sl);
    else hipLaunchKernelGGL((lineart_in_partial_kernel<bf16_t>), dim3(sl.S, a->B), dim3(256), 0, st, *a, sl);
    if (hipGetLastError() != hipSuccess) return MI355X_ELAUNCH;
    hipLaunchKernelGGL(lineart_in_final_kernel, dim3(a->C / 4, a->B), dim3(256), 0, st, a->ws, a->stats, a->C, a->layout == MI355X_LINEART_QUAD ? 4 : 1, sl, a->eps);
    return LA_LAUNCH_OK();
}

extern "C" int mi355x_lineart_in_apply(const mi355x_lineart_in_apply_args* a, void* stream) {
    if (!a || !a->stats || !a->out) return MI355X_EARG;
    const int st_src = check_src(a->dtype, a->layout, a->pad, a->B, a->H, a->W, a->C, a->x, a->ldx);
    if (st_src != MI355X_OK) return st_src;
    if (a->C != 64 && a->C != 128 && a->C != 256) return MI355X_ESHAPE;
    if (a->ring < 0 || a->ring >= a->H || a->ring >= a->W || a->res_pad < 0 || (reinterpret_cast<uintptr_t>(a->stats) & 15)) return MI355X_ESHAPE;
    if (a->ldo < a->C || !aligned_to(a->out, a->ldo, a->dtype, 4)) return MI355X_ESHAPE;
    if (a->res && (a->ldr < a->C || !aligned_to(a->res, a->ldr, a->dtype, 4))) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t blocks = ((int64_t)a->B * a->H * a->W * (a->C / 4) + 255) / 256;
    const dim3 grid((int)(blocks < 4096 ? blocks : 4096));
    if (a->dtype == MI355X_F32) hipLaunchKernelGGL((lineart_in_apply_kernel<float>), grid, dim3(256), 0, st, *a);
    else hipLaunchKernelGGL((lineart_in_apply_kernel<bf16_t>), grid, dim3(256), 0, st, *a);
    return LA_LAUNCH_OK();
}

extern "C" int mi355x_lineart_head(const mi355x_lineart_head_args* a, void* stream) {
    if (!a || !a->stats || !a->w || !a->out) return MI355X_EARG;
    const int st_src = check_src(a->dtype, a->layout, a->pad, a->B, a->H, a->W, 64, a->x, a->ldx);
    if (st_src != MI355X_OK) return st_src;
    if (a->H < 4 || a->W < 4 || a->B > 65535 || (reinterpret_cast<uintptr_t>(a->w) & 15) || (reinterpret_cast<uintptr_t>(a->stats) & 15)) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ntiles = ((a->W + HD_TW - 1) / HD_TW) * ((a->H + HD_TH - 1) / HD_TH);
    int per_image = 1024 / a->B;  // about four workgroups' worth of tiles per compute unit in all; each loads the weights once
    per_image = per_image < 8 ? 8 : per_image;
    per_image = per_image > ntiles ? ntiles : per_image;
    const dim3 grid(per_image, a->B);
    if (a->dtype == MI355X_F32) hipLaunchKernelGGL((lineart_head_kernel<float>), grid, dim3(256), 0, st, *a);
    else hipLaunchKernelGGL((lineart_head_kernel<bf16_t>), grid, dim3(256), 0, st, *a);
    return LA_LAUNCH_OK();
}
