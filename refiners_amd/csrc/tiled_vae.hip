// Tiled VAE (auto_encoder.py:254-279, 466-591 of the reference): the two streaming passes around the per-tile encoder / decoder programs.
//   vae_tile_gather  T tiles of one size cut from the NCHW canvas -> a destination with explicit strides: the decoder's NCHW latent batch, or the
//                    encoder's token-major first activation with its channels zero-padded to one K block (no nchw_to_nhwc per tile)
//   vae_tile_blend   result / weights in gather form: one thread per canvas element finds the covering tiles of the GRID by arithmetic on the strides
//                    (at most ceil(tile / stride)^2 of them), walks them in list order and builds each weight from the ramp table -- no mask tensor
// Both HBM-bound.  Blend reads the tiles where the programs left them (explicit source strides: token-major rows of the decoder's last convolution,
// NCHW latents of the encoder).  float32 arithmetic, one rounding per product / sum / quotient (contraction is off in this file), which is what torch's
// separate mul / add / div kernels compute: in float32 blend gives the reference's bits.  No float atomics: replays are bit-equal.
#include "common.cuh"
#include "../../include/mi355x_refiners.h"

// every product and sum below is rounded on its own: the float32 results are compared bit for bit with torch's
#pragma clang fp contract(off)

namespace {

// Defined HERE, under the pragma (see multi_diffusion.hip: the runtime header's __fmul_rn / __fadd_rn fuse once inlined)
MI_DEV float mul_rn(float a, float b) { return a * b; }
MI_DEV float add_rn(float a, float b) { return a + b; }
MI_DEV float div_rn(float a, float b) { return a / b; }

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? MI355X_OK : MI355X_ELAUNCH)

inline int grid_for(int64_t work, int cap = 4096) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// MODE 0: one element per thread, any strides.  MODE 1: s_x == 1, a thread writes one 16-byte vector of a tile row.  MODE 2: s_c == 1, a thread writes
// one 16-byte vector of a pixel's (padded) channels.  grid (blocks, T); the canvas side is read by element in every mode (a row starts anywhere).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void vae_gather_kernel(const T* __restrict__ canvas, const mi355x_vae_tile_pos* __restrict__ pos, T* __restrict__ dst, int C, int cpad,
                                                          int h, int w, int H, int W, int64_t s_tile, int64_t s_c, int64_t s_y, int64_t s_x) {
    constexpr int EPC = DT<T>::EPC;
    const int t = blockIdx.y;
    const mi355x_vae_tile_pos p = pos[t];
    // the host validated its copy of the rows; a device row that left the contract since moves nothing
    if (p.top < 0 || p.left < 0 || p.top > H - h || p.left > W - w) return;
    T* d = dst + (int64_t)t * s_tile;
    const int64_t plane = (int64_t)H * W;
    const int64_t n = (int64_t)cpad * h * w / (MODE == 0 ? 1 : EPC);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
        if constexpr (MODE == 2) {  // q = (y, x, channel vector)
            const int nv = cpad / EPC;
            const int cv = (int)(q % nv);
            const int64_t px = q / nv;
            const int y = (int)(px / w), x = (int)(px - (int64_t)y * w);
            const T* s = canvas + (int64_t)(p.top + y) * W + p.left + x;
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const int c = cv * EPC + e;
                o.set(e, c < C ? to_f32(s[c * plane]) : 0.f);
            }
            store16<T>(d + y * s_y + x * s_x + cv * EPC, o);
        } else if constexpr (MODE == 1) {  // q = (c, y, x vector)
            const int nv = w / EPC;
            const int xv = (int)(q % nv);
            const int64_t r = q / nv;
            const int c = (int)(r / h), y = (int)(r - (int64_t)c * h);
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < EPC; ++e) o.set(e, c < C ? to_f32(canvas[c * plane + (int64_t)(p.top + y) * W + p.left + xv * EPC + e]) : 0.f);
            store16<T>(d + c * s_c + y * s_y + xv * EPC, o);
        } else {  // q = (c, y, x)
            const int x = (int)(q % w);
            const int64_t r = q / w;
            const int c = (int)(r / h), y = (int)(r - (int64_t)c * h);
            d[c * s_c + y * s_y + x * s_x] = c < C ? canvas[c * plane + (int64_t)(p.top + y) * W + p.left + x] : from_f32<T>(0.f);
        }
    }
}

// the ramp factor of tile-local position i on an axis of `len` positions: ramp[i] at the head unless the tile starts on the canvas edge, the flipped
// ramp at the tail unless it ends there (2 b <= len: the two never meet), else 1
MI_DEV float ramp_factor(const float* __restrict__ ramp, int b, int i, int len, bool head_edge, bool tail_edge) {
    if (i < b) return head_edge ? 1.f : ramp[i];
    if (i >= len - b) return tail_edge ? 1.f : ramp[len - 1 - i];
    return 1.f;
}

// One thread per VEC consecutive canvas elements of one row (VEC = 4: W % 4 == 0).  The axis table goes through LDS once per workgroup.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void vae_blend_kernel(T* __restrict__ canvas, const T* __restrict__ src, int64_t src_elems, const float* __restrict__ ramps, int64_t ramp_elems,
                                                         const mi355x_vae_axis* __restrict__ axis, const mi355x_vae_blend_tile* __restrict__ tiles, int C, int H, int W,
                                                         int nx, int ny, int stride_x, int stride_y, int tile_w, int tile_h) {
    __shared__ mi355x_vae_axis ax[MI355X_VAE_MAX_AXIS];
    for (int i = threadIdx.x; i < nx + ny; i += 256) {
        mi355x_vae_axis a = axis[i];
        const int size = i < nx ? W : H, idx = i < nx ? i : i - nx, stride = i < nx ? stride_x : stride_y, tile = i < nx ? tile_w : tile_h;
        // a row outside the contract (see vae_gather_kernel) covers nothing
        if (a.extent < 1 || a.extent > tile || a.start != idx * stride || a.start > size - a.extent) a.extent = 0;
        ax[i] = a;
    }
    __syncthreads();
    const int64_t total = (int64_t)C * H * W / VEC;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t i = q * VEC;
        const int c = (int)(i / ((int64_t)H * W));
        const int r = (int)(i - (int64_t)c * H * W);
        const int y = r / W, x0 = r - y * W;
        float num[VEC], cum[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) num[e] = 0.f, cum[e] = 0.f;
        int hit = 0;  // bit e: some tile holds element e
        // tiles whose nominal span [index * stride, index * stride + tile) reaches the element(s); the extents in LDS decide
        const int ix0 = max(0, (x0 - tile_w + stride_x) / stride_x), ix1 = min(nx - 1, (x0 + VEC - 1) / stride_x);
        const int iy0 = max(0, (y - tile_h + stride_y) / stride_y), iy1 = min(ny - 1, y / stride_y);
        for (int ix = ix0; ix <= ix1; ++ix) {  // list order: x outer, y inner (_generate_latent_tiles), the reference's summation order
            const mi355x_vae_axis cx = ax[ix];
            for (int iy = iy0; iy <= iy1; ++iy) {
                const mi355x_vae_axis cy = ax[nx + iy];
                const int ty = y - cy.start;
                if (ty < 0 || ty >= cy.extent) continue;
                const mi355x_vae_blend_tile d = tiles[ix * ny + iy];
                const int h = cy.extent, w = cx.extent, b = d.ramp_len;
                const bool ok = w > 0 && b >= 0 && 2 * b <= min(h, w) && d.ramp_off >= 0 && d.ramp_off + (int64_t)b <= ramp_elems && d.off >= 0 && d.s_c >= 0 && d.s_y >= 0 &&
                                d.s_x >= 0 && d.off + (C - 1) * d.s_c + (h - 1) * d.s_y + (w - 1) * d.s_x < src_elems;
                if (!ok) continue;
                const float* ramp = ramps + d.ramp_off;
                const float rv = ramp_factor(ramp, b, ty, h, cy.start == 0, cy.start + h == H);
                const T* row = src + d.off + c * d.s_c + ty * d.s_y;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int tx = x0 + e - cx.start;
                    if (tx < 0 || tx >= w) continue;
                    const float wgt = mul_rn(rv, ramp_factor(ramp, b, tx, w, cx.start == 0, cx.start + w == W));  // vertical, then horizontal
                    hit |= 1 << e;
                    num[e] = add_rn(num[e], wgt);
                    cum[e] = add_rn(cum[e], mul_rn(to_f32(row[tx * d.s_x]), wgt));
                }
            }
        }
        T* o = canvas + i;
        if (hit == 0) continue;  // no tile holds these elements: they keep their values
        if constexpr (VEC == 4) {
            T v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (hit >> e) & 1 ? from_f32<T>(div_rn(cum[e], num[e])) : o[e];
            if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
                *reinterpret_cast<bf16x4*>(o) = bf16x4{v[0], v[1], v[2], v[3]};
            }
        } else {
            o[0] = from_f32<T>(div_rn(cum[0], num[0]));
        }
    }
}

}  // namespace

extern "C" int mi355x_vae_tile_gather(const mi355x_vae_gather_args* a, void* stream) {
    if (!a || !a->canvas || !a->pos || !a->pos_host || !a->dst) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->T < 1 || a->T > 65535 || a->C < 1 || a->cpad < a->C || a->h < 1 || a->w < 1 || a->H < a->h || a->W < a->w) return MI355X_ESHAPE;
    if (a->s_tile < 0 || a->s_c < 0 || a->s_y < 0 || a->s_x < 0 || a->dst_elems < 1) return MI355X_ESHAPE;
    const int64_t last = (a->T - 1) * a->s_tile + (a->cpad - 1) * a->s_c + (a->h - 1) * a->s_y + (a->w - 1) * a->s_x;
    if (last >= a->dst_elems) return MI355X_ESHAPE;
    for (int t = 0; t < a->T; ++t) {
        const mi355x_vae_tile_pos& p = a->pos_host[t];
        if (p.top < 0 || p.left < 0 || p.top > a->H - a->h || p.left > a->W - a->w) return MI355X_ESHAPE;  // a tile outside the canvas
    }
    const int64_t es = a->dtype == MI355X_F32 ? 4 : 2, epc = 16 / es;
    if (overlap(a->dst, a->dst_elems * es, a->canvas, (int64_t)a->C * a->H * a->W * es)) return MI355X_EARG;
    int mode = 0;
    if (al16(a->dst) && a->s_tile % epc == 0) {
        if (a->s_x == 1 && a->w % epc == 0 && a->s_y % epc == 0 && a->s_c % epc == 0) mode = 1;
        else if (a->s_c == 1 && a->cpad % epc == 0 && a->s_y % epc == 0 && a->s_x % epc == 0) mode = 2;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)a->cpad * a->h * a->w;
    const dim3 grid(grid_for(mode ? n / epc : n), a->T);
#define VAE_GATHER(TT, M)                                                                                                                                         \
    hipLaunchKernelGGL((vae_gather_kernel<TT, M>), grid, dim3(256), 0, st, static_cast<const TT*>(a->canvas), a->pos, static_cast<TT*>(a->dst), a->C, a->cpad, a->h, \
                       a->w, a->H, a->W, a->s_tile, a->s_c, a->s_y, a->s_x)
#define VAE_GATHER_M(TT)                 \
    do {                                 \
        if (mode == 1) VAE_GATHER(TT, 1); \
        else if (mode == 2) VAE_GATHER(TT, 2); \
        else VAE_GATHER(TT, 0);          \
    } while (0)
    if (a->dtype == MI355X_F32) VAE_GATHER_M(float); else VAE_GATHER_M(bf16_t);
#undef VAE_GATHER_M
#undef VAE_GATHER
    return LAUNCH_OK();
}

extern "C" int mi355x_vae_tile_blend(const mi355x_vae_blend_args* a, void* stream) {
    if (!a || !a->canvas || !a->src || !a->axis || !a->axis_host || !a->tiles || !a->tiles_host) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    if (a->C < 1 || a->H < 1 || a->W < 1 || a->nx < 1 || a->ny < 1 || a->nx + a->ny > MI355X_VAE_MAX_AXIS) return MI355X_ESHAPE;
    if (a->stride_x < 1 || a->stride_y < 1 || a->tile_w < 1 || a->tile_h < 1 || a->src_elems < 1 || a->ramp_elems < 0 || (a->ramp_elems > 0 && !a->ramps)) return MI355X_ESHAPE;
    for (int i = 0; i < a->nx + a->ny; ++i) {
        const mi355x_vae_axis& s = a->axis_host[i];
        const bool isx = i < a->nx;
        const int size = isx ? a->W : a->H, idx = isx ? i : i - a->nx, stride = isx ? a->stride_x : a->stride_y, tile = isx ? a->tile_w : a->tile_h;
        if (s.extent < 1 || s.extent > tile || s.start != idx * stride || s.start > size - s.extent) return MI355X_ESHAPE;  // not the grid, or a tile outside the canvas
    }
    for (int ix = 0; ix < a->nx; ++ix)
        for (int iy = 0; iy < a->ny; ++iy) {
            const mi355x_vae_blend_tile& d = a->tiles_host[ix * a->ny + iy];
            const int64_t w = a->axis_host[ix].extent, h = a->axis_host[a->nx + iy].extent;
            if (d.ramp_len < 0 || 2 * (int64_t)d.ramp_len > (h < w ? h : w) || d.ramp_off < 0 || d.ramp_off + (int64_t)d.ramp_len > a->ramp_elems) return MI355X_ESHAPE;
            if (d.off < 0 || d.s_c < 0 || d.s_y < 0 || d.s_x < 0 || d.off + (a->C - 1) * d.s_c + (h - 1) * d.s_y + (w - 1) * d.s_x >= a->src_elems) return MI355X_EARG;
        }
    const int64_t es = a->dtype == MI355X_F32 ? 4 : 2, cn = (int64_t)a->C * a->H * a->W;
    if (overlap(a->canvas, cn * es, a->src, a->src_elems * es) || overlap(a->canvas, cn * es, a->ramps, a->ramp_elems * 4)) return MI355X_EARG;
    const bool vec = a->W % 4 == 0 && al16(a->canvas);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(vec ? cn / 4 : cn, 16384));
#define VAE_BLEND(TT, V)                                                                                                                                          \
    hipLaunchKernelGGL((vae_blend_kernel<TT, V>), grid, dim3(256), 0, st, static_cast<TT*>(a->canvas), static_cast<const TT*>(a->src), a->src_elems, a->ramps,     \
                       a->ramp_elems, a->axis, a->tiles, a->C, a->H, a->W, a->nx, a->ny, a->stride_x, a->stride_y, a->tile_w, a->tile_h)
    if (a->dtype == MI355X_F32) {
        if (vec) VAE_BLEND(float, 4); else VAE_BLEND(float, 1);
    } else {
        if (vec) VAE_BLEND(bf16_t, 4); else VAE_BLEND(bf16_t, 1);
    }
#undef VAE_BLEND
    return LAUNCH_OK();
}
