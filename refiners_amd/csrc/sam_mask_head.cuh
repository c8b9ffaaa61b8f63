// The SAM mask head, shared by mi355x_sam_mask_head (sam_decoder.hip) and mi355x_sam_mask_head_up (sam_hq.hip): ONE kernel body, so that
// the two entry points give the same bits.  STORE_U also writes the upscaled embedding the masks are contracted from.
#pragma once
#include "common.cuh"
#include "../../include/mi355x_refiners.h"

// 256 lanes = 4 waves: wave q = output quadrant (dy, dx), lane = one of 64 consecutive input pixels.  Per lane: the 32 output channels
// of ConvTranspose2d(64 -> 32, 2, 2) at (2y + dy, 2x + dx) (weights broadcast from LDS), + bias, GELU, then the dot products with the
// prompt's nk kept hypernetwork vectors -> low_res[p][kk][2y + dy][2x + dx].  Without STORE_U the upscaled embedding never leaves
// registers; with it the 32 channels also go to row (p, 2y + dy, 2x + dx) of u (ldu elements per row, 16-byte stores).
template <typename T, bool STORE_U>
__global__ __launch_bounds__(256) void sam_mask_head_kernel(mi355x_sam_mask_head_args a, T* __restrict__ u, int64_t ldu) {
    __shared__ float4 ws4[64][32];      // [ci][(q, co) / 4]
    __shared__ float xs[64][65];        // [pixel][ci]
    __shared__ float hs[4][32];
    __shared__ float bs[32];
    const int tid = threadIdx.x, q = tid >> 6, lane = tid & 63;
    const float4* w4 = reinterpret_cast<const float4*>(a.w);
    for (int i = tid; i < 64 * 32; i += 256) ws4[i / 32][i % 32] = w4[i];
    if (tid < 32) bs[tid] = a.bias[tid];
    const int HW = a.Hin * a.Win;
    const int tiles_per_img = (HW + 63) / 64;
    const int64_t ntiles = (int64_t)a.P * tiles_per_img;
    int p_loaded = -1;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int p = (int)(tile / tiles_per_img);
        const int pix0 = (int)(tile % tiles_per_img) * 64;
        __syncthreads();  // previous tile's readers are done with xs / hs
        if (p != p_loaded) {
            const T* hv = static_cast<const T*>(a.hyper) + (int64_t)p * a.hyper_batch_stride;
            if (tid < a.nk * 32) hs[tid / 32][tid % 32] = to_f32(hv[(int64_t)(tid / 32) * a.ld_hyper + tid % 32]);
            p_loaded = p;
        }
        const T* xb = static_cast<const T*>(a.x) + ((int64_t)p * HW + pix0) * a.ldx;
        for (int i = tid; i < 64 * 64; i += 256) {
            const int r = i >> 6, c = i & 63;
            xs[r][c] = pix0 + r < HW ? to_f32(xb[(int64_t)r * a.ldx + c]) : 0.f;
        }
        __syncthreads();
        float acc[32];
#pragma unroll
        for (int o = 0; o < 32; ++o) acc[o] = bs[o];
#pragma unroll 4
        for (int c = 0; c < 64; ++c) {
            const float xv = xs[lane][c];
#pragma unroll
            for (int o4 = 0; o4 < 8; ++o4) {
                const float4 wv = ws4[c][q * 8 + o4];
                acc[4 * o4 + 0] += xv * wv.x;
                acc[4 * o4 + 1] += xv * wv.y;
                acc[4 * o4 + 2] += xv * wv.z;
                acc[4 * o4 + 3] += xv * wv.w;
            }
        }
#pragma unroll
        for (int o = 0; o < 32; ++o) acc[o] = gelu_exact(acc[o]);
        const int pix = pix0 + lane;
        if (pix < HW) {
            const int yy = pix / a.Win, xx = pix % a.Win;
            const int Ho = 2 * a.Hin, Wo = 2 * a.Win;
            const int64_t opix = (int64_t)(2 * yy + (q >> 1)) * Wo + 2 * xx + (q & 1);
            T* ob = static_cast<T*>(a.out) + (int64_t)p * a.out_batch_stride;
            for (int kk = 0; kk < a.nk; ++kk) {
                float m = 0.f;
#pragma unroll
                for (int o = 0; o < 32; ++o) m += acc[o] * hs[kk][o];
                ob[(int64_t)kk * Ho * Wo + opix] = from_f32<T>(m);
            }
            if constexpr (STORE_U) {
                T* ur = u + ((int64_t)p * Ho * Wo + opix) * ldu;
#pragma unroll
                for (int o0 = 0; o0 < 32; o0 += Vec16<T>::N) {
                    Vec16<T> v;
#pragma unroll
                    for (int j = 0; j < Vec16<T>::N; ++j) v.set(j, acc[o0 + j]);
                    store16(ur + o0, v);
                }
            }
        }
    }
}
