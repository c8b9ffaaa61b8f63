/*
 * mi355x_refiners_t2i.h -- the T2I-Adapter condition encoder's own kernels (refiners_amd/csrc/t2i.hip; reference
 * latent_diffusion/t2i_adapter.py, ConditionEncoder / ConditionEncoderXL): the pixel-unshuffle stem and the 2 x 2 average pool.
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1), return value 0 or one of that header's negative MI355X_E*
 * codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its outputs untouched.  The calls do
 * not allocate, synchronise with the host, keep a pointer past their return or use atomics: every output element is written by exactly
 * one lane and every sum has a fixed order, replays are bit-equal.
 *
 * mi355x_t2i_stem: Conv2d(cin r^2 -> C0, 3 x 3, padding 1) of PixelUnshuffle(r) of an NCHW picture, as channels-last rows; the
 * unshuffled tensor is never written.
 *   out[(b h + oy) w + ox][n] = bias[n] + sum over c < cin, ky < 3, dy < r, kx < 3, dx < r of
 *                               weight(n, c, ky, dy, kx, dx) * picture[b][c][(oy + ky - 1) r + dy][(ox + kx - 1) r + dx]     (0 outside the picture)
 *   picture  [B][cin][r h][r w], contiguous, of pic_dtype
 *   weight   the convolution's weight [C0][cin r^2][3][3] (unshuffled channel c r^2 + dy r + dx) re-ordered to K = (c, ky, dy, kx, dx)
 *            and stored in 16-byte chunks of K, chunk-major: [K / E][C0][E] with E = 16 / sizeof(dtype) -- refiners_amd.native.t2i_pack_stem
 *   bias     [C0] of dtype, or NULL
 *   out      [B h w][C0] of dtype, row stride ld_out
 * dtype = MI355X_BF16: the picture is rounded to bfloat16, products accumulate in float32 on v_mfma_f32_16x16x32_bf16.
 * dtype = MI355X_F32:  v_mfma_f32_16x16x4_f32, as mi355x_gemm's float32 mode.  One rounding on store.
 * Alignment: picture, weight and out on 16 bytes; ld_out * sizeof(dtype) a multiple of 16.
 * ESHAPE: r not 8 or 16; cin not 1 or 3; B, h or w < 1; C0 < 16 or C0 % 16 != 0; ld_out < C0; an alignment rule broken; out overlapping the picture
 *         or the weight; more than 2^31 - 1 workgroups.   EDTYPE: dtype or pic_dtype not F32 / BF16.   EARG: args, picture, weight or out NULL.
 *
 * mi355x_t2i_pool: AvgPool2d(2, 2) on channels-last rows; an odd H or W is floored (the last row / column is not read).
 *   out[(b (H / 2) + y) (W / 2) + x][c] = (x00 + x01 + x10 + x11) / 4, summed in float32 in that order, xij = in[(b H + 2 y + i) W + 2 x + j][c]
 *   in [B H W][C] row stride ld_in; out [B (H / 2) (W / 2)][C] row stride ld_out; both 16-byte aligned with row strides multiples of 16 bytes.
 * ESHAPE: B < 1, H < 2, W < 2, C < 1, C * sizeof(dtype) % 16 != 0; a stride below C; an alignment rule broken; in and out overlapping.
 */
#ifndef MI355X_REFINERS_T2I_H
#define MI355X_REFINERS_T2I_H

#include <stdint.h>
#include "mi355x_refiners.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t dtype;
    int32_t pic_dtype;
    int32_t B, cin, r;
    int32_t h, w;
    int32_t C0;
} mi355x_t2i_stem_args;

typedef struct {
    int32_t dtype;
    int32_t B, H, W;
    int32_t C;
} mi355x_t2i_pool_args;

int mi355x_t2i_stem(const mi355x_t2i_stem_args* args, const void* picture, const void* weight, const void* bias, void* out, int64_t ld_out,
                    void* stream);

int mi355x_t2i_pool(const mi355x_t2i_pool_args* args, const void* in, int64_t ld_in, void* out, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_T2I_H */
