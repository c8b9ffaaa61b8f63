/*
 * mi355x_refiners_lineart.h -- the InformativeDrawings (lineart preprocessor) entry points of libmi355x_refiners.so
 * (refiners_amd/csrc/lineart.hip).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1), return value 0 or one of that header's negative MI355X_E*
 * codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its outputs untouched.  It is a
 * header of its own because mi355x_refiners.h is a frozen list (ABI version 7: its 39 prototypes and 24 structs are pinned);
 * refiners_amd.native reads both headers the same way.  Arithmetic is float32 whatever the storage type, there are no atomics, every
 * output element is written by exactly one lane and every reduction runs in a fixed order: replays are bit-equal.
 *
 * They replace foundationals/latent_diffusion/preprocessors/informative_drawings.py:8-107 around the 3x3 convolutions, which run on
 * mi355x_gemm's implicit-GEMM path.  Between launches an activation is channels-last pixel rows [B H W][C] in one of three LAYOUTS,
 * named by (layout, pad) next to the pointer; (H, W) is always the LOGICAL image the normalisation sees:
 *   MI355X_LINEART_ROWS    pixel (b, y, x) is row (b H + y) W + x, channel c is column c.
 *   MI355X_LINEART_PADDED  the interior of rows of (H + 2 pad) x (W + 2 pad) images: pixel (b, y, x) is row
 *                          (b (H + 2 pad) + y + pad)(W + 2 pad) + x + pad.  What a zero-padded 3x3 convolution over a
 *                          reflect-padded image leaves: its interior is the valid convolution of the reflect-padded image.
 *   MI355X_LINEART_QUAD    H, W even; pixel (b, y, x) is row (b H/2 + (y >> 1)) W/2 + (x >> 1), channel c is column
 *                          ((y & 1) 2 + (x & 1)) C + c of 4 C.  What the 3x3 convolution form of ConvTranspose2d(3, stride 2,
 *                          padding 1, output_padding 1) leaves; nothing un-shuffles it but the index arithmetic of its readers.
 * Every activation pointer is aligned to 4 elements (16 bytes float32, 8 bytes bfloat16) and every leading dimension is a multiple
 * of 4 elements and at least the columns read or written (C; 4 C for QUAD).
 */
#ifndef MI355X_REFINERS_LINEART_H
#define MI355X_REFINERS_LINEART_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MI355X_LINEART_ROWS = 0, MI355X_LINEART_PADDED = 1, MI355X_LINEART_QUAD = 2 };
#define MI355X_LINEART_MAX_CIN 4

/* mi355x_lineart_stem -- ReflectionPad2d(3) + Conv2d(Cin -> 64, 7) in one launch, reading the NCHW image and writing ROWS.
 *   image  dtype [B][Cin][H][W]: element (b, ci, y, x) at b batch_stride + ci channel_stride + y row_stride + x (no alignment asked)
 *   w      float32 [Cin 49][64] = weight[co][ci][ky][kx] as row (ci 7 + ky) 7 + kx, column co; 16-byte aligned
 *   bias   float32 [64] or NULL (a bias in front of a non-affine InstanceNorm2d cancels; the lowering passes NULL)
 *   out    dtype [B H W][ldo] ROWS, 64 columns written
 * The reflection is index arithmetic on the load of a 22 x 22 halo tile; the weights sit in LDS; plain float32 FMAs.
 * ESHAPE: H or W < 4 (the reflection needs 3 < H, W), Cin > MI355X_LINEART_MAX_CIN, ldo < 64, a misaligned w / out / ldo.
 * EARG: a NULL image / w / out, B / H / W / Cin <= 0. */
typedef struct mi355x_lineart_stem_args {
    int32_t dtype;
    int32_t B, H, W, Cin;
    const void* image;
    int64_t batch_stride, channel_stride, row_stride;
    const float* w;
    const float* bias;
    void* out;
    int64_t ldo;
} mi355x_lineart_stem_args;
int mi355x_lineart_stem(const mi355x_lineart_stem_args* a, void* stream);

/* mi355x_lineart_in_stats -- the InstanceNorm2d statistics of x in any layout: stats float32 [B][C][2] = (mean, rstd) per image and
 * channel, rstd = 1 / sqrt(biased variance + eps).  C is 64, 128 or 256.  Two kernels behind one call: per-slab Welford partials
 * (mean, M2) of every column into ws, then per channel the partials (and, for QUAD, the four column groups) combined as
 * (count, mean, M2) in slab order -- never E[x^2] - E[x]^2, so a mean of 50 standard deviations costs nothing.
 *   ws  float32 scratch of at least mi355x_lineart_in_stats_ws_floats(B, H, W, C, layout) floats (ws_floats says how many there are)
 * ESHAPE: another C, pad < 0, pad != 0 outside PADDED, odd H or W for QUAD, ldx too small, misaligned x / ldx, ws_floats too small,
 * B > 65535.  EARG: a NULL pointer, B / H / W <= 0, an unknown layout. */
typedef struct mi355x_lineart_in_stats_args {
    int32_t dtype;
    int32_t B, H, W, C;
    int32_t layout, pad;
    const void* x;
    int64_t ldx;
    float eps;
    float* stats;
    float* ws;
    int64_t ws_floats;
} mi355x_lineart_in_stats_args;
int mi355x_lineart_in_stats(const mi355x_lineart_in_stats_args* a, void* stream);
int64_t mi355x_lineart_in_stats_ws_floats(int32_t B, int32_t H, int32_t W, int32_t C, int32_t layout);

/* mi355x_lineart_in_apply -- out = (x - mean) rstd [ReLU'd when relu != 0] [+ res], from the statistics table.
 *   x      any layout (C = 64, 128 or 256)
 *   res    NULL, or dtype rows of (H + 2 res_pad) x (W + 2 res_pad) images whose interior is added AFTER the optional ReLU (res_pad 0: ROWS)
 *   out    dtype rows of (H + 2 ring) x (W + 2 ring) images, leading dimension ldo, C columns written.  ring 0 is ROWS.  With ring > 0
 *          the ring is ReflectionPad2d(ring) of the interior: the lane that owns interior pixel (y, x) also writes its mirror images
 *          (y -> -y for 1 <= y <= ring, y -> 2 (H - 1) - y for H - 1 - ring <= y <= H - 2; the same along x), so every output pixel
 *          still has one writer.  out must not overlap x or res.
 * ESHAPE: another C, ring >= H or ring >= W (ReflectionPad2d refuses it), a negative pad / res_pad / ring, pad != 0 outside PADDED,
 * odd H or W for QUAD, a leading dimension too small, a misaligned pointer or leading dimension.
 * EARG: a NULL x / stats / out, B / H / W <= 0, an unknown layout. */
typedef struct mi355x_lineart_in_apply_args {
    int32_t dtype;
    int32_t B, H, W, C;
    int32_t layout, pad;
    const void* x;
    int64_t ldx;
    const float* stats;
    int32_t relu;
    int32_t res_pad;
    const void* res;
    int64_t ldr;
    int32_t ring;
    void* out;
    int64_t ldo;
} mi355x_lineart_in_apply_args;
int mi355x_lineart_in_apply(const mi355x_lineart_in_apply_args* a, void* stream);

/* mi355x_lineart_head -- InstanceNorm2d(64) + ReLU + ReflectionPad2d(3) + Conv2d(64 -> 1, 7) + bias + Sigmoid in one launch; the
 * normalised [B H W][64] tensor is never stored.
 *   x      any layout, 64 channels;  stats float32 [B][64][2] of x (mi355x_lineart_in_stats)
 *   w      float32 [49][64] = weight[0][ci][ky][kx] as row 7 ky + kx, column ci; 16-byte aligned
 *   out    dtype [H][W] per image at out + b out_batch_stride (NCHW with one channel)
 * One workgroup = 16 x 8 pixel tiles of one image: the 22 x 14 halo is staged into LDS normalised and ReLU'd on the way in (reflected
 * by index arithmetic), then 49 x 64 FMAs per pixel from LDS, four lanes per pair of horizontally adjacent pixels.
 * ESHAPE: H or W < 4, pad < 0, pad != 0 outside PADDED, odd H or W for QUAD, ldx too small, misaligned x / ldx / w, B > 65535.
 * EARG: a NULL pointer, B / H / W <= 0, an unknown layout. */
typedef struct mi355x_lineart_head_args {
    int32_t dtype;
    int32_t B, H, W;
    int32_t layout, pad;
    const void* x;
    int64_t ldx;
    const float* stats;
    const float* w;
    float bias;
    void* out;
    int64_t out_batch_stride;
} mi355x_lineart_head_args;
int mi355x_lineart_head(const mi355x_lineart_head_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_LINEART_H */
