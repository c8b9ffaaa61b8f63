/*
 * mi355x_refiners_mvanet.h -- the streaming entry points of MVANet's multi-view decoder in libmi355x_refiners.so
 * (refiners_amd/csrc/mvanet.hip; reference foundationals/swin/mvanet/{mvanet,mclm,mcrm,utils}.py).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1) storage with float32 arithmetic, return value 0 or one of that
 * header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its
 * output untouched.  It is a header of its own because mi355x_refiners.h is a frozen list; refiners_amd.native reads every header the
 * same way.  No call allocates, synchronises with the host, keeps a pointer past its return or uses atomics: every output element
 * is written by exactly one lane, replays are bit-equal.
 *
 * Activations are channels-last token rows: a view of side S is [S * S][E] with row stride ld, token y * S + x.  "Four views" are the
 * four local views one after the other, [4 * S * S][E]; read as the QUADRANTS of one merged 2S x 2S map (the reference's PatchMerge),
 * pixel (Y, X) of that map is token (Y % S) * S + X % S of view 2 * (Y / S) + X / S.  PatchSplit is the inverse: quadrant
 * q = 2 * qy + qx of an S x S map is the (S / 2) x (S / 2) block at (qy * S / 2, qx * S / 2).
 * Pointers are 16-byte aligned and E * sizeof(element) and every row stride are multiples of 16 bytes unless said otherwise.
 */
#ifndef MI355X_REFINERS_MVANET_H
#define MI355X_REFINERS_MVANET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355X_MVANET_MAX_RATIOS 3

/* mi355x_mvanet_pool -- MultiPool: average pools of a map at up to three ratios, written as token rows one ratio after the other.
 *   mode 0   src = four views of side S; the map is their PatchMerge, side G = 2 S; ONE output group.
 *   mode 1   src = one view of side S; FOUR output groups, group q pools quadrant q (PatchSplit), side G = S / 2.
 *   out      group g at out + g * group_stride, `rows` rows each: row base_i + py * (G / r_i) + px holds the mean of the r_i x r_i block
 *            at (py r_i, px r_i), base_i = sum over j < i of (G / r_j)^2 (ratio 1 is a copy).  Rows from sum_i (G / r_i)^2 up to
 *            `rows` are written as ZEROS: the attention kernel reads V^T up to the next multiple of 64 keys and needs it finite.
 *   The mean is the float32 sum in row-major order of the block times 1 / r^2.
 * ESHAPE: S < 1 (mode 1: S odd), n_ratios outside 1..3, a ratio < 1 or not dividing G, rows < the pooled row count, group_stride <
 *         rows * ldo in mode 1, lds or ldo < E, misalignment.  EARG: NULL pointer, E < 1, mode not 0 / 1, out overlapping src. */
typedef struct mi355x_mvanet_pool_args {
    int32_t dtype;
    int32_t mode, S, E;
    int32_t n_ratios;
    int32_t ratio[MI355X_MVANET_MAX_RATIOS];
    const void* src;
    int64_t lds;
    void* out;
    int64_t ldo;
    int32_t rows;
    int64_t group_stride;
} mi355x_mvanet_pool_args;
int mi355x_mvanet_pool(const mi355x_mvanet_pool_args* a, void* stream);

/* mi355x_mvanet_gate -- MCRM's gate: out[v][y][x][:] = local[v][y][x][:] * sigmoid(w . glb[(qy S + y) / 2][(qx S + x) / 2][:] + b[0]),
 * v = 2 qy + qx: the 1 x 1 convolution to one channel, the sigmoid, the nearest 2x upsampling and the PatchSplit as index arithmetic
 * (no [2S][2S] map is stored).  local / out: four views of side S (out may BE local, same pointer and stride); glb: one view of side S;
 * w [E] and b [1]: dtype, read from device memory at every launch.  One wave per global pixel: the dot product is a float32 wave
 * reduction in a fixed order, then the wave scales that pixel's four local tokens.
 * ESHAPE: S < 1, a row stride < E, misalignment (rows: 16 bytes; w, b: element).  EARG: NULL pointer, E < 1, out overlapping glb, or
 *         overlapping local without being it. */
typedef struct mi355x_mvanet_gate_args {
    int32_t dtype;
    int32_t S, E;
    const void* local;
    int64_t ldl;
    const void* glb;
    int64_t ldg;
    const void* w;
    const void* b;
    void* out;
    int64_t ldo;
} mi355x_mvanet_gate_args;
int mi355x_mvanet_gate(const mi355x_mvanet_gate_args* a, void* stream);

/* mi355x_mvanet_resize_add -- out = resize(f(a)) + g(b) over B maps, f / g = identity (slope NULL) or PReLU with ONE slope read
 * from device memory (slope_a / slope_b: one element of dtype; max(v, 0) + slope * min(v, 0)).
 *   a        B maps of Ha x Wa, [B * Ha * Wa][E]; a_merge = 1: four views of (Ha / 2) x (Wa / 2) read as their PatchMerge (B = 1).
 *   b, out   B maps of Ho x Wo; b_merge = 1: b is four views of (Ho / 2) x (Wo / 2) read as their PatchMerge (B = 1).  out is always a
 *            plain map and may BE b (same pointer and stride, b_merge = 0).
 *   mode 0   bilinear as torch's interpolate(mode="bilinear", align_corners=False, antialias=False), up or down: along each axis
 *            src = max((dst + 0.5) * in / out - 0.5, 0) (float32, in / out one float32 quotient), i0 = floor(src), i1 = min(i0 + 1,
 *            in - 1), l1 = src - i0, l0 = 1 - l1;  value = h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11).  f is applied to the four
 *            samples, before the weights.
 *   mode 1   nearest as torch's interpolate(mode="nearest"): src = floor(dst * in / out) in exact integer arithmetic (equal to
 *            torch's float32 rule for every integer ratio up or down), clamped to in - 1.
 *   Ha == Ho and Wa == Wo is a plain (activated) sum in either mode.
 * ESHAPE: a size < 1, a merged operand with B != 1 or an odd side, a row stride < E, misalignment.  EARG: NULL a / b / out, E < 1,
 *         mode not 0 / 1, out overlapping a, or overlapping b without being it. */
typedef struct mi355x_mvanet_resize_add_args {
    int32_t dtype;
    int32_t mode, B, E;
    int32_t Ha, Wa, Ho, Wo;
    int32_t a_merge, b_merge;
    const void* a;
    int64_t lda;
    const void* b;
    int64_t ldb;
    const void* slope_a;
    const void* slope_b;
    void* out;
    int64_t ldo;
} mi355x_mvanet_resize_add_args;
int mi355x_mvanet_resize_add(const mi355x_mvanet_resize_add_args* a, void* stream);

/* mi355x_mvanet_prelu -- x[i] = max(x[i], 0) + slope[0] * min(x[i], 0) in place over n contiguous elements; slope: one element of
 * dtype in device memory.  ESHAPE: n no multiple of 16 bytes, x misaligned.  EARG: NULL pointer, n < 1. */
int mi355x_mvanet_prelu(int32_t dtype, void* x, const void* slope, int64_t n, void* stream);

/* mi355x_mvanet_split_views -- SplitMultiView: img [C][H][W] (NCHW, one image) -> out [5][C][H / 2][W / 2]: views 0..3 are the
 * quadrants 2 qy + qx, view 4 is bilinear 0.5x (align_corners=False), i.e. 0.5 (0.5 p00 + 0.5 p01) + 0.5 (0.5 p10 + 0.5 p11) of every
 * 2 x 2 block.  Pointers element-aligned.  ESHAPE: C, H or W < 1, H or W odd.  EARG: NULL pointer, out overlapping img. */
int mi355x_mvanet_split_views(int32_t dtype, const void* img, void* out, int32_t C, int32_t H, int32_t W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_MVANET_H */
