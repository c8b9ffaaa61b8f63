/*
 * mi355x_refiners_dinov2.h -- the streaming entry points of the DINOv2 encoder in libmi355x_refiners.so
 * (refiners_amd/csrc/dinov2.hip; reference foundationals/dinov2/{vit,dinov2}.py).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1) storage with float32 arithmetic, return value 0 or one of that
 * header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its
 * output untouched.  It is a header of its own because mi355x_refiners.h is a frozen list; refiners_amd.native reads every header the
 * same way.  No call allocates, synchronises with the host, keeps a pointer past its return or uses atomics: every output element
 * is written by exactly one lane, replays are bit-equal.
 *
 * Token rows are channels-last, [rows][D] at a row stride; pointers of `dtype` rows are 16-byte aligned and D * sizeof(element) and
 * every such row stride are multiples of 16 bytes.  float32 tables (tap weights, the resampled positions) are 4-byte aligned
 * unless said otherwise.
 */
#ifndef MI355X_REFINERS_DINOV2_H
#define MI355X_REFINERS_DINOV2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mi355x_dinov2_pos_resample -- InterpolateEmbedding as a separable filter over the patch part of the position table:
 *   out[(i * w + j) * ldo + c] = sum_a sum_b wy[wy_off[i] + a] * wx[wx_off[j] + b] * src[((y0[i] + a) * Ws + x0[j] + b) * lds + c]
 *   for i < h, j < w, a < ny[i], b < nx[j], c < D.  src: [Hs * Ws][D] of `dtype` (row (y, x) of the learned grid); out: [h * w][D] FLOAT32
 *   whatever dtype says (ldo in floats, 16-byte aligned rows).  Per output index of an axis the host gives the first source index
 *   (y0 / x0), the tap count (ny / nx, any count >= 1: antialiased downsampling to one cell spans the whole axis) and the offset of its
 *   first weight in the axis' float32 weight list (wy_off / wx_off); wy_len / wx_len are the lengths of those lists.  The kernel reads
 *   the tables from device memory and never leaves them: the entry point cannot see their contents, so the CALLER guarantees
 *   0 <= y0[i], y0[i] + ny[i] <= Hs, wy_off[i] + ny[i] <= wy_len (the same along x); refiners_amd.native checks it on the host copy.
 *   Sums run in float32, taps in ascending (a, b) order.  Bicubic, antialiased bicubic and bilinear differ in the tables alone.
 * ESHAPE: h, w, Hs, Ws < 1, wy_len / wx_len < 1, lds or ldo < D, misalignment.  EARG: NULL pointer, D < 1, out overlapping src. */
typedef struct mi355x_dinov2_pos_resample_args {
    int32_t dtype;
    int32_t Hs, Ws, h, w, D;
    const void* src;
    int64_t lds;
    const int32_t* y0;
    const int32_t* ny;
    const int32_t* wy_off;
    const float* wy;
    int32_t wy_len;
    const int32_t* x0;
    const int32_t* nx;
    const int32_t* wx_off;
    const float* wx;
    int32_t wx_len;
    float* out;
    int64_t ldo;
} mi355x_dinov2_pos_resample_args;
int mi355x_dinov2_pos_resample(const mi355x_dinov2_pos_resample_args* a, void* stream);

/* mi355x_dinov2_tokens -- the token matrix of B images from the patch GEMM's output, one launch: image b owns `rows` >= T = 1 + R + n
 * consecutive rows of out, starting at row b * rows.
 *   row 0            cls[:] + pos0[:]            (class token + position 0)
 *   rows 1 .. R      reg[r - 1][:]               (register tokens: the reference splices them in AFTER the position add)
 *   row 1 + R + i    patch[b * n + i][:] + pos[i][:]   (pos: the FLOAT32 [n][D] output of mi355x_dinov2_pos_resample)
 *   rows T .. rows-1 zeros                       (padding up to the attention kernel's 64-key blocks stays finite in every replay)
 *   cls [D], pos0 [D], reg [R][D] (row stride ldr; NULL when R == 0) and patch [B * n][D] are `dtype`; every sum is taken in float32 and
 *   rounded once.  Nothing outside the B * rows rows is written.
 * ESHAPE: B, n < 1, R < 0, rows < 1 + R + n, a row stride < D, misalignment.  EARG: NULL pointer (reg with R > 0), D < 1, out
 *         overlapping patch. */
typedef struct mi355x_dinov2_tokens_args {
    int32_t dtype;
    int32_t B, n, R, D, rows;
    const void* patch;
    int64_t ldp;
    const float* pos;
    int64_t ldpos;
    const void* cls;
    const void* pos0;
    const void* reg;
    int64_t ldr;
    void* out;
    int64_t ldo;
} mi355x_dinov2_tokens_args;
int mi355x_dinov2_tokens(const mi355x_dinov2_tokens_args* a, void* stream);

/* mi355x_glu_silu -- GLU(SiLU()): out[m][j] = x[m][j] * silu(x[m][F + j]), silu(g) = g / (1 + exp(-g)), over x [M][2 F] -> out [M][F]
 * (the reference's `output, gate = chunk(2)`).  exp(-g) overflows to +inf for g < -88 and the quotient is then -0: finite for every
 * finite gate.  ESHAPE: M < 1, ldx < 2 F, ldo < F, misalignment (F * sizeof(element) a multiple of 16 bytes).
 * EARG: NULL pointer, F < 1, out overlapping x. */
int mi355x_glu_silu(int32_t dtype, const void* x, int64_t ldx, void* out, int64_t ldo, int32_t M, int32_t F, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_DINOV2_H */
