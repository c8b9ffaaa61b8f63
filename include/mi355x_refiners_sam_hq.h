/*
 * mi355x_refiners_sam_hq.h -- the HQ-SAM mask-prediction entry points of libmi355x_refiners.so (refiners_amd/csrc/sam_hq.hip).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1), return value 0 or one of that header's negative MI355X_E*
 * codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its outputs untouched.  It is a
 * header of its own because mi355x_refiners.h is a frozen list (ABI version 7: its 39 prototypes and 24 structs are pinned);
 * refiners_amd.native reads both headers the same way.  Arithmetic is float32 whatever the storage type, there are no atomics, and
 * every output element is written by exactly one lane: replays are bit-equal.
 *
 * They replace the decoder side of segment_anything/hq_sam.py:16-167 (CompressViTFeat, EmbeddingMaskfeature, HQSAMMaskPrediction).
 */
#ifndef MI355X_REFINERS_SAM_HQ_H
#define MI355X_REFINERS_SAM_HQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mi355x_sam_hq_mask_head -- the HQ mask of P prompts of H x W pixels (H, W even) in one launch, with the second 3x3 convolution of
 * EmbeddingMaskfeature folded into the HQ token's vector.  With z = GELU(LayerNorm2d(y)) (exact-erf GELU; float32 statistics over the
 * 64 channels of a pixel; gamma / beta float32 [64]) the reference computes  sum_c h[p][c] (conv2(z)[c] + F[c]),  conv2 = Conv2d(64 ->
 * 32, 3, padding 1).  Everything after z is linear, so
 *     out[p][y][x] = sum_{tap, ci} weff[p][tap][ci] z[p][y + dy][x + dx][ci] + sum_c h[p][c] (F[y][x][c] + b2[c]),
 *     weff[p][tap][ci] = sum_c h[p][c] w2[c][tap][ci],   tap = 3 (dy + 1) + (dx + 1),   z = 0 outside the image (zero padding applies to
 *     z, i.e. AFTER the activation: a halo pixel outside the image is 0, not GELU(LayerNorm2d(0)))
 * and the [P][32][H][W] tensor is never formed.
 *   y    [P H W][ldy] rows (ldy >= 64, a multiple of 4 elements; 16-byte aligned for float32, 8-byte for bfloat16), row (p H + yy) W + xx
 *   w2   float32 [32][9][64] = weight[c][ci][ky][kx] as [c][3 ky + kx][ci], 16-byte aligned;  b2 float32 [32]
 *   h    dtype, 32 values per prompt at h + p * h_stride
 *   fq   dtype, the shared HQ features in QUADRANT layout (the output of the GEMM of a 2x2 / 2 transposed convolution, unscattered):
 *        pixel (yy, xx) is row (yy >> 1) (W / 2) + (xx >> 1), columns ((yy & 1) 2 + (xx & 1)) 32 + c, leading dimension ldf >= 128 (a
 *        multiple of 4 elements, aligned like y); the same for every prompt
 *   out  dtype [H][W] per prompt at out + p * out_batch_stride
 * One workgroup = 16 x 8 pixel tiles of one prompt: weff and h . b2 folded into LDS once, then per tile the 18 x 10 halo of z staged
 * into LDS (LayerNorm2d + GELU on the way in) and 9 x 64 FMAs per pixel from LDS.
 * ESHAPE: odd H or W, ldy < 64, ldf < 128, a misaligned y / fq / w2 or leading dimension.  EARG: a NULL pointer, P / H / W <= 0. */
typedef struct mi355x_sam_hq_mask_head_args {
    int32_t dtype;
    int32_t P, H, W;
    const void* y;
    int64_t ldy;
    const float* gamma;
    const float* beta;
    float eps;
    const float* w2;
    const float* b2;
    const void* h;
    int64_t h_stride;
    const void* fq;
    int64_t ldf;
    void* out;
    int64_t out_batch_stride;
} mi355x_sam_hq_mask_head_args;
int mi355x_sam_hq_mask_head(const mi355x_sam_hq_mask_head_args* a, void* stream);

/* mi355x_sam_mask_head_up -- mi355x_sam_mask_head (same fields, same kernel body, masks bit-equal on the same inputs) that ALSO stores
 * the upscaled dense embedding it contracts: the 32 GELU'd channels of output pixel (p, yy, xx) go to u[((p 2 Hin + yy) 2 Win + xx) ldu
 * + c] in dtype (one rounding of the float32 value; ldu >= 32, u 16-byte aligned and ldu a multiple of 16 bytes; columns >= 32 of a
 * wider row are not written).  EmbeddingMaskfeature (hq_sam.py:92-106) reads it as context "upscaled_dense_embedding".
 * ESHAPE adds: ldu < 32 or a misaligned u / ldu.  EARG adds: u NULL. */
typedef struct mi355x_sam_mask_head_up_args {
    int32_t dtype;
    int32_t P, Hin, Win, nk;
    const void* x;
    int64_t ldx;
    const float* w;
    const float* bias;
    const void* hyper;
    int64_t ld_hyper, hyper_batch_stride;
    void* out;
    int64_t out_batch_stride;
    void* u;
    int64_t ldu;
} mi355x_sam_mask_head_up_args;
int mi355x_sam_mask_head_up(const mi355x_sam_mask_head_up_args* a, void* stream);

/* mi355x_ln2d_gelu_wide -- the Hs > 0 form of mi355x_convt2x2_ln_gelu for C = 128 or 256 channels (CompressViTFeat's LayerNorm2d +
 * GELU after ConvTranspose2d(1280 -> 256, 2, 2), hq_sam.py:16-45): x [M][ldx] = the GEMM output with 4 groups of C columns per row
 * (group g = (dy, dx) = (g / 2, g % 2)), rows = pixels (p, y, x) of images of Hs x Ws; group g of row m is normalised over its C
 * channels (float32 statistics; gamma / beta float32 [C]), GELU'd and written to pixel (p, 2y + dy, 2x + dx) of the NHWC output
 * [P][2 Hs][2 Ws][ldo].  One wave per group, each lane owns C / 64 consecutive channels, the reductions stay inside the wave.
 * ESHAPE: another C, Hs or Ws <= 0, M not a multiple of Hs Ws, ldx < 4 C, ldo < C.  EARG: a NULL pointer, M <= 0. */
int mi355x_ln2d_gelu_wide(int32_t dtype, const void* x, int64_t ldx, int64_t M, int32_t C, const float* gamma, const float* beta, float eps,
                          void* out, int64_t ldo, int32_t Hs, int32_t Ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_SAM_HQ_H */
