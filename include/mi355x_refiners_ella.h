/*
 * mi355x_refiners_ella.h -- the streaming entry point of the ELLA timestep-aware text connector in libmi355x_refiners.so
 * (refiners_amd/csrc/ella.hip; reference foundationals/latent_diffusion/ella_adapter.py).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1) storage with float32 arithmetic, return value 0 or one of that
 * header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its
 * output untouched.  It is a header of its own because mi355x_refiners.h is a frozen list; refiners_amd.native reads every header the
 * same way.  The call does not allocate, synchronise with the host, keep a pointer past its return or use atomics: every output
 * element is written by exactly one lane, replays are bit-equal.
 *
 * The resampler's other launches are the library's GEMM (mi355x_gemm, whose epilogue code 5 is ELLA's squared ReLU), attention
 * (mi355x_attention_general at head dim 96) and LayerNorm entry points.
 */
#ifndef MI355X_REFINERS_ELLA_H
#define MI355X_REFINERS_ELLA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mi355x_ella_adaln -- PerceiverAttention's Distribute(AdaLayerNorm, AdaLayerNorm) and its to_kv = cat(latents_n, x_n), or the
 * feed-forward AdaLayerNorm (T == 0), in one launch.  Batch row b owns Lp consecutive rows of out, starting at out + b * out_batch_stride:
 *   rows r < Nl             LN0(latents[b][r]) * (1 + scale_l[b]) + shift_l[b]
 *   rows Nl <= r < Nl + T   LN0(x[b][r - Nl])  * (1 + scale_x[b]) + shift_x[b]
 *   rows Nl + T <= r < Lp   exactly 0 (the attention kernel reads key rows up to the next multiple of 64: they stay finite in every replay)
 * LN0 = LayerNorm without affine over the C columns of a row: biased variance, float32 statistics, two passes over the row held in
 * registers (mean, then the centred sum of squares), rstd = 1 / sqrt(var + eps).  The query source of the attention is the first Nl rows
 * of the same buffer: no second tensor and no concatenation exist.
 *   latents [B][Nl][C] (row stride ldl, batch stride l_batch_stride) and x [B][T][C] (ldx, x_batch_stride; ignored when T == 0) are `dtype`.
 *   shift_* / scale_* are rows [B][C] of `dtype` at batch stride mod_batch_stride: column slices of one time-embedding projection (the
 *   reference's chunk(2): shift first, scale second).  shift_x / scale_x are ignored when T == 0.
 * ESHAPE: B, Nl < 1, T < 0, Lp < Nl + T, C < 1, C > 4096, C * sizeof(element) or a stride * sizeof(element) no multiple of 16 bytes, a row
 *         stride < C, a batch stride that lets batch rows overlap, a misaligned pointer.
 * EARG:   NULL pointer, out overlapping latents or x. */
typedef struct mi355x_ella_adaln_args {
    int32_t dtype;
    int32_t B, Nl, T, Lp, C;
    const void* latents;
    int64_t ldl, l_batch_stride;
    const void* x;
    int64_t ldx, x_batch_stride;
    const void* shift_l;
    const void* scale_l;
    const void* shift_x;
    const void* scale_x;
    int64_t mod_batch_stride;
    float eps;
    void* out;
    int64_t ldo, out_batch_stride;
} mi355x_ella_adaln_args;
int mi355x_ella_adaln(const mi355x_ella_adaln_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_ELLA_H */
