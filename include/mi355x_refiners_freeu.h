/*
 * mi355x_refiners_freeu.h -- FreeU's residual concatenator in one launch: the Fourier filter of the skip features as a low-rank update, and the
 * scaled first half of the backbone features (refiners_amd/csrc/freeu.hip; reference latent_diffusion/freeu.py, fourier_filter +
 * FreeUBackboneFeatures + FreeUSkipFeatures).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1) storage with float32 arithmetic, return value 0 or one of that
 * header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its
 * outputs untouched.  The call does not allocate, synchronise with the host, keep a pointer past its return or use atomics: every output
 * element is written by exactly one lane and every sum has a fixed order, replays are bit-equal.
 *
 * mi355x_freeu_filter, on token rows (row b * HW + p = pixel p of image b, channels contiguous):
 *   skip_out[b][p][c] = skip[b][p][c] + sum over r < 16 of synthesis[r][p] * (sum over p' < HW of analysis[r][p'] * skip[b][p'][c])
 *   backbone[b][p][c] *= backbone_scale   for c < C_b / 2, in place; columns C_b / 2 .. C_b - 1 are neither read nor written
 * `analysis` and `synthesis` are float32 tables of 16 rows with row stride ld_table; rows at or beyond R and columns at or beyond HW hold
 * zeros (the kernel reads whole 128-column blocks of them).  With bfloat16 storage the analysis table enters the matrix pipe as a sum of two
 * bfloat16 parts, so it keeps float32-level accuracy; sums and the update are float32, one rounding on store.
 *   skip      [B * HW][C_skip], row stride ld_skip; rows at or beyond B * HW are not read
 *   skip_out  [B * HW][C_skip], row stride ld_out; the same buffer as `skip` (same pointer and stride) or one that shares no byte with it
 *   backbone  [B * HW][C_b], row stride ld_backbone; shares no byte with skip or skip_out
 * Alignment: skip, skip_out, backbone, analysis and synthesis on 16 bytes, the three row strides multiples of 16 bytes.
 * ESHAPE: B, HW, C_skip or R < 1; R > 16; C_skip % 8 != 0; C_b < 2, C_b odd or (C_b / 2) % 8 != 0; a row stride below its channel count;
 *         ld_table % 128 != 0 or ld_table < HW; an alignment or overlap rule broken; backbone_scale not finite; more than 2^31 - 1 workgroups.
 * EARG:   args or a pointer NULL.
 */
#ifndef MI355X_REFINERS_FREEU_H
#define MI355X_REFINERS_FREEU_H

#include <stdint.h>
#include "mi355x_refiners.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t dtype;
    int32_t B, HW;
    int32_t C_skip, C_b;
    int32_t R;
    float backbone_scale;
} mi355x_freeu_args;

int mi355x_freeu_filter(const mi355x_freeu_args* args, const void* skip, int64_t ld_skip, void* skip_out, int64_t ld_out, void* backbone,
                        int64_t ld_backbone, const float* analysis, const float* synthesis, int64_t ld_table, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_FREEU_H */
