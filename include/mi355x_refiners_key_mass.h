/*
 * mi355x_refiners_key_mass.h -- the attention mass every key receives, without the attention matrix
 * (refiners_amd/csrc/attn_key_mass.hip; the Self-Attention Guidance tap: reference latent_diffusion/self_attention_guidance.py,
 * SelfAttentionMap + compute_sag_mask).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1) storage with float32 arithmetic, return value 0 or one of that
 * header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its
 * outputs untouched.  It is a header of its own because mi355x_refiners.h is a frozen list.  The call does not allocate, synchronise
 * with the host, keep a pointer past its return or use atomics: every output element is written by exactly one lane, replays are
 * bit-equal.
 *
 * mi355x_attention_key_mass:
 *   mass[b][j] = 1 / H * sum over heads h and queries i of softmax_j(scale * q[b][i][h] . k[b][j][h]),   j < L
 * i.e. softmax(scale Q K^T) averaged over the heads and summed down every column; each row of `mass` sums to L.  Two dependent launches on
 * `stream`: the first writes the base-2 log-sum-exp of every score row, lse[b][h][i] = max_j(c s_ij) + log2(sum_j 2^(c s_ij - max)) with
 * c = scale * log2(e), to `lse`; the second forms 2^(c s_ij - lse[b][h][i]) again and sums it per key.  The L x L scores exist in registers only.
 *   q, k   [B][L][H * D] token-major, head h at columns h * D .. h * D + D - 1, each with a row stride (ldq, ldk) and a batch stride; both may
 *          be column slices of one wider buffer.  Rows at or beyond L are not read.
 *   lse    float32 scratch, row (b, h) at lse + (b * H + h) * ldl, ldl >= L; columns 0 .. L-1 are written.
 *   mass   float32 output, row b at mass + b * ldm, ldm >= L; columns 0 .. L-1 are written, ALL of them and nothing else: the row needs no
 *          zeroing before the call and there is no accumulate flag.
 * D * sizeof(element) % 16 == 0 and D <= 160 (40, 64, 80, 96, 128, 160 ...); any L >= 1.
 * Alignment: q and k on 16 bytes, their row and batch strides multiples of 16 bytes; lse and mass on 4 bytes.
 * ESHAPE: B, H, L or D < 1; D > 160 or D * sizeof(element) % 16 != 0; ldl < L or ldm < L; scale not a positive finite number; an alignment rule
 *         broken; a negative row stride; a (batch, head) slice of q or k that spans 2 GB or more ((L - 1) * ld + D elements); more than 2^31 - 1
 *         workgroups in either launch.
 * EARG:   args, q, k, lse or mass NULL.
 */
#ifndef MI355X_REFINERS_KEY_MASS_H
#define MI355X_REFINERS_KEY_MASS_H

#include <stdint.h>
#include "mi355x_refiners.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t dtype;
    int32_t B, H, L, D;
    float scale;
} mi355x_key_mass_args;

int mi355x_attention_key_mass(const mi355x_key_mass_args* args, const void* q, int64_t ldq, int64_t q_batch_stride, const void* k, int64_t ldk,
                              int64_t k_batch_stride, float* lse, int64_t ldl, float* mass, int64_t ldm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_KEY_MASS_H */
