/*
 * mi355x_refiners_attn_streams.h -- short-key attention over one or two K/V streams at the general head widths, in one launch
 * (refiners_amd/csrc/attn_streams.hip; the IP-Adapter cross-attention of SD1.5: reference latent_diffusion/image_prompt.py,
 * stable_diffusion_1/image_prompt.py).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1) storage with float32 arithmetic, return value 0 or one of that
 * header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its
 * output untouched.  It is a header of its own because mi355x_refiners.h is a frozen list; it takes that header's mi355x_attn_args
 * (and the mi355x_kv_stream inside it) unchanged.  The call does not allocate, synchronise with the host, keep a pointer past its
 * return or use atomics: every output element is written by exactly one lane, replays are bit-equal.
 *
 * mi355x_attention_streams:
 *   out = sum_s out_scale_s * softmax(scale * Q K_s^T) V_s ,   s < nstream, nstream in {1, 2}
 * what mi355x_attention computes at D = 64, for the head widths of mi355x_attention_general with Dqk == Dv, where all streams together
 * have at most three 64-key tiles: sum_s ceil(Lk_s / 64) <= 3.  Each stream has an exact softmax of its own (its true maximum over its Lk_s
 * keys, base-2 exponentials, its row sum); a stream whose out_scale is exactly 0 contributes an exact zero and is not read.
 *   Layouts as for mi355x_attention_general: Q [B][Lq][H * D], K_s [B][Lk_s][H * D] and out [B][Lq][H * D] token-major with a row stride
 *   and a batch stride each (Q and K may be column slices of a wider buffer); V_s^T at vt + (h * D + d) * ldvt + b * vt_batch_stride + key,
 *   every row readable and finite up to the next multiple of 64 keys OF ITS STREAM.  K rows at or beyond Lk_s are not read; V^T columns at
 *   or beyond Lk_s meet a zero probability.
 * D * sizeof(element) % 16 == 0, D % 4 == 0, D <= 160.
 * Alignment: q, k, vt on 16 bytes and their row and batch strides multiples of 16 bytes; out, ldo and o_batch_stride multiples of 4
 * ELEMENTS (a lane stores 4 elements at once).
 * ESHAPE: B, H, Lq, D < 1; nstream not 1 or 2; an Lk_s < 1; more than three key tiles over all streams; D > 160 or a D that misses the
 *         rules above; an alignment rule broken; a (batch, head) slice of K or V^T that spans 2 GB or more.
 * EARG:   args, q, out, or a stream's k / vt NULL.
 */
#ifndef MI355X_REFINERS_ATTN_STREAMS_H
#define MI355X_REFINERS_ATTN_STREAMS_H

#include <stdint.h>
#include "mi355x_refiners.h"

#ifdef __cplusplus
extern "C" {
#endif

int mi355x_attention_streams(const mi355x_attn_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_ATTN_STREAMS_H */
