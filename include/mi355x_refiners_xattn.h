/*
 * mi355x_refiners_xattn.h -- a cross-attention folded into its Q projection (refiners_amd/csrc/gemm_xattn.hip).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, `stream` a hipStream_t passed as void*,
 * return value 0 or one of that header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches
 * nothing.  It is a header of its own because mi355x_refiners.h is a frozen list (ABI version 7: its 39 prototypes and 24 structs are
 * pinned); it takes two of that header's structs unchanged.
 *
 * mi355x_gemm_attention(gemm, attn) computes what mi355x_gemm(gemm) followed by mi355x_attention(attn) computes when gemm->out is the
 * attention's q -- Q = epi(x W^T) rounded to bfloat16, out = sum_s out_scale_s softmax(scale Q K_s^T) V_s -- in ONE launch: the workgroup
 * that finishes a 64 x 64 tile of Q (64 queries of one batch element x the 64 columns of one head) attends with it against the K / V^T
 * tiles of that (batch element, head) and stores the attention output.  Q is never written: gemm->out, gemm->ldo and attn->q, attn->ldq,
 * attn->q_batch_stride are not read and may be NULL / 0.  Arithmetic, rounding points and the treatment of keys beyond Lk are those of the
 * two launches (the bfloat16 LDS-DMA form of the short-K/V kernel with 16 queries per wave); there are no atomics, every output element
 * is written by exactly one lane.
 *
 * Honoured from mi355x_gemm_args: M, N, seg[0] (either operand K-blocked or not), bias, the folded LayerNorm (ln_stats, ln_parts, ln_eps,
 * ln_s, ln_c), the in-launch LoRA (lora_a[0], lora_b, lora_r, lora_ls, lora_lc, lora_t, lora_flags, lora_epoch), prefetch / prefetch_bytes /
 * prefetch_blocks and tile.  From mi355x_attn_args: everything but the q fields.
 *
 * Refusals (every check of mi355x_gemm / mi355x_attention for the fields above applies as well, with its code):
 *   EARG    gemm, attn or attn->out NULL
 *   EDTYPE  gemm->dtype or attn->dtype is not MI355X_BF16
 *   ESHAPE  attn->D != 64;  gemm->N != attn->H * 64;  gemm->M != attn->B * attn->Lq;  attn->Lq % 64 != 0 (a row tile must not straddle
 *           two batch elements);  nstream not 1 or 2, an Lk < 1, more than three 64-key tiles over all streams, or three tiles of which
 *           the second or third holds more than 32 keys (with three tiles the Q image shares the drained stage buffers with the last
 *           two: Lk0 in 65 .. 96 and Lk1 <= 32, e.g. 77 text + 4 image-prompt keys);  not a plain GEMM: nseg != 1, conv, geglu != 0, res,
 *           rowbias, out_t, out_f32, ksplit > 1, stats_out, colstats_out, out_kblocked;  LoRA other than one column group of stacked rank
 *           32;  tile other than 0 or 4 (the 64 x 64 tile of the 4-wave loop is the only one with this form);  an operand of 2 GB or more
 *           (x, w, a K / V^T batch-head slice's extent, the output).
 */
#ifndef MI355X_REFINERS_XATTN_H
#define MI355X_REFINERS_XATTN_H

#include <stdint.h>
#include "mi355x_refiners.h"

#ifdef __cplusplus
extern "C" {
#endif

int mi355x_gemm_attention(const mi355x_gemm_args* gemm, const mi355x_attn_args* attn, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_XATTN_H */
