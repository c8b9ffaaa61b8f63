/*
 * mi355x_refiners_swin.h -- the Swin Transformer entry point of libmi355x_refiners.so (refiners_amd/csrc/window_attention.hip).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1), return value 0 or one of that header's negative MI355X_E*
 * codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its output untouched.  It is a
 * header of its own because mi355x_refiners.h is a frozen list; refiners_amd.native reads every header the same way.  The call
 * allocates nothing, does not synchronise with the host, keeps no pointer past its return, and uses no atomics: every output
 * element is written by exactly one lane, replays are bit-equal.
 */
#ifndef MI355X_REFINERS_SWIN_H
#define MI355X_REFINERS_SWIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mi355x_window_attention -- (shifted-)window attention of the Swin Transformer (foundationals/swin/swin_transformer.py, WindowSDPA
 * with its RelativePositionBias and get_attn_mask).  For every window w < nW and head h < H, with N = ws * ws tokens per window:
 *     out[w, :, h] = softmax(scale * Q K^T + table[rel(i, j)][h] + shiftmask_w(i, j)) V
 *   q, k, v   dtype; token i of window w, head h, channel c at  p + w * p_win_stride + i * ldp + h * 32 + c  (head dim is exactly 32).
 *             They are normally three column views of one packed QKV GEMM output [nW N][3 H 32] (columns ordered (3, H, 32)).
 *             Pointers 16-byte aligned, leading dimensions a multiple of 16 bytes and >= H * 32.
 *   table     float32 [(2 ws - 1)^2][H], the relative_position_bias_table parameter as stored in the tree.  The pair (query i, key j)
 *             with in-window coordinates (y, x) reads row (y_i - y_j + ws - 1) (2 ws - 1) + (x_i - x_j + ws - 1): the canonical
 *             relative_position_index, as arithmetic.  The table is staged in LDS; no N x N bias is ever stored.
 *   shift     0: no mask.  > 0 (the block's shift_size, < ws): the windows are those of a grid of nw x nw windows rolled by -shift,
 *             window w sits at ((w / nw) % nw, w % nw), and a position p of the grid has region id 0 for p < nw ws - ws, 1 for
 *             p < nw ws - shift, else 2, along each axis.  Pairs whose (row id, column id) differ get -100 ADDED (not -inf).
 *   out       dtype; token i of window w at out + w * o_win_stride + i * ldo + h * 32 + c: [nW N][H 32] row-major when
 *             o_win_stride = N ldo, ready for the output projection.  out 16-byte aligned (8-byte for bfloat16), ldo likewise.
 * Only rows i < N of a window are read and written; keys >= N of the kernel's 16-key blocks contribute exactly nothing.
 * float32 runs on v_mfma_f32_16x16x4_f32 (exact float32 products), bfloat16 on v_mfma_f32_16x16x32_bf16 with float32 softmax; the
 * whole score row of a query lives in registers, so the softmax is two-pass with the true row maximum.
 * One workgroup = one window and 4 (bfloat16) or 2 (float32) heads, one wave per head: V^T of the head in LDS, K in registers.
 * ESHAPE: ws < 1 or ws * ws > 144, shift < 0 or >= ws, shift > 0 with nw < 1 or nW no multiple of nw * nw, a leading dimension
 *         < H * 32, a misaligned pointer or leading dimension, more than 65535 head groups.  EARG: a NULL pointer, nW or H <= 0. */
typedef struct mi355x_window_attention_args {
    int32_t dtype;
    int32_t nW, H, ws, nw, shift;
    const void* q;
    const void* k;
    const void* v;
    int64_t ldq, ldk, ldv;
    int64_t q_win_stride, k_win_stride, v_win_stride;
    const float* table;
    float scale;
    void* out;
    int64_t ldo, o_win_stride;
} mi355x_window_attention_args;
int mi355x_window_attention(const mi355x_window_attention_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_SWIN_H */
