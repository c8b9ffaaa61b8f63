/*
 * mi355x_refiners_reference_only.h -- the joint self-attention of reference-only control in libmi355x_refiners.so
 * (refiners_amd/csrc/reference_only.hip; reference foundationals/latent_diffusion/reference_only_control.py).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, strides in ELEMENTS, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1) storage with float32 arithmetic, return value 0 or one of that
 * header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing and leaves its
 * output untouched.  It is a header of its own because mi355x_refiners.h is a frozen list; refiners_amd.native reads every header the
 * same way.  The call does not allocate, synchronise with the host, keep a pointer past its return or use atomics: every output
 * element is written by exactly one lane, replays are bit-equal.
 */
#ifndef MI355X_REFINERS_REFERENCE_ONLY_H
#define MI355X_REFINERS_REFERENCE_ONLY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mi355x_attention_joint -- SelfAttentionInjectionAdapter's two attentions and their blend, before the out-projection, in one launch:
 *   out[b] = mix[b] * softmax(scale * Q [K0 ; K1]^T) [V0 ; V1] + (1 - mix[b]) * softmax(scale * Q K0^T) V0
 * Non-causal, one head width D for Q, K and V.  Segment 0 is the sample's own keys, segment 1 the guide's.  The second term is the state
 * of the online softmax where segment 0 ends: no key is read twice.
 *   Layouts as for mi355x_attention_general: Q [B][Lq][H * D], K0 / K1 [B][Lk][H * D] and out [B][Lq][H * D] token-major with a row stride
 *   and a batch stride each (K may be a column slice of a wider buffer); V0^T / V1^T [H * D][...] with key columns, row stride ldvt and
 *   batch stride vt_batch_stride, every row readable and finite up to the next multiple of 64 keys OF ITS SEGMENT.  Each segment's last
 *   64-key tile is masked by that segment's own Lk.
 *   mix: B floats (float32, whatever `dtype`) in DEVICE memory, read by the kernel at every launch (a captured graph follows a new value);
 *   NULL = all ones.  A sample whose mix is exactly 1 does no snapshot work; one whose mix is exactly 0 does not read segment 1.
 * D * sizeof(element) % 16 == 0; D up to 160 (the instances of mi355x_attention_general with Dqk == Dv: 40, 64, 80, 128, 160 and what lies
 * below them).
 * Alignment: q, k0, k1, vt0, vt1 on 16 bytes, and their row and batch strides multiples of 16 bytes (8 bf16 or 4 f32 elements); out, ldo and
 * o_batch_stride multiples of 4 ELEMENTS (8 bytes in bf16, 16 in f32: a lane stores 4 elements at once); mix, where given, on 4 bytes.
 * ESHAPE: B, H, Lq, D < 1, an empty segment (Lk0 < 1 or Lk1 < 1), a D no instance serves (D > 160 or D * sizeof(element) % 16 != 0), any of the
 *         alignment rules above broken, the one for mix included.
 * EARG:   NULL q / k / vt / out, out overlapping q, a K or a V^T segment (out doubles as the kernel's parking space: a lane keeps the
 *         (1 - mix) term in its own output elements from the segment boundary to the end). */
typedef struct mi355x_attn_joint_args {
    int32_t dtype;
    int32_t B, H, Lq, D;
    int32_t Lk0, Lk1;
    const void* q;
    int64_t ldq, q_batch_stride;
    const void* k0;
    int64_t ldk0, k0_batch_stride;
    const void* vt0;
    int64_t ldvt0, vt0_batch_stride;
    const void* k1;
    int64_t ldk1, k1_batch_stride;
    const void* vt1;
    int64_t ldvt1, vt1_batch_stride;
    const void* mix;
    void* out;
    int64_t ldo, o_batch_stride;
    float scale;
} mi355x_attn_joint_args;
int mi355x_attention_joint(const mi355x_attn_joint_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_REFERENCE_ONLY_H */
