// The wide-head half of mi355x_attention_general: head widths above attn_general_kernel.cuh's instances, up to (Dqk, Dv) = (512, 512).
// The kernel and its design notes are attn_wide_kernel.cuh's.  A translation unit of its own, so that the 128-accumulator kernel compiles beside
// attention_general.hip's instances, not after them; mi355x_attention_general (attention_general.hip) has checked the arguments and calls
// mi355x::attention_wide where its own instance table ends.  Not an export of the C ABI.
#include "attn_wide_kernel.cuh"

namespace mi355x {

// `a` has passed every check of mi355x_attention_general.  MI355X_ESHAPE for a width above 512.
int attention_wide(const mi355x_attn_general_args* a, hipStream_t st) {
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    GAttnP p{};
    p.B = a->B, p.H = a->H, p.Lq = a->Lq, p.seg[0].Lk = a->Lk, p.Dqk = a->Dqk, p.Dv = a->Dv, p.causal = a->causal ? 1 : 0;
    p.q = static_cast<const char*>(a->q), p.seg[0].k = static_cast<const char*>(a->k), p.seg[0].vt = static_cast<const char*>(a->vt), p.out = static_cast<char*>(a->out);
    p.ldqb = a->ldq * es, p.qbsb = a->q_batch_stride * es, p.seg[0].ldkb = a->ldk * es, p.seg[0].kbsb = a->k_batch_stride * es;
    p.seg[0].ldvtb = a->ldvt * es, p.seg[0].vtbsb = a->vt_batch_stride * es, p.ldob = a->ldo * es, p.obsb = a->o_batch_stride * es;
    p.c = a->scale * 1.44269504088896340736f;
    p.out_scale = a->out_scale;
    return a->dtype == MI355X_F32 ? attn_wide_dispatch<float>(p, st) : attn_wide_dispatch<bf16_t>(p, st);
}

}  // namespace mi355x
