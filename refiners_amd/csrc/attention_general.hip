// mi355x_attention, general head shapes: softmax(scale * Q K^T [causal]) V with a QK width Dqk and a V width Dv that need not
// be 64 and need not be equal.
//
// Who needs it (reference shapes): SD1.5's 8 heads over 320 / 640 / 1280 channels (head dims 40 / 80 / 160,
// stable_diffusion_1/unet.py:30-45), SegmentAnything ViT-H (16 heads of 80 whose decomposed relative-position bias is
// folded by the host into extra Q / K feature columns, so Dqk = 112 or 208 while Dv = 80,
// segment_anything/image_encoder.py:82-127), CLIP-style causal self-attention (is_causal, layers/attentions.py:60-202).
//
// The kernel, its launcher and the instance table are attn_general_kernel.cuh's (JOINT = false: one key segment; reference_only.hip runs the
// same loop over two).  This file holds the entry point: argument checks, the parameter block, and the switch between the two bf16 instances.
#include "attn_general_kernel.cuh"

namespace {

int g_gattn_fast = 1;  // bf16 launches take the FAST instance (mi355x_attention_general_set_fast: A/B and tests)

}  // namespace

extern "C" int mi355x_attention_general_set_fast(int v) {  // probing / A-B only, not part of the stable contract
    g_gattn_fast = v ? 1 : 0;
    return MI355X_OK;
}

extern "C" int mi355x_attention_general(const mi355x_attn_general_args* a, void* stream) {
    if (!a || !a->q || !a->k || !a->vt || !a->out) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->Lk <= 0 || a->Dqk <= 0 || a->Dv <= 0) return MI355X_ESHAPE;
    // every head's Q / K row segment and every V^T row must start on a 16-byte boundary; Dv % 4: a lane stores whole groups of four output
    // columns d0 = 16 i + 4 g .. d0 + 3 and skips a group that crosses Dv, so with a Dv that is no multiple of 4 the last columns would stay unwritten
    if ((a->Dqk * es) % 16 || (a->ldq * es) % 16 || (a->ldk * es) % 16 || (a->ldvt * es) % 16 || a->ldo % 4 || a->Dv % 4) return MI355X_ESHAPE;
    if ((a->q_batch_stride * es) % 16 || (a->k_batch_stride * es) % 16 || (a->vt_batch_stride * es) % 16 || a->o_batch_stride % 4) return MI355X_ESHAPE;
    if (!al16(a->q) || !al16(a->k) || !al16(a->vt) || (reinterpret_cast<uintptr_t>(a->out) & (4 * es - 1))) return MI355X_ESHAPE;
    GAttnP p{};
    p.B = a->B, p.H = a->H, p.Lq = a->Lq, p.seg[0].Lk = a->Lk, p.Dqk = a->Dqk, p.Dv = a->Dv, p.causal = a->causal ? 1 : 0;
    p.q = static_cast<const char*>(a->q), p.seg[0].k = static_cast<const char*>(a->k), p.seg[0].vt = static_cast<const char*>(a->vt), p.out = static_cast<char*>(a->out);
    p.ldqb = a->ldq * es, p.qbsb = a->q_batch_stride * es, p.seg[0].ldkb = a->ldk * es, p.seg[0].kbsb = a->k_batch_stride * es;
    p.seg[0].ldvtb = a->ldvt * es, p.seg[0].vtbsb = a->vt_batch_stride * es, p.ldob = a->ldo * es, p.obsb = a->o_batch_stride * es;
    p.c = a->scale * 1.44269504088896340736f;
    p.thr = p.c > 0.f ? 8.0f / p.c : 0.f;
    p.out_scale = a->out_scale;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return a->dtype == MI355X_F32 ? attn_general_dispatch<float, false>(p, st) : attn_general_dispatch<bf16_t, false>(p, st, g_gattn_fast != 0);
}
