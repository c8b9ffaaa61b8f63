// mi355x_attention_joint: the self-attention of reference-only control (foundationals/latent_diffusion/reference_only_control.py of the
// reference, SelfAttentionInjectionAdapter) as one launch:
//   out[b] = mix[b] * softmax(scale * Q [K0 ; K1]^T) [V0 ; V1] + (1 - mix[b]) * softmax(scale * Q K0^T) V0
// Segment 0 is the sample's own keys, segment 1 the keys the guide pass projected at the same site.  The second term is the online
// softmax's own state at the moment segment 0 ends (O / l over the keys seen so far), so neither attention reads a key twice.
//
// The kernel, its launcher and the instance table are attn_general_kernel.cuh's (JOINT = true), the tile loop that attention_general.hip runs over
// one segment: what the two segments, the snapshot and mix add to it is described there.  This file holds the entry point: argument checks
// (no input may overlap `out`, which the kernel reads back) and the parameter block.
#include "attn_general_kernel.cuh"
#include "../../include/mi355x_refiners_reference_only.h"

namespace {

// bytes spanned by B batch rows of `rows` rows of `cols` elements
inline int64_t span(int64_t B, int64_t bs, int64_t rows, int64_t ld, int64_t cols, int es) { return ((B - 1) * bs + (rows - 1) * ld + cols) * es; }

}  // namespace

extern "C" int mi355x_attention_joint(const mi355x_attn_joint_args* a, void* stream) {
    if (!a || !a->q || !a->k0 || !a->vt0 || !a->k1 || !a->vt1 || !a->out) return MI355X_EARG;
    if (a->dtype != MI355X_F32 && a->dtype != MI355X_BF16) return MI355X_EDTYPE;
    const int es = a->dtype == MI355X_F32 ? 4 : 2;
    if (a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->D <= 0 || a->Lk0 <= 0 || a->Lk1 <= 0 || a->D > 160) return MI355X_ESHAPE;
    // every head's Q / K row segment and every V^T row must start on a 16-byte boundary
    if ((a->D * es) % 16 || (a->ldq * es) % 16 || (a->ldk0 * es) % 16 || (a->ldvt0 * es) % 16 || (a->ldk1 * es) % 16 || (a->ldvt1 * es) % 16 || a->ldo % 4) return MI355X_ESHAPE;
    if ((a->q_batch_stride * es) % 16 || (a->k0_batch_stride * es) % 16 || (a->vt0_batch_stride * es) % 16 || (a->k1_batch_stride * es) % 16 ||
        (a->vt1_batch_stride * es) % 16 || a->o_batch_stride % 4)
        return MI355X_ESHAPE;
    if (!al16(a->q) || !al16(a->k0) || !al16(a->vt0) || !al16(a->k1) || !al16(a->vt1) || (reinterpret_cast<uintptr_t>(a->out) & (4 * es - 1)) ||
        (reinterpret_cast<uintptr_t>(a->mix) & 3))
        return MI355X_ESHAPE;
    const int64_t HD = (int64_t)a->H * a->D;
    const int64_t obytes = span(a->B, a->o_batch_stride, a->Lq, a->ldo, HD, es);
    const int64_t lp0 = ((int64_t)a->Lk0 + 63) / 64 * 64, lp1 = ((int64_t)a->Lk1 + 63) / 64 * 64;
    if (overlap(a->q, span(a->B, a->q_batch_stride, a->Lq, a->ldq, HD, es), a->out, obytes) ||
        overlap(a->k0, span(a->B, a->k0_batch_stride, a->Lk0, a->ldk0, HD, es), a->out, obytes) ||
        overlap(a->k1, span(a->B, a->k1_batch_stride, a->Lk1, a->ldk1, HD, es), a->out, obytes) ||
        overlap(a->vt0, span(a->B, a->vt0_batch_stride, HD, a->ldvt0, lp0, es), a->out, obytes) ||
        overlap(a->vt1, span(a->B, a->vt1_batch_stride, HD, a->ldvt1, lp1, es), a->out, obytes))
        return MI355X_EARG;
    GAttnP p{};
    p.B = a->B, p.H = a->H, p.Lq = a->Lq, p.Dqk = p.Dv = a->D, p.seg[0].Lk = a->Lk0, p.seg[1].Lk = a->Lk1;
    p.q = static_cast<const char*>(a->q), p.out = static_cast<char*>(a->out), p.mix = static_cast<const float*>(a->mix);
    p.seg[0].k = static_cast<const char*>(a->k0), p.seg[0].vt = static_cast<const char*>(a->vt0), p.seg[1].k = static_cast<const char*>(a->k1), p.seg[1].vt = static_cast<const char*>(a->vt1);
    p.ldqb = a->ldq * es, p.qbsb = a->q_batch_stride * es, p.ldob = a->ldo * es, p.obsb = a->o_batch_stride * es;
    p.seg[0].ldkb = a->ldk0 * es, p.seg[0].kbsb = a->k0_batch_stride * es, p.seg[0].ldvtb = a->ldvt0 * es, p.seg[0].vtbsb = a->vt0_batch_stride * es;
    p.seg[1].ldkb = a->ldk1 * es, p.seg[1].kbsb = a->k1_batch_stride * es, p.seg[1].ldvtb = a->ldvt1 * es, p.seg[1].vtbsb = a->vt1_batch_stride * es;
    p.c = a->scale * 1.44269504088896340736f;
    p.thr = p.c > 0.f ? 8.0f / p.c : 0.f;
    p.out_scale = 1.f;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return a->dtype == MI355X_F32 ? attn_general_dispatch<float, true>(p, st) : attn_general_dispatch<bf16_t, true>(p, st);
}
