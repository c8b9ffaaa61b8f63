// mi355x_gemm_attention: a cross-attention's Q projection and the attention itself as one launch (include/mi355x_refiners_xattn.h).
// The kernel is the cross-attention form of the 4-wave GEMM (gemm_kernel.cuh, XATTN) with the short-K/V attention body of attn_short_body.cuh as its
// tail; this translation unit holds its two instances (with and without the in-launch LoRA) and the entry point, so that gemm.hip's build time does not grow.
#include "../../include/mi355x_refiners_xattn.h"
#include "gemm_kernel.cuh"

using namespace mi355x;

extern "C" int mi355x_gemm_attention(const mi355x_gemm_args* gemm, const mi355x_attn_args* attn, void* stream) {
    if (!gemm || !attn) return MI355X_EARG;
    if (gemm->dtype != MI355X_BF16 || attn->dtype != MI355X_BF16) return MI355X_EDTYPE;
    GemmP p;
    if (const int err = gemm_params(gemm, p, false)) return err;
    mi355x_attn::AttnP xa{};
    if (const int err = mi355x_attn::attn_params(attn, xa, false)) return err;
    // the shapes must describe one cross-attention: a column tile is a head, a row tile lies inside one batch element
    if (attn->D != 64 || (int64_t)gemm->N != (int64_t)attn->H * 64 || (int64_t)gemm->M != (int64_t)attn->B * attn->Lq || attn->Lq % 64) return MI355X_ESHAPE;
    const int nt0 = (xa.kv[0].Lk + 63) / 64, nt1 = xa.nstream > 1 ? (xa.kv[1].Lk + 63) / 64 : 0;
    if (nt0 + nt1 > 3) return MI355X_ESHAPE;
    if (nt0 + nt1 == 3 && !(nt0 == 2 && xa.kv[0].Lk - 64 <= 32 && xa.kv[1].Lk <= 32)) return MI355X_ESHAPE;  // tiles 1 and 2 must be half tiles (the LDS plan in gemm_kernel.cuh)
    // a plain GEMM
    if (gemm->nseg != 1 || gemm->conv || gemm->geglu || gemm->res || gemm->rowbias || gemm->out_t || gemm->out_f32 || gemm->ksplit > 1 || gemm->stats_out || gemm->colstats_out ||
        gemm->out_kblocked)
        return MI355X_ESHAPE;
    if (gemm->lora_b && (gemm->lora_groups != 1 || gemm->lora_r != 32)) return MI355X_ESHAPE;
    if (gemm->tile != 0 && gemm->tile != 4) return MI355X_ESHAPE;
    if (gemm->bias && (reinterpret_cast<uintptr_t>(gemm->bias) & 15)) return MI355X_ESHAPE;
    // 32-bit offsets: inside a tile's K / V^T slice (the buffer descriptors of the LDS-DMA loads) and, like the GEMM's own loader, below 2 GB per operand
    constexpr int64_t LIM = 0x7fffffff;
    if (p.seg[0].xbytes >= LIM || p.seg[0].wbytes >= LIM) return MI355X_ESHAPE;
    for (int s = 0; s < xa.nstream; ++s)
        if (64 * xa.kv[s].ldkb >= LIM || 64 * xa.kv[s].ldvtb >= LIM) return MI355X_ESHAPE;
    if ((int64_t)(attn->B - 1) * xa.obsb + (int64_t)(attn->Lq - 1) * xa.ldob + (int64_t)attn->H * 128 >= LIM) return MI355X_ESHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return p.lora_b ? launch_xattn<true>(p, xa, st) : launch_xattn<false>(p, xa, st);
}
