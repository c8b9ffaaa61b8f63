"""Recipes of the StyleAligned golden cases (tests/golden/sdxl_style_aligned.safetensors, written by tools/make_golden_style_aligned.py
from the REAL reference): SDXL with synthetic weights, one classifier-free-guidance DDIM step of a batch of images that share the style
of the first one.  Everything is rebuilt from seeds: weights (seed 0), inputs (`synth.sdxl_inputs(images, latent_hw, input_seed)`),
and for case d the adapters of golden case `sdxl_lora_ip` at this batch size."""
from __future__ import annotations

from typing import Any, Mapping, Sequence

from refiners_amd import synth
from tests.golden_cases import CASES, build_specs

COMMON = dict(weight_seed=0, num_steps=30, step=11, condition_scale=5.0)

STYLE_ALIGNED_CASES: dict[str, dict[str, Any]] = {
    # three images at 32 x 32 latents: 1024 / 256 tokens in the two transformer levels
    "a": dict(COMMON, images=3, latent_hw=(32, 32), input_seed=61, scale=0.5, adapters=False),
    # the SAME inputs at scale 1.0: what a live `adapter.scale = 1.0` on case a's tree must give
    "b": dict(COMMON, images=3, latent_hw=(32, 32), input_seed=61, scale=1.0, adapters=False),
    # 24 x 40 latents: 240 and 60 tokens, neither a multiple of 64 (padded keys, unaligned V^T halves)
    "c": dict(COMMON, images=2, latent_hw=(24, 40), input_seed=62, scale=0.7, adapters=False),
    # IP-Adapter + the two rank-16 LoRAs of `sdxl_lora_ip` UNDER the adapter: StyleAligned on top of the in-launch LoRA Q|K|V^T projections
    "d": dict(COMMON, images=2, latent_hw=(32, 32), input_seed=63, scale=0.6, adapters=True),
}


def case_specs(case: Mapping[str, Any], shapes: Mapping[str, Sequence[int]]) -> dict[str, Any]:
    """kwargs of synth.apply_adapters for a case (IP-Adapter tokens sized for the case's CFG batch)."""
    if not case["adapters"]:
        return {"loras": [], "ip": None, "control": []}
    return build_specs(dict(CASES["sdxl_lora_ip"], images=case["images"]), shapes)


def case_inputs(case: Mapping[str, Any]) -> dict[str, Any]:
    return synth.sdxl_inputs(case["images"], case["latent_hw"], case["input_seed"])


def pack_model(q, k, v, group: int, scale: float, eps: float = 1e-8):
    """Torch model of what mi355x_adain_stats + mi355x_style_aligned_pack compute, index arithmetic included: q, k, v [B, L, C] ->
    (AdaIN(q) [B, L, C], k_sh [B, Lkp, C], vt_sh [C, B, Lkp]) with r(b) = (b // group) * group, s_b = 1 on the reference rows and `scale`
    elsewhere, Lkp = 2 L rounded up to 64 and zero padding."""
    import torch

    B, L, C = q.shape
    rows = torch.arange(B, device=q.device)
    ref = rows // group * group
    s = torch.where(rows == ref, 1.0, float(scale)).to(q.dtype)[:, None, None]

    def adain(t):
        std, mean = torch.std_mean(t, dim=1, keepdim=True)
        return (t - mean) / (std + eps) * std[ref] + mean[ref]

    lkp = (2 * L + 63) // 64 * 64
    k_sh = torch.zeros(B, lkp, C, device=q.device, dtype=q.dtype)
    k_sh[:, :L], k_sh[:, L : 2 * L] = adain(k), s * k[ref]
    vt_sh = torch.zeros(C, B, lkp, device=q.device, dtype=q.dtype)
    vt_sh[:, :, :L], vt_sh[:, :, L : 2 * L] = v.permute(2, 0, 1), (s * v[ref]).permute(2, 0, 1)
    return adain(q), k_sh, vt_sh
