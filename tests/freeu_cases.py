"""Cases of the FreeU fixtures (tests/golden/freeu.safetensors and freeu_keys.json, written by tools/make_golden_freeu.py from the reference's own
UNets and SDFreeUAdapter on CPU float32): bare weights as `sd1_bare` / `sdxl_bare` draw them, a CFG pair of seeded latents and text tokens.  The SD1.5
latents are 40 x 24, so the two FreeU sites filter 5 x 3 planes (odd sizes, no power of two); SDXL's are 16 x 16, the smallest of the SDXL goldens
(4 x 4 planes)."""
from __future__ import annotations

SCALES = dict(backbone_scales=[1.2, 1.4], skip_scales=[0.9, 0.2])
#: name -> family, latent size, seeds, the timesteps run in sequence (SDXL: DDIM step `step` of `num_steps`, stored with its solver update); "sd1_lora": a LoRA under the adapter
CASES = {
    "sd1": dict(family="sd1", latent_hw=(40, 24), weight_seed=0, input_seed=61, timesteps=[500.0, 37.0]),
    "sd1_lora": dict(family="sd1", latent_hw=(40, 24), weight_seed=0, input_seed=61, timesteps=[500.0], lora_rank=16, lora_scale=0.8),
    "sdxl": dict(family="sdxl", latent_hw=(16, 16), weight_seed=0, input_seed=62, num_steps=50, step=10, condition_scale=5.0),
}


def inputs(case: str) -> dict:
    """SD1.5: x [1, 4, H, W] (the CFG pair shares it) and text [2, 77, 768]; SDXL: synth.sdxl_inputs of one image."""
    import torch

    from refiners_amd import synth

    c = CASES[case]
    if c["family"] == "sdxl":
        return synth.sdxl_inputs(1, c["latent_hw"], c["input_seed"])
    return {"x": torch.randn((1, 4, *c["latent_hw"]), generator=synth._gen("in.x", c["input_seed"])),
            "text": torch.randn((2, 77, 768), generator=synth._gen("in.text", c["input_seed"]))}


def mirror_api():
    """refiners_amd.namespace() with the mirror's SDFreeUAdapter."""
    from types import SimpleNamespace

    import refiners_amd
    from refiners_amd.latent_diffusion.freeu import SDFreeUAdapter

    return SimpleNamespace(**vars(refiners_amd.namespace()), SDFreeUAdapter=SDFreeUAdapter)


def inject(unet, api, case: str, shapes: dict, device=None, dtype=None):
    """SDFreeUAdapter(SCALES) on a (reference or mirror) UNet, after the case's LoRA.  `api`: the namespace synth.apply_adapters takes, with
    SDFreeUAdapter.  Returns the adapter, injected."""
    from refiners_amd import synth

    c = CASES[case]
    if "lora_rank" in c:  # (first: its key prefixes name the bare tree's Linears)
        from tests.ella_cases import unet_lora_targets

        spec = synth.lora_spec(shapes, "freeu_kv", c["lora_scale"], rank=c["lora_rank"], seed=3, targets=unet_lora_targets(shapes))
        synth.apply_adapters(unet, api, loras=[spec], device=device, dtype=dtype)
    return api.SDFreeUAdapter(target=unet, **SCALES).inject()


def repr_digest(tree) -> str:
    """sha256 of a tree's repr without the signatures its Lambdas print (as tests/test_wire_format.py compares trees)."""
    import hashlib
    import re

    return hashlib.sha256(re.sub(r"Lambda\(.*\)", "Lambda", repr(tree)).encode()).hexdigest()


def set_context(unet, case: str, timestep: float, device=None, dtype=None) -> None:
    import torch

    inp = inputs(case)
    unet.set_timestep(torch.tensor([timestep], device=device))
    unet.set_clip_text_embedding(inp["text"].to(device=device, dtype=dtype))
    if CASES[case]["family"] == "sdxl":
        unet.set_pooled_text_embedding(inp["pooled"].to(device=device, dtype=dtype))
        unet.set_time_ids(inp["time_ids"].to(device=device))


def pair(case: str, device=None, dtype=None):
    """The CFG pair's latents [2, 4, H, W]."""
    return inputs(case)["x"].to(device=device, dtype=dtype).expand(2, -1, -1, -1).contiguous()


def run_chain(unet, case: str, timestep: float, device=None, dtype=None):
    """The Chain forward (reference or mirror) of the CFG pair at one timestep: [2, 4, H, W]."""
    import torch

    set_context(unet, case, timestep, device, dtype)
    with torch.no_grad():
        return unet(pair(case, device, dtype))
