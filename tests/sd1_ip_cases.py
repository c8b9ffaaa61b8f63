"""Cases of the SD1.5 IP-Adapter fixtures (tests/golden/sd1_ip.safetensors and sd1_ip_keys.json, written by tools/make_golden_sd1_ip.py from the
reference's own SD1UNet and SD1IPAdapter on CPU float32): the bare UNet's weights as `sd1_bare` draws them, a CFG pair of 32 x 32 latents, 77 text
tokens and the adapter's image tokens as seeded unit normals (what its image projection hands over is layer-normed)."""
from __future__ import annotations

UNET = dict(batch=2, latent_hw=(32, 32), text_tokens=77, weight_seed=0, input_seed=41, ip_seed=9)
#: name -> adapter keywords, image tokens per sample, the timesteps run in sequence; "lora": a LoRA on the cross-attention K / V Linears, and a scale assigned later
CASES = {
    "plain": dict(fine_grained=False, tokens=4, scale=0.6, timesteps=[500.0]),
    "plus": dict(fine_grained=True, tokens=16, scale=1.0, timesteps=[500.0, 37.0]),
    "lora": dict(fine_grained=False, tokens=4, scale=0.6, timesteps=[500.0], lora_rank=16, lora_scale=0.8, rescale=0.25),
}
#: the DPM-Solver++ step stored for "plain": x_next of step STEP of NUM_STEPS with the CFG pair combined at CONDITION_SCALE
SOLVER = dict(num_steps=30, step=0, condition_scale=5.0)


def inputs(case: str) -> dict:
    """x [1, 4, H, W] (the CFG pair shares it), text [2, 77, 768] and image tokens [2, n, 768] = [negative ; conditional]."""
    import torch

    from refiners_amd import synth

    h, w = UNET["latent_hw"]
    seed = UNET["input_seed"]
    return {"x": torch.randn((1, 4, h, w), generator=synth._gen("in.x", seed)),
            "text": torch.randn((UNET["batch"], UNET["text_tokens"], 768), generator=synth._gen("in.text", seed)),
            "tokens": torch.randn((UNET["batch"], CASES[case]["tokens"], 768), generator=synth._gen(f"in.ip.{case}", seed))}


def inject(unet, api, case: str, shapes: dict, device=None, dtype=None, encoder=None):
    """SD1IPAdapter of a case on a (reference or mirror) SD1UNet through its public interface, image K / V matrices from synth.ip_spec, after the
    case's LoRA.  `api`: the namespace synth.apply_adapters takes, with SD1IPAdapter.  Returns the adapter, injected, tokens set."""
    import torch

    from refiners_amd import synth

    c = CASES[case]
    conv = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
    if "lora_rank" in c:  # (first: its key prefixes name the bare tree's Linears)
        from tests.ella_cases import unet_lora_targets

        spec = synth.lora_spec(shapes, "ip_kv", c["lora_scale"], rank=c["lora_rank"], seed=3, targets=unet_lora_targets(shapes))
        assert len(spec["pairs"]) == 32
        synth.apply_adapters(unet, api, loras=[spec], device=device, dtype=dtype)
    kv = synth.ip_spec(shapes, c["scale"], batch=UNET["batch"], num_tokens=c["tokens"], seed=UNET["ip_seed"])["kv"]
    ad = api.SD1IPAdapter(target=unet, clip_image_encoder=encoder or synth._NoImageEncoder(), scale=c["scale"], fine_grained=c["fine_grained"])
    assert len(ad.sub_adapters) == len(kv) == 16
    for sub, (wk, wv) in zip(ad.sub_adapters, kv.values()):
        sub.image_key_projection.weight = torch.nn.Parameter(conv(wk))
        sub.image_value_projection.weight = torch.nn.Parameter(conv(wv))
    ad.inject()
    ad.set_clip_image_embedding(conv(inputs(case)["tokens"]))
    return ad


def repr_digest(tree) -> str:
    """sha256 of a tree's repr without the signatures its Lambdas print (as tests/test_wire_format.py compares trees)."""
    import hashlib
    import re

    return hashlib.sha256(re.sub(r"Lambda\(.*\)", "Lambda", repr(tree)).encode()).hexdigest()


def run_chain(unet, case: str, timestep: float, device=None, dtype=None):
    """The Chain forward (reference or mirror) of the CFG pair at one timestep: [2, 4, H, W]."""
    import torch

    inp = inputs(case)
    unet.set_clip_text_embedding(inp["text"].to(device=device, dtype=dtype))
    unet.set_timestep(torch.tensor([timestep], device=device))
    with torch.no_grad():
        return unet(inp["x"].to(device=device, dtype=dtype).expand(UNET["batch"], -1, -1, -1).contiguous())
