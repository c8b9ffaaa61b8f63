"""Cases of the reference-only fixtures (tests/golden/reference_only*.safetensors, written by tools/make_golden_reference_only.py from the
reference's own SD1UNet + ReferenceOnlyControlAdapter on CPU float32): shapes, seeded inputs, the LoRA's targets, and the builder both the
tool (on the reference's classes) and the tests (on the mirror's) go through."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Any

SEED = dict(weight_seed=0, input_seed=43)
TOKENS = 77
#: name -> latent size and the golden keys it provides.  Every case is a CFG pair (B = 2) whose two rows differ in the latents, the guide and the text.
#:   main  32 x 32 latents: self-attention over L = 1024 / 256 / 64 / 16 keys per segment (16 whole tiles ... a quarter of one)
#:   odd   24 x 40 latents: L = 960 / 240 / 60 / 15, no level a multiple of 64 keys, so every level masks both segments' tail tiles
CASES = {
    "main": dict(latent_hw=(32, 32), timesteps=[500.0, 37.0]),
    "odd": dict(latent_hw=(24, 40), timesteps=[500.0]),
}
#: golden key -> what produced it (style_cfg 0.5 unless named)
#:   main.t0 / main.t1      the adapted tree at the case's two timesteps
#:   main.s1 / main.s0      timestep 0 with style_cfg 1.0 / 0.0
#:   main.lora              timestep 0 with a rank-16 LoRA on the 64 self-attention Linears (q, k, v, out of the 16 sites), injected BEFORE the adapter
#:   main.bare              timestep 0 after eject(): the bare UNet
#:   odd.t0                 the adapted tree at 24 x 40
STYLES = {"s1": 1.0, "s0": 0.0}
LORA = dict(rank=16, scale=0.8, seed=5)


def inputs(case: str) -> dict:
    """Latents x, the guide (the UNet input's shape) and the CLIP text embedding of a case: rows differ."""
    import torch

    h, w = CASES[case]["latent_hw"]
    g = torch.Generator().manual_seed(SEED["input_seed"] + sum(map(ord, case)))
    return {"x": torch.randn((2, 4, h, w), generator=g), "guide": torch.randn((2, 4, h, w), generator=g), "text": torch.randn((2, TOKENS, 768), generator=g)}


def timestep(value: float):
    import torch

    return torch.tensor([value])


def lora_targets(shapes: dict) -> list[str]:
    """Key prefixes of the self-attention Linears of the bare SD1 UNet (Distribute.Linear_1..3 and the out-projection), in walk order."""
    return [k[: -len(".weight")] for k in shapes if ".Residual_1.SelfAttention." in k and k.endswith(".weight") and k.split(".")[-2].startswith("Linear")]


def lora_api(ns: Any) -> Any:
    """What synth.apply_adapters needs of a namespace with `fl`, `LinearLora`, `Conv2dLora`, `LoraAdapter`."""
    return SimpleNamespace(fl=ns.fl, LinearLora=ns.LinearLora, Conv2dLora=ns.Conv2dLora, LoraAdapter=ns.LoraAdapter)


def add_lora(unet: Any, api: Any, shapes: dict, device: Any = None, dtype: Any = None) -> None:
    from refiners_amd import synth

    spec = synth.lora_spec(shapes, "reference_only_sa", LORA["scale"], rank=LORA["rank"], seed=LORA["seed"], targets=lora_targets(shapes))
    assert len(spec["pairs"]) == 64
    synth.apply_adapters(unet, api, loras=[spec], device=device, dtype=dtype)


def run(unet: Any, adapter: Any, case: str, ts: float, device: Any = "cpu", dtype: Any = None):
    """One stock forward of the (reference's or mirror's) tree at a case's inputs."""
    import torch

    inp = {k: v.to(device=device, dtype=dtype) for k, v in inputs(case).items()}
    if adapter is not None:
        adapter.set_controlnet_condition(inp["guide"])
    unet.set_clip_text_embedding(inp["text"])
    unet.set_timestep(timestep(ts).to(device))
    with torch.no_grad():
        return unet(inp["x"].clone()).contiguous()
