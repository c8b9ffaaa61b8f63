"""Cases of the T2I-Adapter condition-encoder fixtures (tests/golden/t2i_encoder.safetensors, written by tools/make_golden_t2i_encoder.py from the
reference's own ConditionEncoder / ConditionEncoderXL / SD1UNet + SD1T2IAdapter on CPU float32).  Weights are drawn per key from a seeded CPU
generator over the tree's own key / shape list, pictures by seeded torch.rand: only the outputs are stored."""
from __future__ import annotations

import torch

from refiners_amd import synth

SEED = dict(weight_seed=23, input_seed=61)
CHANNELS = (64, 128, 256, 256)  # the narrowest widths whose bfloat16 rows are whole 128-byte blocks

#: name -> encoder class + keywords, picture [B, in_channels, H, W]
#:   sd1  r = 8, batch 2, an odd 9 x 13 map: floored by each of the three pools (4 x 6, 2 x 3, 1 x 1), a shortcut in two stages
#:   xl   r = 16, one picture channel, one block per stage, 5 x 7 -> one pool (2 x 3), shortcuts in stages 2 and 3
ENCODER_CASES = {
    "sd1": dict(cls="ConditionEncoder", kw=dict(in_channels=3, channels=CHANNELS, num_residual_blocks=2), shape=(2, 3, 72, 104)),
    "xl": dict(cls="ConditionEncoderXL", kw=dict(in_channels=1, channels=CHANNELS, num_residual_blocks=1), shape=(1, 1, 80, 112)),
}
#: one SD1UNet + SD1T2IAdapter (default encoder widths) step: 16 x 16 latents, a 128 x 128 picture
SD1_STEP = dict(latent_hw=(16, 16), text_tokens=77, unet_seed=0, timestep=400.0, scale=0.8, name="depth")


def picture(case: str, shift: int = 0):
    g = torch.Generator().manual_seed(SEED["input_seed"] + sum(map(ord, case)) + 1000 * shift)
    return torch.rand(ENCODER_CASES[case]["shape"], generator=g)


def draw(tree, seed_shift: int = 0) -> dict:
    """Synthetic float32 weights over a tree's own state-dict keys."""
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in tree.state_dict().items()}, SEED["weight_seed"] + seed_shift)


def encoder(case: str, module, device="cpu", dtype=None):
    """The case's encoder from `module` (the mirror's refiners_amd.latent_diffusion.t2i or the reference's t2i_adapter) with the drawn weights."""
    c = ENCODER_CASES[case]
    enc = getattr(module, c["cls"])(**c["kw"], device="meta")
    enc.load_state_dict({k: v.to(device=device, dtype=dtype or torch.float32) for k, v in draw(enc).items()}, assign=True)
    return enc


def sd1_inputs() -> dict:
    h, w = SD1_STEP["latent_hw"]
    s = SEED["input_seed"]
    return {"x": torch.randn((1, 4, h, w), generator=synth._gen("in.x", s)), "text": torch.randn((1, SD1_STEP["text_tokens"], 768), generator=synth._gen("in.text", s)),
            "picture": torch.rand((1, 3, 8 * h, 8 * w), generator=synth._gen("t2i.condition", s))}


def sd1_adapter(unet, adapter_cls, device="cpu", dtype=None):
    """SD1T2IAdapter (mirror's or reference's) injected into `unet`, its default encoder holding drawn weights."""
    ad = adapter_cls(unet, name=SD1_STEP["name"], scale=SD1_STEP["scale"])
    ad.condition_encoder.load_state_dict({k: v.to(device=device, dtype=dtype or torch.float32) for k, v in draw(ad.condition_encoder, 7).items()}, assign=True)
    return ad.inject()


def sd1_run(unet, features, device="cpu", dtype=None, call=None):
    """One forward (the Chain's, or `call`) with the adapter's features set: [1, 4, h, w]."""
    inp = sd1_inputs()
    unet.set_clip_text_embedding(inp["text"].to(device=device, dtype=dtype))
    unet.set_timestep(torch.tensor([SD1_STEP["timestep"]], device=device))
    unet.set_context("t2iadapter", {f"condition_features_{SD1_STEP['name']}": features})
    with torch.no_grad():
        return (call or unet)(inp["x"].to(device=device, dtype=dtype))
