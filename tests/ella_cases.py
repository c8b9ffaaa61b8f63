"""Cases of the ELLA fixtures (tests/golden/ella_keys.json and ella*.safetensors, written by tools/make_golden_ella.py from the reference's
own classes): encoder configurations, the synthetic weight draw, seeded inputs, a float64 torch model of mi355x_ella_adaln, and the digest of a
lowered program the "plain trees lower as before" test compares."""
from __future__ import annotations

import hashlib
import json
from functools import lru_cache
from pathlib import Path

ELLA_SEED = dict(weight_seed=17, input_seed=29)
GOLD = Path(__file__).resolve().parent / "golden"

#: the SD1 adapter's encoder (stable_diffusion_1/ella_adapter.py) at 2 layers instead of 6, which keeps the fixture small
_SD1 = dict(time_channel=320, timestep_embedding_dim=768, width=768, num_layers=2, num_heads=8, num_latents=64, input_dim=2048)
#: name -> ELLA keywords, batch, text tokens, and the timesteps run in sequence on one engine (a number: shared by the batch; a list: one per row)
#:   sd1      SD1's own shape, T = 128: Lk = 192, three full 64-key tiles
#:   sd1_t77  T = 77 with per-row timesteps: Lk = 141, a ragged last tile and 51 zero rows
#:   odd      width 192, 2 heads (head dim 96 again), 16 latents (Nlp = 64: 48 padding rows per sample), T = 5, no input Linear, an OutputProjection
ELLA_CASES = {
    "sd1": dict(model=_SD1, batch=2, tokens=128, timesteps=[500.0, 37.0]),
    "sd1_t77": dict(model=_SD1, batch=2, tokens=77, timesteps=[[981.0, 12.0], [3.0, 640.0]]),
    "odd": dict(model=dict(time_channel=64, timestep_embedding_dim=192, width=192, num_layers=2, num_heads=2, num_latents=16, input_dim=None, out_dim=96),
                batch=3, tokens=5, timesteps=[250.0, [7.0, 999.0, 420.0]]),
}
#: the whole SD1 UNet with SD1ELLAAdapter (6 layers): B = 2, 32 x 32 latents, T = 77; UNet weights of tests/support.weights("sd1", 0)
UNET_CASE = dict(batch=2, latent_hw=(32, 32), tokens=77, timesteps=[500.0, 37.0], unet_weight_seed=0, lora_rank=16, lora_scale=0.8)


def llm_width(case: str) -> int:
    m = ELLA_CASES[case]["model"]
    return m["input_dim"] or m["width"]


def llm_embedding(case: str, shift: int = 0):
    """The LLM's token embeddings of a case, [B, T, width], standard normal."""
    import torch

    c = ELLA_CASES[case]
    g = torch.Generator().manual_seed(ELLA_SEED["input_seed"] + sum(map(ord, case)) + 1000 * shift)
    return torch.randn((c["batch"], c["tokens"], llm_width(case)), generator=g)


def timestep(value):
    """A case's timestep as the tensor the reference's context takes: [1] shared, or [B, 1] per row (RangeEncoder broadcasts both)."""
    import torch

    return torch.tensor([value]) if not isinstance(value, list) else torch.tensor(value).unsqueeze(1)


def unet_inputs(shift: int = 0) -> dict:
    """Latents and LLM embeddings of UNET_CASE."""
    import torch

    c = UNET_CASE
    g = torch.Generator().manual_seed(ELLA_SEED["input_seed"] + 7 + 1000 * shift)
    return {"x": torch.randn((c["batch"], 4) + tuple(c["latent_hw"]), generator=g), "llm": torch.randn((c["batch"], c["tokens"], 2048), generator=g)}


@lru_cache(maxsize=None)
def key_shapes(name: str) -> dict[str, tuple[int, ...]]:
    """State-dict keys and shapes of a case's encoder ("sd1_full": the 6-layer encoder of SD1ELLAAdapter), in the reference's order."""
    return {k: tuple(v) for k, v in json.loads((GOLD / "ella_keys.json").read_text())[name].items()}


def draw_weights(shapes: dict, name: str = "") -> dict:
    """synth.synth_state_dict over the key / shape list, with two exceptions.  The reference zero-initialises every AdaLayerNorm Linear, which
    would hide the modulation: those weights are drawn like any matrix (the 2 C outputs then have unit scale for a unit-scale SiLU'd embedding) and
    their biases with standard deviation 0.5, so that scale rows are of order 0.5 and differ per batch row with the timestep.  The latents
    Parameter has standard deviation 1 (the reference's own draw is sqrt(width): layer-normed at once, any scale does)."""
    from refiners_amd import synth

    seed = ELLA_SEED["weight_seed"]
    sd = synth.synth_state_dict(shapes, seed)
    for k, s in shapes.items():
        if ".AdaLayerNorm" in k and k.endswith("Linear.bias"):
            sd[k] = synth.synth_tensor(k, s, seed) * 5.0
        elif k.endswith("ParameterInitialized.weight"):
            sd[k] = synth.synth_tensor(k, s, seed, gain=s[1] ** 0.5)
    return sd


def weights(name: str) -> dict:
    return draw_weights(key_shapes(name), name)


def mirror(case: str, device="cpu", dtype=None):
    """The mirror's ELLA of a case with the fixture's weights loaded."""
    import torch

    from refiners_amd.latent_diffusion.ella import ELLA

    dtype = dtype or torch.float32
    model = ELLA(**ELLA_CASES[case]["model"], device="meta")
    model.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in weights(case).items()}, assign=True)
    return model


def run_tree(ella, timestep_value, llm):
    """What a forward of the ELLA chain (the mirror's or the reference's) leaves in context ella.latents."""
    import torch

    # the context store is reset when the forward returns: the writer's own callback hook hands the value over as it is written
    seen = {}
    writer = list(ella._modules.values())[-1]  # SetContext ella.latents
    assert (writer.context, writer.key) == ("ella", "latents") and writer.callback is None
    writer.callback = lambda _current, value: seen.__setitem__("latents", value)
    try:
        ella.set_context("ella", {"timestep_embedding": None, "latents": None})  # (ELLAAdapter.init_context provides it once the encoder sits in a UNet)
        ella.set_context("diffusion", {"timestep": timestep(timestep_value).to(llm.device)})
        ella.set_context("adapted_cross_attention_block", {"llm_text_embedding": llm})
        with torch.no_grad():
            ella(torch.zeros(1, device=llm.device))
    finally:
        writer.callback = None
    return seen["latents"]


def unet_lora_targets(shapes: dict) -> list[str]:
    """Key prefixes of the cross-attention K / V Linears of the bare SD1 UNet (the Linears that read ELLA's tokens), in walk order."""
    return [k[: -len(".weight")] for k in shapes if ".Residual_2.Attention.Distribute.Linear_" in k and k.endswith(".weight") and k.split(".")[-2] in ("Linear_2", "Linear_3")]


# ------------------------------------------------------------------------------------------------ float64 model of mi355x_ella_adaln
def adaln_model(latents, shift_l, scale_l, Lp: int, x=None, shift_x=None, scale_x=None, eps: float = 1e-6):
    """[LN0(latents) * (1 + scale_l) + shift_l ; LN0(x) * (1 + scale_x) + shift_x ; zero rows] in float64: latents [B, Nl, C], x [B, T, C] or None,
    shift / scale [B, C] -> [B, Lp, C].  LN0: biased variance, no affine."""
    import torch

    def ln0(t):
        t = t.double()
        mu = t.mean(-1, keepdim=True)
        var = ((t - mu) ** 2).mean(-1, keepdim=True)
        return (t - mu) / torch.sqrt(var + eps)

    parts = [ln0(latents) * (1 + scale_l.double().unsqueeze(1)) + shift_l.double().unsqueeze(1)]
    if x is not None and x.shape[1]:
        parts.append(ln0(x) * (1 + scale_x.double().unsqueeze(1)) + shift_x.double().unsqueeze(1))
    y = torch.cat(parts, 1)
    B, rows, C = y.shape
    return torch.cat([y, torch.zeros(B, Lp - rows, C, dtype=torch.float64, device=y.device)], 1)


# ------------------------------------------------------------------------------------------------ program digests
def program_digest(ops: list) -> dict:
    """Launch count, launches per entry point and a hash over the sequence of (entry point, GEMM signature and epilogue code) of a recorded program."""
    from refiners_amd import native

    names, counts = [], {}
    for fn, args, what, _keep in ops:
        if fn is None:
            names.append(f"python:{what}")
            continue
        sig = f"{native.gemm_signature(args[0]._obj)} e{args[0]._obj.geglu}" if what == "mi355x_gemm" else ""
        names.append(f"{what} {sig}".strip())
        counts[what] = counts.get(what, 0) + 1
    return {"launches": sum(counts.values()), "counts": dict(sorted(counts.items())), "sha256": hashlib.sha256("\n".join(names).encode()).hexdigest()}


def bare_program(family: str, dtype):
    """Dry lowering (meta device) of the bare SD1 / SDXL UNet at a CFG pair of 32 x 32 latents and 77 text tokens -> {"step": digest, "prologue": digest}."""
    import torch

    from refiners_amd.engine.unet_lowering import UNetIO, UNetLowering
    from refiners_amd.latent_diffusion.sd1 import SD1UNet
    from refiners_amd.latent_diffusion.sdxl import SDXLUNet

    dev, B, H, W = torch.device("meta"), 2, 32, 32
    unet = (SD1UNet if family == "sd1" else SDXLUNet)(4, device="meta", dtype=dtype)
    io = UNetIO(x=torch.empty(B, 4, H, W, device=dev, dtype=dtype), timestep=torch.empty(B, device=dev), out=torch.empty(B, 4, H, W, device=dev, dtype=dtype))
    if family == "sdxl":
        io.pooled = torch.empty(B, 1280, device=dev, dtype=dtype)
        io.time_ids = torch.empty(B, 6, device=dev)
    io.tokens[("cross_attention_block", "clip_text_embedding")] = (torch.zeros(B * 128, 768 if family == "sd1" else 2048, device=dev, dtype=dtype), 77)
    low = UNetLowering(dev, dtype)
    low.lower(unet, io)
    return {"step": program_digest(low.step), "prologue": program_digest(low.prologue)}


BARE_PROGRAMS = [("sd1", "float32"), ("sd1", "bfloat16"), ("sdxl", "float32"), ("sdxl", "bfloat16")]
