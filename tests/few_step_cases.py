"""Recipes of the few-step golden cases (tests/golden/sdxl_few_step.safetensors + sdxl_few_step.json, written by
tools/make_golden_few_step.py from the REAL reference): SDXL with synthetic weights, WITHOUT classifier-free guidance (cases a - d) --
LCM with its condition-scale adapter, Euler with trailing timesteps (noise and sample prediction: SDXL-Lightning's forms), DDIM, DPM-Solver++
-- and an LCM-LoRA-shaped LoRA attached by `add_lcm_lora` (cases b, e).  Everything is rebuilt from seeds: weights (seed 0), inputs
(`synth.sdxl_inputs(images, latent_hw, input_seed, cfg)`), the adapter's Linear, the LoRA's tensors, LCM's noise draws."""
from __future__ import annotations

from typing import Any, Mapping

import torch
from torch import Tensor

from refiners_amd import synth

FEW_STEP_CASES: dict[str, dict[str, Any]] = {
    # LCM: SDXLLcmAdapter(condition_scale 8.0), 4 steps, one image; `alt_scale`: x after step 0 once more with set_condition_scale(3.0)
    "a": dict(weight_seed=0, images=1, latent_hw=(16, 16), input_seed=71, solver="lcm", steps=4, cfg=False, lcm_scale=8.0, alt_scale=3.0, noise_seed=1234, lora=False),
    # Euler, trailing timesteps, noise prediction, two images at 24 x 40 latents (960 / 240 tokens: no multiple of 64), LCM-LoRA layout attached
    "b": dict(weight_seed=0, images=2, latent_hw=(24, 40), input_seed=72, solver="euler_trailing_noise", steps=4, cfg=False, lora=True),
    # SDXL-Lightning's one-step form: Euler(1, trailing, sample prediction)
    "c": dict(weight_seed=0, images=1, latent_hw=(16, 16), input_seed=73, solver="euler_trailing_sample", steps=1, cfg=False, lora=False),
    "d_ddim": dict(weight_seed=0, images=1, latent_hw=(16, 16), input_seed=74, solver="ddim", steps=4, cfg=False, lora=False),
    "d_dpm": dict(weight_seed=0, images=1, latent_hw=(16, 16), input_seed=74, solver="dpm", steps=4, cfg=False, lora=False),
    # case b's LoRA WITH guidance (add_lcm_lora on the guided path): one step at condition_scale 1.2
    "e": dict(weight_seed=0, images=2, latent_hw=(24, 40), input_seed=72, solver="euler_trailing_noise", steps=4, run_steps=1, cfg=True, condition_scale=1.2, lora=True),
}

LCM_EMBEDDING_DIM = 256
LORA_RANK, LORA_SEED, LORA_SCALE = 4, 9, 0.5


def _stage(parts: list[str]) -> tuple[str, int] | None:
    """UNet stage of a state-dict key -> (diffusers block name, index of the unit inside it): SDXL's layout (xl/unet.py:258-351)."""
    if parts[0] == "DownBlocks":
        c = int(parts[1].split("_")[1])
        return None if c == 1 else (f"down_blocks_{(c - 2) // 3}", (c - 2) % 3)  # Chain_1 is the input convolution
    if parts[0] == "MiddleBlock":
        return "mid_block", int(parts[1].split("_")[1]) - 1 if "_" in parts[1] else 0
    if parts[0] == "UpBlocks":
        c = int(parts[1].split("_")[1])
        return f"up_blocks_{(c - 1) // 3}", (c - 1) % 3
    return None


def lcm_lora_targets(shapes: Mapping[str, Any]) -> list[tuple[str, tuple[int, ...]]]:
    """(kohya key below "lora_unet_", shape of the target's weight) of every layer an LCM-LoRA file adapts, in the UNet's walk order: the
    attention and feed-forward Linears, proj_in / proj_out, the residual blocks' 3x3 convolutions, 1x1 shortcuts and time projections, the
    down- and up-samplers (NOT the input / output convolutions and the TimestepEncoder).  `shapes`: the bare UNet's state-dict keys
    (tests/golden/sdxl_unet_keys.json).  The coverage is complete because `auto_attach_loras` checks that a second copy of every LoRA finds no
    free compatible layer."""
    attn = {"Residual_1.SelfAttention.Distribute.Linear_1": "attn1_to_q", "Residual_1.SelfAttention.Distribute.Linear_2": "attn1_to_k",
            "Residual_1.SelfAttention.Distribute.Linear_3": "attn1_to_v", "Residual_1.SelfAttention.Linear": "attn1_to_out_0",
            "Residual_2.Attention.Distribute.Linear_1": "attn2_to_q", "Residual_2.Attention.Distribute.Linear_2": "attn2_to_k",
            "Residual_2.Attention.Distribute.Linear_3": "attn2_to_v", "Residual_2.Attention.Linear": "attn2_to_out_0",
            "Residual_3.Linear_1": "ff_net_0_proj", "Residual_3.Linear_2": "ff_net_2"}
    out: list[tuple[str, tuple[int, ...]]] = []
    for key, shape in shapes.items():
        if not key.endswith(".weight") or len(shape) not in (2, 4):
            continue
        parts = key[: -len(".weight")].split(".")
        st = _stage(parts)
        if st is None:
            continue
        block, unit = st
        rest = parts[1:] if parts[0] == "MiddleBlock" else parts[2:]
        head, tail = rest[0].split("_")[0], ".".join(rest[1:])
        if head == "ResidualBlock":
            name = {"Chain.RangeAdapter2d.Conv2d": "conv1", "Chain.RangeAdapter2d.Chain.Linear": "time_emb_proj", "Chain.Conv2d": "conv2", "Conv2d": "conv_shortcut"}.get(tail)
            if name is None:
                continue  # (the GroupNorms)
            if block == "mid_block":
                unit = 0 if rest[0].endswith("_1") else 1
            out.append((f"{block}_resnets_{unit}_{name}", tuple(shape)))
        elif head == "SDXLCrossAttention":
            if block == "mid_block":
                unit = 0
            if tail == "Chain_1.Linear":
                out.append((f"{block}_attentions_{unit}_proj_in", tuple(shape)))
            elif tail == "Chain_3.Linear":
                out.append((f"{block}_attentions_{unit}_proj_out", tuple(shape)))
            elif tail.startswith("Chain_2.CrossAttentionBlock"):
                tb = tail.split(".")[1]
                j = int(tb.split("_")[1]) - 1 if "_" in tb else 0
                name = attn.get(".".join(tail.split(".")[2:]))
                if name is not None:
                    out.append((f"{block}_attentions_{unit}_transformer_blocks_{j}_{name}", tuple(shape)))
        elif head == "Downsample" and tail == "Conv2d":
            out.append((f"{block}_downsamplers_0_conv", tuple(shape)))
        elif head == "Upsample" and tail.endswith("Conv2d"):
            out.append((f"{block}_upsamplers_0_conv", tuple(shape)))
    return out


def lcm_lora_tensors(shapes: Mapping[str, Any], rank: int = LORA_RANK, seed: int = LORA_SEED) -> dict[str, Tensor]:
    """A state dict in the layout of an LCM-LoRA file: `<key>.lora_down.weight`, `<key>.lora_up.weight` (down k x k for a convolution, up 1 x 1)
    and the scalar `<key>.alpha` such files carry (not a weight: the loaders skip it)."""
    out: dict[str, Tensor] = {}
    for key, w in lcm_lora_targets(shapes):
        full = f"lora_unet_{key}"
        if len(w) == 2:
            down, up = (rank, w[1]), (w[0], rank)
        else:
            down, up = (rank, w[1], w[2], w[3]), (w[0], rank, 1, 1)
        out[f"{full}.lora_down.weight"] = synth.synth_tensor(f"lcm_lora.{key}.down.weight", down, seed)
        out[f"{full}.lora_up.weight"] = synth.synth_tensor(f"lcm_lora.{key}.up.weight", up, seed, gain=0.5)
        out[f"{full}.alpha"] = torch.tensor(float(rank))
    return out


def condition_scale_weight(sinusoidal_dim: int = 320, seed: int = 0) -> Tensor:
    """The adapter's Linear(256 -> 320, no bias)."""
    return synth.synth_tensor("lcm.ConditionScaleBlock.Linear.weight", (sinusoidal_dim, LCM_EMBEDDING_DIM), seed)


def load_condition_scale_weight(unet: Any, device: Any = None, dtype: Any = None) -> None:
    """Into the injected ConditionScaleBlock of a reference or mirror tree (found by class name)."""
    block = next(m for m in unet.modules() if type(m).__name__ == "ConditionScaleBlock")
    linear = next(m for m in block.modules() if type(m).__name__ == "Linear")
    linear.weight = torch.nn.Parameter(condition_scale_weight().to(device=device, dtype=dtype), requires_grad=False)


def make_solver(case: Mapping[str, Any], api: Any) -> Any:
    """`api`: a namespace with DDIM, DPMSolver, LCMSolver and `euler(steps, spacing, prediction)` of the reference or of the mirror."""
    kind, n = case["solver"], case["steps"]
    if kind == "lcm":
        return api.LCMSolver(n)
    if kind == "ddim":
        return api.DDIM(n)
    if kind == "dpm":
        return api.DPMSolver(n)
    _, spacing, prediction = kind.split("_")
    return api.euler(n, spacing, prediction)


def case_inputs(case: Mapping[str, Any]) -> dict[str, Tensor]:
    return synth.sdxl_inputs(case["images"], case["latent_hw"], case["input_seed"], cfg=case["cfg"])


def noise_draws(case: Mapping[str, Any]) -> list[Tensor]:
    """LCM's re-noising draws in the order the solver makes them: float32 on the CPU from one generator seeded with the case's `noise_seed`
    (`torch.manual_seed` on the default generator gives the same stream)."""
    g = torch.Generator().manual_seed(case["noise_seed"])
    shape = (case["images"], 4, *case["latent_hw"])
    return [torch.randn(shape, generator=g) for _ in range(case["steps"] - 1)]


def noise_generator(case: Mapping[str, Any], after_trajectories: int = 0) -> torch.Generator:
    """The generator a run hands to the solver.  `after_trajectories`: advanced past that many whole trajectories' draws -- the reference run
    draws everything from ONE stream, so `a.alt_x0` (step 0 once more, after the 4-step trajectory) got the stream's NEXT draw."""
    g = torch.Generator().manual_seed(case["noise_seed"])
    shape = (case["images"], 4, *case["latent_hw"])
    for _ in range(after_trajectories * (case["steps"] - 1)):
        torch.randn(shape, generator=g)
    return g


def reference_debug_map() -> list[list[str]]:
    """refiners' own (key, module path) pairs of `add_lcm_lora` on the LoRA cases' tree, in attachment order: kept in the metadata of
    tests/golden/sdxl_few_step.safetensors; sdxl_few_step.json holds its length and SHA-256 per case."""
    import json
    from pathlib import Path

    from safetensors import safe_open

    with safe_open(str(Path(__file__).resolve().parent / "golden" / "sdxl_few_step.safetensors"), framework="pt") as f:
        return json.loads(f.metadata()["debug_map"])
