"""Host-side mirror of refiners' Latent Consistency Model support for SDXL:

* `SDXLLcmAdapter` / `ConditionScaleBlock`  `stable_diffusion_xl/lcm.py:12-100`  (arXiv:2310.04378): the distilled UNet takes the guidance
  scale w as an INPUT -- a sinusoidal embedding of (w - 1) * 1000, projected to the timestep sinusoid's width and added to it inside
  the RangeEncoder -- and runs WITHOUT classifier-free guidance (`SDXLDenoiser(classifier_free_guidance=False)`,
  `CompiledSDXL(classifier_free_guidance=False)`).
* `add_lcm_lora`                            `stable_diffusion_xl/lcm_lora.py:8-78` (arXiv:2311.05556; SDXL-Lightning, arXiv:2402.13929,
  ships the same layout): a LoRA over attentions, feed-forwards, `proj_in` / `proj_out`, the residual blocks' convolutions, shortcuts and
  time projections, attached in two passes of `auto_attach_loras`.

Class names, child order and context keys follow the reference, so the lowering (which matches nodes by class name) treats refiners'
own tree the same way: refiners_amd.engine.unet_lowering.UNetLowering._fold_condition_scale turns the block into one bias row computed in
the prologue.
"""
from __future__ import annotations

import math
import re
from typing import Any

import torch
from torch import Tensor

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.adapters import Adapter, Lora, auto_attach_loras
from refiners_amd.fluxion.tree import Contexts

from .adapters import SDLoraManager
from .blocks import RangeEncoder


def compute_sinusoidal_embedding(x: Tensor, embedding_dim: int) -> Tensor:
    """One row [sin(x f_0) .. sin(x f_h-1) | cos(x f_0) .. cos(x f_h-1)] per value of x, h = embedding_dim / 2, f_i = 10000^(-i / (h - 1)),
    float32 whatever x is.  NOT the RangeEncoder's embedding: that one puts the cosines first and spreads the exponent over h, not h - 1.
    The frequencies are formed as exp(i * (-ln 10000) / (h - 1)) in float32, the rounding sequence the distilled weights were trained against
    (at x = 7000 a last-bit difference in f_i moves the angle by 1e-3)."""
    h = embedding_dim // 2
    steps = torch.arange(h, dtype=torch.float32, device=x.device)
    frequencies = torch.exp(steps * -math.log(10000) / (h - 1))
    angles = x.to(torch.float32)[:, None] * frequencies[None, :]
    return torch.cat((angles.sin(), angles.cos()), dim=1)


class ConditionScaleBlock(fl.Residual):
    """x + Linear(context lcm.condition_scale_embedding): one constant row added to the timestep sinusoid (no bias)."""

    def __init__(self, in_channels: int, out_channels: int, device: Any = None, dtype: Any = None) -> None:
        reader = fl.UseContext("lcm", "condition_scale_embedding")
        super().__init__(reader, fl.Converter(), fl.Linear(in_channels, out_channels, bias=False, device=device, dtype=dtype))


class SDXLLcmAdapter(fl.Chain, Adapter[fl.Chain]):
    """Wraps an SDXL UNet for `LCMSolver`: puts a `ConditionScaleBlock` in front of the RangeEncoder's first Linear and owns context "lcm".
    The guidance scale w is given HERE (`condition_scale`, `set_condition_scale`); the one passed to the denoiser is ignored, and the
    model runs without classifier-free guidance."""

    def __init__(self, target: fl.Chain, condition_scale_embedding_dim: int = 256, condition_scale: float = 7.5) -> None:
        if condition_scale_embedding_dim % 2:
            raise ValueError(f"condition_scale_embedding_dim must be even, got {condition_scale_embedding_dim}")
        self.condition_scale_embedding_dim = condition_scale_embedding_dim
        self.condition_scale = condition_scale
        with self.setup_adapter(target):
            super().__init__(target)

    @property
    def sinusoidal_embedding(self) -> Tensor:
        """[1, condition_scale_embedding_dim] float32 on the model's device, of the LIVE condition scale."""
        argument = torch.tensor([1000.0 * (self.condition_scale - 1.0)], device=self.device)
        return compute_sinusoidal_embedding(argument, self.condition_scale_embedding_dim)

    def _context(self) -> Contexts:
        return {"lcm": {"condition_scale_embedding": self.sinusoidal_embedding}}

    def init_context(self) -> Contexts:  # what the store is reset to after every forward: always the live scale
        return self._context()

    def set_condition_scale(self, scale: float) -> None:
        self.condition_scale = scale
        for name, value in self._context().items():
            self.set_context(name, value)

    def _encoder(self) -> RangeEncoder:
        return self.target.ensure_find(RangeEncoder)

    def inject(self, parent: fl.Chain | None = None) -> "SDXLLcmAdapter":
        encoder = self._encoder()
        first_linear = next(i for i, child in enumerate(encoder) if isinstance(child, fl.Linear))
        encoder.insert(first_linear, ConditionScaleBlock(self.condition_scale_embedding_dim, encoder.sinusoidal_embedding_dim,
                                                         device=self.target.device, dtype=self.target.dtype))
        return super().inject(parent)

    def eject(self) -> None:
        encoder = self._encoder()
        for child in [c for c in encoder if isinstance(c, ConditionScaleBlock)]:
            encoder.remove(child)
        super().eject()


# ------------------------------------------------------------------------------------------------ LCM-LoRA
_KEY_STAGE = re.compile(r"lora_unet_((?:down|up)_blocks_\d|mid_block)_")


def _stage_of_path(path: str) -> str | None:
    """The diffusers block a module path of the SDXL UNet lies in: three stages of three chains going down (the input convolution, Chain_1,
    counted with the first), the middle block, three stages of three chains going up.  None: not a path below `SDXLUNet`."""
    parts = path.split(".")
    if len(parts) < 2 or parts[0] != "SDXLUNet":
        return None
    if parts[1] == "MiddleBlock":
        return "mid_block"
    if parts[1] in ("DownBlocks", "UpBlocks") and len(parts) > 2 and parts[2].startswith("Chain_"):
        chain = int(parts[2][len("Chain_"):])
        return f"down_blocks_{max(chain - 2, 0) // 3}" if parts[1] == "DownBlocks" else f"up_blocks_{(chain - 1) // 3}"
    return None


def _check_placement(placed: list[tuple[str, str]]) -> None:
    """Attachment is by shape and walk order, not by name: a key that names a block must have landed in that block."""
    for key, path in placed:
        named = _KEY_STAGE.match(key)
        if named is not None and _stage_of_path(path) != named[1]:
            raise AssertionError(f"bad mapping: {key} {path}")


def add_lcm_lora(manager: SDLoraManager, tensors: dict[str, Tensor], name: str = "lcm", scale: float = 8.0 / 64.0, check_validity: bool = True,
                 debug_map: list[tuple[str, str]] | None = None) -> None:
    """Attach an LCM-LoRA file -- or one of the same layout, such as SDXL-Lightning's -- to the manager's SDXL UNet at `scale` (alpha / rank of
    those files; leave it).  `SDLoraManager.add_loras` cannot place this layout: `proj_in` / `proj_out` name Linears that sit inside
    `SDXLCrossAttention` but outside every `CrossAttentionBlock`, so those keys go first under that filter and the others through
    `add_loras_to_unet`.  `check_validity`: every key that names a UNet block must have landed in it.  `debug_map` receives the (key, module
    path) pairs in attachment order.  Usable with classifier-free guidance too (scales of 1 - 2) and without."""
    unet = manager.unet
    loras = Lora.from_dict(name, {k: t.to(device=unet.device, dtype=unet.dtype) for k, t in tensors.items()})
    foreign = [k for k in loras if not k.startswith("lora_unet_")]
    if foreign:
        raise AssertionError(f"not UNet keys: {foreign[:3]}")
    projections, others = {}, {}
    for key in sorted(loras, key=SDLoraManager.sort_keys):
        (projections if key.endswith(("proj_in", "proj_out")) else others)[key] = loras[key]
    placed: list[tuple[str, str]] = []
    auto_attach_loras(projections, unet, include=["SDXLCrossAttention"], exclude=["CrossAttentionBlock"], debug_map=placed)
    manager.add_loras_to_unet(others, debug_map=placed)
    if check_validity:
        _check_placement(placed)
    if debug_map is not None:
        debug_map.extend(placed)
    manager.set_scale(name, scale)
