"""Host-side mirror of refiners' MultiDiffusion (https://arxiv.org/abs/2302.08113):

* `Tile`, `Size`, `DiffusionTarget`, `MultiDiffusion`   reference latent_diffusion/multi_diffusion.py:15-175
* `SDXLTarget`, `SDXLMultiDiffusion`                    reference stable_diffusion_xl/multi_diffusion.py:9-33
* `SD1DiffusionTarget`, `SD1MultiDiffusion`             reference stable_diffusion_1/multi_diffusion.py:11-33

A canvas larger than one UNet call is denoised as a list of targets: each target is a tile of the canvas with its own prompt, guidance
scale, solver instance, weight, optional opacity mask, optional init latents and step window.  One call of `MultiDiffusion` takes every
active target one denoising step further and blends the results back: `where(num_updates > 0, cumulative / num_updates, x)`.

This file is the unfused torch path, with the reference's formulas and operation order; `refiners_amd.engine.multi_diffusion.
CompiledMultiDiffusion` runs the same step as batched UNet launches between three streaming kernels (mi355x_md_gather, mi355x_md_target_step,
mi355x_md_blend).  Per-target ControlLora / ControlNet conditions and IP-Adapter embeddings, the tiled VAE and the `MultiUpscaler` pipeline of
the reference are not mirrored.
"""
from __future__ import annotations

import math
from abc import ABC, abstractmethod
from dataclasses import dataclass
from typing import Any, Generic, NamedTuple, Sequence, TypeVar

import torch
from torch import Tensor

from .sampling import SDXLDenoiser

MAX_STEPS = 1000


class Tile(NamedTuple):
    top: int
    left: int
    bottom: int
    right: int


class Size(NamedTuple):
    height: int
    width: int


@dataclass(kw_only=True)
class DiffusionTarget:
    """One area of the canvas (multi_diffusion.py:27-91).  `solver`: one instance PER target -- multistep solvers keep the previous data
    estimate, which two targets must not share.  `opacity_mask` (1 = opaque, 0 = no influence) and `weight` together give the target's
    share in the blend; the target takes part in steps `start_step <= step <= end_step`, starting from `init_latents` noised to
    `start_step` when they are given and from the canvas otherwise."""

    tile: Tile
    solver: Any
    init_latents: Tensor | None = None
    opacity_mask: Tensor | None = None
    weight: int = 1
    start_step: int = 0
    end_step: int = MAX_STEPS

    @property
    def size(self) -> Size:
        return Size(height=self.tile.bottom - self.tile.top, width=self.tile.right - self.tile.left)

    @property
    def offset(self) -> tuple[int, int]:
        return self.tile.top, self.tile.left

    def crop(self, tensor: Tensor, /) -> Tensor:
        height, width = self.size
        top, left = self.offset
        return tensor[:, :, top : top + height, left : left + width]

    def paste(self, tensor: Tensor, /, crop: Tensor) -> Tensor:
        height, width = self.size
        top, left = self.offset
        tensor[:, :, top : top + height, left : left + width] = crop
        return tensor


T = TypeVar("T", bound=DiffusionTarget)


class MultiDiffusion(ABC, Generic[T]):
    def __call__(self, x: Tensor, /, noise: Tensor, step: int, targets: Sequence[T]) -> Tensor:
        num_updates = torch.zeros_like(input=x)
        cumulative_values = torch.zeros_like(input=x)
        for target in targets:
            if step == target.start_step and target.init_latents is not None:
                view = target.solver.add_noise(x=target.init_latents, noise=target.crop(noise), step=step)
            elif target.start_step <= step <= target.end_step:
                view = target.crop(x)
            else:
                continue
            view = self.diffuse_target(x=view, step=step, target=target)
            weight = target.weight * target.opacity_mask if target.opacity_mask is not None else target.weight
            num_updates = target.paste(num_updates, crop=target.crop(num_updates) + weight)
            cumulative_values = target.paste(cumulative_values, crop=target.crop(cumulative_values) + weight * view)
        return torch.where(condition=num_updates > 0, input=cumulative_values / num_updates, other=x)

    @abstractmethod
    def diffuse_target(self, x: Tensor, step: int, target: T) -> Tensor: ...

    @staticmethod
    def generate_latent_tiles(size: Size, tile_size: Size, min_overlap: int = 8) -> list[Tile]:
        """Tiles of `tile_size` that cover `size` with at least `min_overlap` between neighbours; one tile for the whole image when the
        tile does not fit (multi_diffusion.py:126-175).  The last tile of a row / column is moved back inside the image."""
        assert 0 <= min_overlap < min(tile_size.height, tile_size.width), "Overlap must be non-negative and less than the tile size"
        if tile_size.width > size.width or tile_size.height > size.height:
            return [Tile(top=0, left=0, bottom=size.height, right=size.width)]

        def count_and_overlap(length: int, tile_length: int) -> tuple[int, int]:
            if tile_length >= length:
                return 1, 0
            num = math.ceil((length - tile_length) / (tile_length - min_overlap)) + 1
            return num, (num * tile_length - length) // (num - 1)

        nx, overlap_x = count_and_overlap(size.width, tile_size.width)
        ny, overlap_y = count_and_overlap(size.height, tile_size.height)
        tiles: list[Tile] = []
        for i in range(ny):
            for j in range(nx):
                x = min(j * (tile_size.width - overlap_x), size.width - tile_size.width)
                y = min(i * (tile_size.height - overlap_y), size.height - tile_size.height)
                tiles.append(Tile(top=y, left=x, bottom=y + tile_size.height, right=x + tile_size.width))
        return tiles


@dataclass(kw_only=True)
class SDXLTarget(DiffusionTarget):
    clip_text_embedding: Tensor
    condition_scale: float = 5.0
    pooled_text_embedding: Tensor
    time_ids: Tensor


class SDXLMultiDiffusion(MultiDiffusion[SDXLTarget]):
    """`sd`: anything called like refiners' StableDiffusion_XL (`SDXLDenoiser` here) with a `.solver` attribute."""

    def __init__(self, sd: Any) -> None:
        self.sd = sd

    def diffuse_target(self, x: Tensor, step: int, target: SDXLTarget) -> Tensor:
        old_solver = self.sd.solver
        self.sd.solver = target.solver
        result = self.sd(x, step=step, clip_text_embedding=target.clip_text_embedding, pooled_text_embedding=target.pooled_text_embedding,
                         time_ids=target.time_ids, condition_scale=target.condition_scale)
        self.sd.solver = old_solver
        return result


class SD1Denoiser(SDXLDenoiser):
    """The SD1.5 counterpart of `SDXLDenoiser` (reference stable_diffusion_1/model.py:90-97: the UNet context is the timestep and the text
    embedding alone)."""

    def set_unet_context(self, *, timestep: Tensor, clip_text_embedding: Tensor, **_: Any) -> None:  # type: ignore[override]
        self.unet.set_timestep(timestep=timestep)
        self.unet.set_clip_text_embedding(clip_text_embedding=clip_text_embedding)

    def __call__(self, x: Tensor, step: int, *, clip_text_embedding: Tensor, condition_scale: float = 7.5, **kwargs: Any) -> Tensor:  # type: ignore[override]
        assert self._find_sag_adapter() is None, "Self-Attention Guidance is mirrored for SDXL only"
        timestep = self.solver.timesteps[step].unsqueeze(dim=0)
        self.set_unet_context(timestep=timestep, clip_text_embedding=clip_text_embedding)
        latents = self.solver.scale_model_input(torch.cat((x, x)), step=step)
        uncond, cond = self.unet(latents).chunk(2)
        return self.solver(x, predicted_noise=uncond + condition_scale * (cond - uncond), step=step)


@dataclass(kw_only=True)
class SD1DiffusionTarget(DiffusionTarget):
    clip_text_embedding: Tensor
    condition_scale: float = 7.0


class SD1MultiDiffusion(MultiDiffusion[SD1DiffusionTarget]):
    def __init__(self, sd: Any) -> None:
        self.sd = sd

    def diffuse_target(self, x: Tensor, step: int, target: SD1DiffusionTarget) -> Tensor:
        old_solver = self.sd.solver
        self.sd.solver = target.solver
        result = self.sd(x, step=step, clip_text_embedding=target.clip_text_embedding, condition_scale=target.condition_scale)
        self.sd.solver = old_solver
        return result
