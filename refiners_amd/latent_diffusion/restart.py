"""Restart sampling (reference latent_diffusion/restart.py, arXiv:2306.14878): after a DDIM trajectory, re-noise the latents from the
interval's last timestep back to its first and run the DDIM segment again, `num_iterations` times.

* `add_noise_interval`  restart.py:13-26
* `Restart`             restart.py:29-109, over the mirror's `SDXLDenoiser`

This file is the unfused torch path; `refiners_amd.engine.compiled.CompiledSDXL.restart` runs the same iterations on the resident latents.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import cached_property
from typing import Any

import torch
from torch import Tensor

from .sampling import DDIM


def add_noise_interval(solver: Any, /, x: Tensor, noise: Tensor, initial_timestep: Tensor, target_timestep: Tensor) -> Tensor:
    """Noise x, which sits at `initial_timestep`, up to `target_timestep`: factor = scale[target] / scale[initial]."""
    factor = solver.cumulative_scale_factors[target_timestep] / solver.cumulative_scale_factors[initial_timestep]
    return factor * x + torch.sqrt(1 - factor ** 2) * noise


@dataclass
class Restart:
    """Works only with the DDIM solver, as the reference's."""

    ldm: Any
    num_steps: int = 10
    num_iterations: int = 2
    start_time: float = 0.1
    end_time: float = 2

    def __post_init__(self) -> None:
        assert isinstance(self.ldm.solver, DDIM), "Restart sampling only works with DDIM solver"

    def __call__(self, x: Tensor, /, clip_text_embedding: Tensor, condition_scale: float = 7.5, generator: torch.Generator | None = None,
                 **kwargs: Tensor) -> Tensor:
        """`generator` is this mirror's one extension: None draws from the global stream, as the reference's randn_like does."""
        original_solver = self.ldm.solver
        new_solver = DDIM(self.ldm.solver.num_inference_steps, device=self.device, dtype=self.dtype)
        new_solver.timesteps = self.timesteps
        self.ldm.solver = new_solver
        try:
            for _ in range(self.num_iterations):
                noise = torch.randn(x.shape, generator=generator, device=self.device if generator is None else generator.device, dtype=self.dtype)
                x = add_noise_interval(new_solver, x=x, noise=noise.to(x.device), initial_timestep=self.timesteps[-1], target_timestep=self.timesteps[0])
                for step in range(len(self.timesteps) - 1):
                    x = self.ldm(x, step=step, clip_text_embedding=clip_text_embedding, condition_scale=condition_scale, **kwargs)
        finally:
            self.ldm.solver = original_solver
        return x

    @cached_property
    def start_step(self) -> int:
        sigmas = self.ldm.solver.noise_std / self.ldm.solver.cumulative_scale_factors
        return int(torch.argmin(torch.abs(sigmas[self.ldm.solver.timesteps] - self.start_time)))

    @cached_property
    def end_timestep(self) -> int:
        sigmas = self.ldm.solver.noise_std / self.ldm.solver.cumulative_scale_factors
        return int(torch.argmin(torch.abs(sigmas - self.end_time)))

    @cached_property
    def timesteps(self) -> Tensor:
        return (torch.round(torch.linspace(start=int(self.ldm.solver.timesteps[self.start_step]), end=self.end_timestep, steps=self.num_steps))
                .flip(0).to(device=self.device, dtype=torch.int64))

    @property
    def device(self) -> torch.device:
        return self.ldm.device

    @property
    def dtype(self) -> torch.dtype:
        return self.ldm.dtype
