"""Preprocessors of conditioned pipelines (reference: foundationals/latent_diffusion/preprocessors/).

InformativeDrawings turns a picture into the line drawing the lineart ControlNet is conditioned on.  The tree, its `repr` and its state-dict
keys are the reference's (informative_drawings.py:8-107); refiners_amd.engine.lineart.CompiledInformativeDrawings runs it on the MI355X kernels.
"""
from __future__ import annotations

from typing import Any

from ..fluxion import layers as fl


class InformativeDrawings(fl.Chain):
    """"Learning to generate line drawings that convey geometry and semantics" (Chan, Durand, Isola, 2022; https://arxiv.org/abs/2203.12691;
    adapted from https://github.com/carolineec/informative-drawings, MIT License).  [B, in_channels, H, W] -> [B, out_channels, H', W'] in (0, 1)
    with H' = 4 ceil(ceil(H / 2) / 2): two stride-2 convolutions down, `n_residual_blocks` reflect-padded residual blocks, two transposed
    convolutions up; every convolution but the last is followed by InstanceNorm2d and ReLU."""

    def __init__(self, in_channels: int = 3, out_channels: int = 1, n_residual_blocks: int = 3, device: Any = None, dtype: Any = None) -> None:
        super().__init__(
            fl.Chain(  # initial convolution
                fl.ReflectionPad2d(3),
                fl.Conv2d(in_channels=in_channels, out_channels=64, kernel_size=7, device=device, dtype=dtype),
                fl.InstanceNorm2d(64, device=device, dtype=dtype),
                fl.ReLU(),
            ),
            *(  # downsampling
                fl.Chain(
                    fl.Conv2d(in_channels=64 * (2**i), out_channels=128 * (2**i), kernel_size=3, stride=2, padding=1, device=device, dtype=dtype),
                    fl.InstanceNorm2d(128 * (2**i), device=device, dtype=dtype),
                    fl.ReLU(),
                )
                for i in range(2)
            ),
            *(  # residual blocks
                fl.Residual(
                    fl.ReflectionPad2d(1),
                    fl.Conv2d(in_channels=256, out_channels=256, kernel_size=3, device=device, dtype=dtype),
                    fl.InstanceNorm2d(256, device=device, dtype=dtype),
                    fl.ReLU(),
                    fl.ReflectionPad2d(1),
                    fl.Conv2d(in_channels=256, out_channels=256, kernel_size=3, device=device, dtype=dtype),
                    fl.InstanceNorm2d(256, device=device, dtype=dtype),
                )
                for _ in range(n_residual_blocks)
            ),
            *(  # upsampling
                fl.Chain(
                    fl.ConvTranspose2d(in_channels=128 * (2**i), out_channels=64 * (2**i), kernel_size=3, stride=2, padding=1, output_padding=1, device=device, dtype=dtype),
                    fl.InstanceNorm2d(64 * (2**i), device=device, dtype=dtype),
                    fl.ReLU(),
                )
                for i in reversed(range(2))
            ),
            fl.Chain(  # output layer
                fl.ReflectionPad2d(3),
                fl.Conv2d(in_channels=64, out_channels=out_channels, kernel_size=7, device=device, dtype=dtype),
                fl.Sigmoid(),
            ),
        )
