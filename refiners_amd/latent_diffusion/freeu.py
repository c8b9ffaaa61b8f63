"""Host-side mirror of refiners' FreeU adapter (`foundationals/latent_diffusion/freeu.py`; Si et al., "FreeU: Free Lunch in Diffusion U-Net",
arXiv 2309.11497): in the first up blocks the ResidualConcatenator is replaced by one that scales the first half of the backbone channels and
damps the lowest frequencies of the skip features.  Class names, constructor arguments, child order and context reads follow the reference
(`repr` / inject / eject identical).  On the MI355X the concatenator is one launch, mi355x_freeu_filter, when REFINERS_AMD_FREEU=1
(engine/unet_lowering.py, engine/freeu.py); the forward below is the stock one, on torch.fft.
"""
import math
from typing import Any, Callable

import torch
from torch import Tensor

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.adapters import Adapter
from refiners_amd.fluxion.tree import bump_epoch

from .blocks import ResidualConcatenator


def fourier_filter(x: Tensor, scale: float = 1, threshold: int = 1) -> Tensor:
    """x [B, C, H, W] with the frequencies {-threshold .. threshold - 1} x {-threshold .. threshold - 1} of every plane multiplied by `scale`:

        out = Re( ifft2( ifftshift( mask * fftshift( fft2(x) ) ) ) ),   mask = scale on rows and columns n // 2 - threshold .. n // 2 + threshold - 1, else 1

    A half-precision input is transformed in float32 when torch.fft cannot take it as it is (a size that is no power of two, bfloat16)."""
    height, width = x.shape[-2:]
    dtype = x.dtype
    pow2 = math.log2(height).is_integer() and math.log2(width).is_integer()
    if dtype == torch.bfloat16 or (dtype == torch.float16 and not pow2):
        x = x.to(dtype=torch.float32)
    freq = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape, device=x.device, dtype=x.dtype)
    rc, cc = height // 2, width // 2
    mask[..., rc - threshold : rc + threshold, cc - threshold : cc + threshold] = scale
    out = torch.fft.ifftn(torch.fft.ifftshift(freq * mask, dim=(-2, -1)), dim=(-2, -1)).real
    return out.to(dtype=dtype)


class FreeUBackboneFeatures(fl.Module):
    """x[:, : C // 2] *= backbone_scale, in place."""

    def __init__(self, backbone_scale: float) -> None:
        super().__init__()
        self.backbone_scale = backbone_scale

    def __setattr__(self, name: str, value: Any) -> None:
        if name == "backbone_scale":
            bump_epoch()  # (baked into the lowered launch)
        super().__setattr__(name, value)

    def forward(self, x: Tensor) -> Tensor:
        half = x.shape[1] // 2
        x[:, :half] = x[:, :half] * self.backbone_scale
        return x


class FreeUSkipFeatures(fl.Chain):
    """fourier_filter(residuals[n], skip_scale)."""

    def __init__(self, n: int, skip_scale: float) -> None:
        apply_filter: Callable[[Tensor], Tensor] = lambda x: fourier_filter(x, scale=skip_scale)  # noqa: E731
        super().__init__(
            fl.UseContext(context="unet", key="residuals").compose(lambda residuals: residuals[n]),
            fl.Lambda(apply_filter),
        )


class FreeUResidualConcatenator(fl.Concatenate):
    def __init__(self, n: int, backbone_scale: float, skip_scale: float) -> None:
        super().__init__(FreeUBackboneFeatures(backbone_scale), FreeUSkipFeatures(n, skip_scale), dim=1)


class SDFreeUAdapter(fl.Chain, Adapter[fl.Chain]):
    """FreeU on the first len(backbone_scales) up blocks of an SD1UNet / SDXLUNet."""

    def __init__(self, target: fl.Chain, backbone_scales: list[float], skip_scales: list[float]) -> None:
        assert len(backbone_scales) == len(skip_scales)
        assert len(backbone_scales) <= len(target.layer("UpBlocks", fl.Chain))
        self.backbone_scales = backbone_scales
        self.skip_scales = skip_scales
        with self.setup_adapter(target):
            super().__init__(target)

    def inject(self, parent: "fl.Chain | None" = None) -> "SDFreeUAdapter":
        for n, (backbone_scale, skip_scale) in enumerate(zip(self.backbone_scales, self.skip_scales)):
            block = self.target.layer(("UpBlocks", n), fl.Chain)
            block.replace(block.ensure_find(ResidualConcatenator), FreeUResidualConcatenator(-n - 2, backbone_scale, skip_scale))
        return super().inject(parent)

    def eject(self) -> None:
        for n in range(len(self.backbone_scales)):
            block = self.target.layer(("UpBlocks", n), fl.Chain)
            block.replace(block.ensure_find(FreeUResidualConcatenator), ResidualConcatenator(-n - 2))
        super().eject()
