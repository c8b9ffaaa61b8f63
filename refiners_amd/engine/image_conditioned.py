"""The conditions of an inpainting run on the device: `StableDiffusion_1_Inpainting.set_inpainting_conditions` (reference
stable_diffusion_1/model.py:259-286) as ONE kernel (mi355x_inpaint_conditions: uint8 picture and mask -> masked picture in [-1, 1] and the
nearest-resampled binary mask) in front of the lowered VAE encoder, whose input buffer is the kernel's output.

    cond = CompiledInpaintConditions(lda)
    mask_latents, target_image_latents = cond(picture, mask, latents_size=(64, 64))
    sd.set_inputs(x, clip_text_embedding=e, input_condition=torch.cat((mask_latents, target_image_latents), dim=1))
"""
from __future__ import annotations

from typing import Any

import torch
from torch import Tensor

from .. import native
from .vae import CompiledVAEEncoder


def _as_uint8(image: Any, mode: str, device: torch.device) -> Tensor:
    """A PIL image (converted to `mode` as the reference converts it) or a uint8 tensor ([H, W, 3] / [n, H, W, 3] for RGB, [H, W] / [n, H, W] for L)."""
    if not torch.is_tensor(image):
        import numpy as np

        image = torch.from_numpy(np.array(image.convert(mode=mode)))
    assert image.dtype == torch.uint8, f"pictures are uint8 (PIL images or numpy.array(pil_image)), not {image.dtype}"
    if image.dim() == (3 if mode == "RGB" else 2):
        image = image[None]
    return image.to(device).contiguous()


class CompiledInpaintConditions:
    """`mask_latents, target_image_latents = CompiledInpaintConditions(lda)(target_image, mask, latents_size)`; lda: LatentDiffusionAutoencoder-like Chain."""

    def __init__(self, lda: Any) -> None:
        native.load()
        self.lda = lda
        self.encoder = CompiledVAEEncoder(lda)

    @torch.no_grad()
    def __call__(self, target_image: Any, mask: Any, latents_size: tuple[int, int] = (64, 64)) -> tuple[Tensor, Tensor]:
        device, dtype = self.lda.device, self.lda.dtype
        image = _as_uint8(target_image, "RGB", device)
        m = _as_uint8(mask, "L", device)
        n, H, W, _ = image.shape
        assert m.shape[0] in (1, n) and tuple(m.shape[1:]) == (H, W), f"the mask is {tuple(m.shape)}, the picture {tuple(image.shape)}"
        masked = self.encoder.prepare((n, 3, H, W), device)  # the encoder's own input buffer: the kernel writes it, nothing is copied
        mask_latents = torch.empty((m.shape[0], 1) + tuple(latents_size), device=device, dtype=dtype)
        native.inpaint_conditions(image, m, masked, mask_latents)
        return mask_latents, self.encoder.run()
