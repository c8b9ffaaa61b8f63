"""Cases of the tiled VAE fixtures (tools/make_golden_tiled_vae.py writes them, tests/test_tiled_vae_*.py read them).  The tile is 64 x 64 pixels (8 x 8
latents), the smallest at which the SDXL autoencoder's three downsamplings still leave a grid to blend:
    a  blending 16, latents 20 wide x 13 high: 3 x 2 tiles of two sizes (8 x 8 and 8 wide x 7 high), non-square, latent width not a multiple of 4
    b  blending 32, latents 14 x 14: 3 x 3 tiles, the overlap of 4 is half the tile, the last tiles are 6 wide so their ramp shortens to 3 latents
    d  blending 16, latents 8 wide x 6 high: ONE tile -- frozen statistics, no blend
GEOMETRY_C is kernel-only (no autoencoder runs): blending 40 gives overlap 5 and stride 3, an element is covered by up to 3 x 3 tiles, 9 x 8 = 72 tiles."""
from __future__ import annotations

import torch

from refiners_amd import synth

TILE = (64, 64)  # (width, height) in pixels, as tiled_inference takes it
WEIGHT_SEED = 0
LATENT_STD = 0.13  # of the latents given to _tiled_decode (VAE_CASE's)
TILED_VAE_CASES = {
    "a": dict(blending=16, latent_wh=(20, 13), grid=(3, 2), seed=31),
    "b": dict(blending=32, latent_wh=(14, 14), grid=(3, 3), seed=32),
    "d": dict(blending=16, latent_wh=(8, 6), grid=(1, 1), seed=33),
}
GEOMETRY_C = dict(blending=40, latent_wh=(31, 29), grid=(9, 8))


def case_image_u8(case: dict) -> torch.Tensor:
    """The case's RGB image as uint8 (H, W, 3): smooth colour gradients plus noise, so that the downscaled calibration image keeps some structure."""
    w, h = (8 * v for v in case["latent_wh"])
    g = synth._gen("tiled_vae.image", case["seed"])
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    base = torch.stack((xx, yy, 1 - 0.5 * (xx + yy)), dim=-1)
    return ((0.7 * base + 0.3 * torch.rand((h, w, 3), generator=g)) * 255).round().clamp(0, 255).to(torch.uint8)


def image_tensor(u8: torch.Tensor) -> torch.Tensor:
    """uint8 (H, W, 3) -> what tiled_image_to_latents hands to _tiled_encode: (1, 3, H, W) float32 in [-1, 1]."""
    return 2 * (u8.to(torch.float32) / 255.0).permute(2, 0, 1)[None] - 1


def case_latents(case: dict) -> torch.Tensor:
    """The latents given to _tiled_decode."""
    w, h = case["latent_wh"]
    return torch.randn((1, 4, h, w), generator=synth._gen("tiled_vae.latents", case["seed"])) * LATENT_STD
