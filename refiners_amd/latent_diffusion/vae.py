"""Latent-diffusion autoencoder as Chain trees (the step right after the sampling loop).

Mirrors reference src/refiners/foundationals/latent_diffusion/auto_encoder.py:83-330 (Resnet, Encoder, Decoder,
LatentDiffusionAutoencoder.encode / decode) and stable_diffusion_xl/model.py:12-19 (SDXLAutoencoder.encoder_scale);
same child order and class names, hence the same state-dict keys (tests/golden/vae_keys.json).  Tensor in, tensor out.
Tiled inference (auto_encoder.py:209-621) is mirrored too: FixedGroupNorm, _create_blending_mask, _generate_latent_tiles,
the tiled_inference context manager and _tiled_encode / _tiled_decode; PIL is imported only inside the methods that take or
return a PIL image.  These forwards are the unfused torch path; refiners_amd.engine.vae.CompiledVAEDecoder lowers the Decoder
tree onto the MI355X kernels and refiners_amd.engine.tiled_vae.CompiledTiledVAE the tiled encode / decode.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Any
from typing import Iterator, NamedTuple

import torch
import torch.nn.functional as F
from torch import Tensor

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.adapt import Adapter
from refiners_amd.fluxion.leaves import Slicing
from refiners_amd.fluxion.tree import Contexts

_WIDTHS = [128, 256, 512, 512, 512]


class Resnet(fl.Sum):
    """Sum( shortcut (1x1 conv iff channels change) , GN -> SiLU -> conv3x3 -> GN -> SiLU -> conv3x3 )."""

    def __init__(self, in_channels: int, out_channels: int, num_groups: int = 32, device: Any = None, dtype: Any = None):
        self.in_channels = in_channels
        self.out_channels = out_channels
        kw = dict(device=device, dtype=dtype)
        shortcut = fl.Conv2d(in_channels, out_channels, kernel_size=1, **kw) if in_channels != out_channels else fl.Identity()
        super().__init__(
            shortcut,
            fl.Chain(
                fl.GroupNorm(channels=in_channels, num_groups=num_groups, **kw),
                fl.SiLU(),
                fl.Conv2d(in_channels, out_channels, kernel_size=3, padding=1, **kw),
                fl.GroupNorm(channels=out_channels, num_groups=num_groups, **kw),
                fl.SiLU(),
                fl.Conv2d(out_channels, out_channels, kernel_size=3, padding=1, **kw),
            ),
        )


def _attention(channels: int, kw: dict[str, Any]) -> fl.Residual:
    return fl.Residual(fl.GroupNorm(channels=channels, num_groups=32, eps=1e-6, **kw), fl.SelfAttention2d(channels=channels, **kw))


class Encoder(fl.Chain):
    def __init__(self, device: Any = None, dtype: Any = None) -> None:
        kw = dict(device=device, dtype=dtype)
        w = _WIDTHS
        stages = [fl.Chain([Resnet(w[i - 1] if i > 0 else w[0], w[i], **kw), Resnet(w[i], w[i], **kw)]) for i in range(len(w))]
        for stage in stages[:3]:
            stage.append(fl.Downsample(channels=stage[-1].out_channels, scale_factor=2, **kw))
        stages[-1].insert_after_type(Resnet, _attention(w[-1], kw))
        super().__init__(
            fl.Conv2d(3, w[0], kernel_size=3, padding=1, **kw),
            fl.Chain(*stages),
            fl.Chain(fl.GroupNorm(channels=w[-1], num_groups=32, eps=1e-6, **kw), fl.SiLU(), fl.Conv2d(w[-1], 8, kernel_size=3, padding=1, **kw)),
            fl.Chain(fl.Conv2d(8, 8, kernel_size=1, **kw), Slicing(dim=1, end=4)),
        )

    def init_context(self) -> Contexts:
        return {"sampling": {"shapes": []}}


class Decoder(fl.Chain):
    def __init__(self, device: Any = None, dtype: Any = None) -> None:
        self.resnet_sizes: list[int] = list(_WIDTHS)
        self.latent_dim: int = 4
        self.output_channels: int = 3
        kw = dict(device=device, dtype=dtype)
        w = _WIDTHS[::-1]
        stages = []
        for i in range(len(w)):
            blocks = [Resnet(w[i - 1] if i > 0 else w[0], w[i], **kw), Resnet(w[i], w[i], **kw)]
            if i > 0:
                blocks.append(Resnet(w[i], w[i], **kw))
            stages.append(fl.Chain(blocks))
        stages[0].insert(1, _attention(w[0], kw))
        for stage in stages[1:4]:
            stage.insert(-1, fl.Upsample(channels=stage.layer(-1, Resnet).out_channels, upsample_factor=2, **kw))
        super().__init__(
            fl.Conv2d(self.latent_dim, self.latent_dim, kernel_size=1, **kw),
            fl.Conv2d(self.latent_dim, w[0], kernel_size=3, padding=1, **kw),
            fl.Chain(*stages),
            fl.Chain(fl.GroupNorm(channels=w[-1], num_groups=32, eps=1e-6, **kw), fl.SiLU(), fl.Conv2d(w[-1], self.output_channels, kernel_size=3, padding=1, **kw)),
        )


class _ImageSize(NamedTuple):
    height: int
    width: int


class _Tile(NamedTuple):
    top: int
    left: int
    bottom: int
    right: int


class FixedGroupNorm(fl.Chain, Adapter[fl.GroupNorm]):
    """A GroupNorm whose statistics are frozen by its first forward (auto_encoder.py:209-251), so that every tile of a tiled encode / decode is
    normalised like the downscaled whole image was.  `mean` / `var`: one value per group (biased variance), None until the first call."""

    mean: Tensor | None
    var: Tensor | None

    def __init__(self, target: fl.GroupNorm) -> None:
        self.mean = None
        self.var = None
        with self.setup_adapter(target):
            super().__init__(fl.Lambda(self.compute_group_norm))

    def compute_group_norm(self, x: Tensor) -> Tensor:
        gn = self.target
        b, c, h, w = x.shape
        # groups become batch-norm channels: batch_norm(training=False) then normalises each with the stored statistics
        grouped = x.reshape(1, b * gn.num_groups, c // gn.num_groups, h, w)
        if self.mean is None or self.var is None:
            self.var, self.mean = torch.var_mean(grouped, dim=(0, 2, 3, 4), correction=0)
        y = F.batch_norm(grouped, self.mean, self.var, weight=None, bias=None, training=False, momentum=0, eps=gn.eps).reshape(b, c, h, w)
        return y * gn.weight.reshape(1, -1, 1, 1) + gn.bias.reshape(1, -1, 1, 1)


def _create_blending_mask(size: _ImageSize, blending: int, num_channels: int, device: Any = None, dtype: Any = None,
                          is_edge: tuple[bool, bool, bool, bool] = (False, False, False, False)) -> Tensor:
    """Ones with a linear ramp of `blending` positions (at most half the shorter side) towards every side that is not on the canvas edge;
    is_edge = (top, bottom, left, right).  (auto_encoder.py:254-279)"""
    mask = torch.ones(size, device=device, dtype=dtype)
    if blending == 0:
        return mask
    blending = min(blending, min(size) // 2)
    ramp = torch.linspace(0, 1, steps=blending, device=device, dtype=dtype)
    top, bottom, left, right = is_edge
    if not top:
        mask[:blending, :] *= ramp.view(-1, 1)
    if not bottom:
        mask[-blending:, :] *= ramp.flip(0).view(-1, 1)
    if not left:
        mask[:, :blending] *= ramp.view(1, -1)
    if not right:
        mask[:, -blending:] *= ramp.flip(0).view(1, -1)
    return mask.unsqueeze(0).unsqueeze(0).expand(1, num_channels, *size)


def _pil_to_tensor(image: Any, device: Any, dtype: Any) -> Tensor:
    """PIL image -> (1, channels, H, W) in [0, 1] (fluxion/utils.py image_to_tensor)."""
    import numpy as np

    t = torch.tensor(np.array(image).astype(np.float32) / 255.0, device=device, dtype=dtype)
    if image.mode == "L":
        return t[None, None]
    if image.mode not in ("RGB", "RGBA"):
        raise ValueError(f"Unsupported image mode: {image.mode}")
    return t.permute(2, 0, 1)[None]


def _tensor_to_pil(t: Tensor) -> Any:
    """(1, 1 | 3 | 4, H, W) in [0, 1] (clamped) -> PIL image (fluxion/utils.py tensor_to_image)."""
    from PIL import Image

    assert t.ndim == 4 and t.shape[0] == 1 and t.shape[1] in (1, 3, 4), f"Unsupported tensor shape: {t.shape}"
    t = t[0].clamp(0, 1).to(torch.float32)
    t = t[0] if t.shape[0] == 1 else t.permute(1, 2, 0)
    return Image.fromarray((t.cpu().numpy() * 255).astype("uint8"))


class LatentDiffusionAutoencoder(fl.Chain):
    encoder_scale = 0.18125
    _tile_size: _ImageSize | None = None  # set while `tiled_inference` is active
    _blending: int | None = None

    def __init__(self, device: Any = None, dtype: Any = None) -> None:
        super().__init__(Encoder(device=device, dtype=dtype), Decoder(device=device, dtype=dtype))

    def encode(self, x: Tensor) -> Tensor:
        return self.encoder_scale * self[0](x)

    def decode(self, x: Tensor) -> Tensor:
        return self[1](x / self.encoder_scale)

    # -- tiled inference (auto_encoder.py:341-357, 381-396, 411-621) -------------------------------------------------------------------------
    _NOT_ACTIVE = "Tiled inference context manager not active. Use `tiled_inference` method to activate."

    def tiled_image_to_latents(self, image: Any) -> Tensor:
        """PIL image -> latents, tile by tile with blended seams; inside `with vae.tiled_inference(image):` only."""
        if self._tile_size is None or self._blending is None:
            raise ValueError(self._NOT_ACTIVE)
        x = _pil_to_tensor(image, self.device, self.dtype)
        return self._tiled_encode(2 * x - 1, self._tile_size, self._blending)

    def tiled_latents_to_image(self, x: Tensor) -> Any:
        """latents -> PIL image, tile by tile with blended seams; inside `with vae.tiled_inference(image):` only."""
        if self._tile_size is None or self._blending is None:
            raise ValueError(self._NOT_ACTIVE)
        return _tensor_to_pil((self._tiled_decode(x, self._tile_size, self._blending) + 1) / 2)

    @staticmethod
    def _generate_latent_tiles(size: _ImageSize, tile_size: _ImageSize, overlap: int = 8) -> list[_Tile]:
        """A grid: one independent run of starts per axis, x outer and y inner, tiles clipped to the latent size."""
        return [
            _Tile(top=max(0, y), left=max(0, x), bottom=min(size.height, y + tile_size.height), right=min(size.width, x + tile_size.width))
            for x in range(0, max(size.width - overlap, 1), tile_size.width - overlap)
            for y in range(0, max(size.height - overlap, 1), tile_size.height - overlap)
        ]

    @torch.no_grad()
    def _add_fixed_group_norm(self, image: Any, inference_size: _ImageSize) -> None:
        """Every GroupNorm becomes a FixedGroupNorm; one encode + decode of the image downscaled to `inference_size` (its colour statistics
        matched to the full image's) sets their statistics."""
        for gn, parent in self.walk(fl.GroupNorm):
            FixedGroupNorm(gn).inject(parent)
        small = image.resize((inference_size.width, inference_size.height))
        full_t = _pil_to_tensor(image, self.device, self.dtype)
        small_t = _pil_to_tensor(small, self.device, self.dtype)
        small_t.clamp_(min=full_t.min(), max=full_t.max())
        std, mean = torch.std_mean(full_t, dim=[0, 2, 3], keepdim=True)
        small_std, small_mean = torch.std_mean(small_t, dim=[0, 2, 3], keepdim=True)
        small_t = (small_t - small_mean) * (std / small_std) + mean
        self.decode(self.encode(2 * small_t - 1))

    def _remove_fixed_group_norm(self) -> None:
        for fixed in list(self.layers(FixedGroupNorm)):
            fixed.eject()

    def _tile_edges(self, tile: _Tile, size: _ImageSize) -> tuple[bool, bool, bool, bool]:
        return (tile.top == 0, tile.bottom == size.height, tile.left == 0, tile.right == size.width)

    @torch.no_grad()
    def _tiled_encode(self, image_tensor: Tensor, tile_size: _ImageSize, blending: int = 64) -> Tensor:
        """(1, 3, 8h, 8w) in [-1, 1] -> latents (1, 4, h, w): every tile encoded on its own, summed under its ramp mask, divided by the summed masks."""
        size = _ImageSize(height=image_tensor.shape[2] // 8, width=image_tensor.shape[3] // 8)
        tiles = self._generate_latent_tiles(size, _ImageSize(height=tile_size.height // 8, width=tile_size.width // 8), overlap=blending // 8)
        if len(tiles) == 1:
            return self.encode(image_tensor)
        result = torch.zeros((1, 4, *size), device=self.device, dtype=self.dtype)
        weights = torch.zeros_like(result)
        for t in tiles:
            enc = self.encode(image_tensor[:, :, t.top * 8 : t.bottom * 8, t.left * 8 : t.right * 8])
            mask = _create_blending_mask(_ImageSize(t.bottom - t.top, t.right - t.left), blending // 8, 4, self.device, self.dtype, self._tile_edges(t, size))
            result[:, :, t.top : t.bottom, t.left : t.right] += enc * mask
            weights[:, :, t.top : t.bottom, t.left : t.right] += mask
        return result / weights

    @torch.no_grad()
    def _tiled_decode(self, latents: Tensor, tile_size: _ImageSize, blending: int = 64) -> Tensor:
        """latents (1, 4, h, w) -> (1, 3, 8h, 8w): every latent tile decoded on its own and blended in pixel space."""
        size = _ImageSize(height=latents.shape[2], width=latents.shape[3])
        tiles = self._generate_latent_tiles(size, _ImageSize(height=tile_size.height // 8, width=tile_size.width // 8), overlap=blending // 8)
        if len(tiles) == 1:
            return self.decode(latents)
        result = torch.zeros((1, 3, size.height * 8, size.width * 8), device=self.device, dtype=self.dtype)
        weights = torch.zeros_like(result)
        for t in tiles:
            dec = self.decode(latents[:, :, t.top : t.bottom, t.left : t.right])
            mask = _create_blending_mask(_ImageSize((t.bottom - t.top) * 8, (t.right - t.left) * 8), blending, 3, self.device, self.dtype, self._tile_edges(t, size))
            result[:, :, t.top * 8 : t.bottom * 8, t.left * 8 : t.right * 8] += dec * mask
            weights[:, :, t.top * 8 : t.bottom * 8, t.left * 8 : t.right * 8] += mask
        return result / weights

    @contextmanager
    def tiled_inference(self, image: Any, tile_size: tuple[int, int] = (512, 512), blending: int = 64) -> Iterator[None]:
        """`with vae.tiled_inference(image, tile_size=(width, height), blending=...):` freezes the GroupNorm statistics on a downscaled copy of
        `image` for the tiled calls inside, and restores the plain GroupNorms on exit.  The untiled encode / decode inside the context run
        with the frozen statistics and no tiling."""
        try:
            self._blending = blending
            self._tile_size = _ImageSize(width=tile_size[0], height=tile_size[1])
            self._add_fixed_group_norm(image, inference_size=self._tile_size)
            yield
        finally:
            self._remove_fixed_group_norm()
            self._tile_size = None
            self._blending = None


class SDXLAutoencoder(LatentDiffusionAutoencoder):
    encoder_scale: float = 0.13025
