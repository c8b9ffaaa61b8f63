"""DINOv2 (arXiv:2304.07193; registers: arXiv:2309.16588) as a Chain tree: the ViT encoder behind feature extraction and the FID metric.

Mirrors reference src/refiners/foundationals/dinov2/{vit,dinov2}.py (same class names, child order and parameter names, hence the
same state-dict keys -- checked against tests/golden/dinov2_keys.json).  Everything here is the unfused torch path, which is also the
CPU path and the fallback of the MI355X engine (refiners_amd/engine/dinov2.py lowers the same tree).

Shapes: (B, 3, H, W), any H, W >= patch size -> a strided patch convolution WITH bias -> (B, n, D) tokens, n = (H // p) (W // p), behind a
class token -> + the learned position table, whose patch part (a square grid of image_size // p cells) is resampled to the input's grid on
every call (bicubic; antialiased in the register variants) -> the register tokens, spliced in between the class token and the
patches AFTER the position add -> `num_layers` pre-norm transformer layers with a LayerScale on both residual branches (GELU MLP, or
SwiGLU = GLU(SiLU()) in the giant model) -> LayerNorm.  The forward returns (B, 1 + num_registers + n, D).

Two facts of the reference that the lowering has to honour as well:
  * InterpolateEmbedding names the input's dimensions 2 and 3 "W" and "H" and asks for size (dim2 // p, dim3 // p): the resampled grid is
    (H // p) rows by (W // p) columns in the usual naming, the same grid the convolution produces, row-major;
  * the table is resampled in float32 and cast back to the tokens' dtype before the add.
"""
from math import sqrt
from typing import Any

import torch
from torch import Tensor

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.leaves import interpolate
from refiners_amd.fluxion.tree import Contexts


class ClassToken(fl.Chain):
    """The learned class token, one row per image."""

    def __init__(self, embedding_dim: int, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        super().__init__(fl.Parameter(1, embedding_dim, device=device, dtype=dtype))


class PositionalEmbedding(fl.Chain):
    """The learned position table: row 0 for the class token, then a square grid of patch positions."""

    def __init__(self, sequence_length: int, embedding_dim: int, patch_size: int, device: Any = None, dtype: Any = None) -> None:
        self.sequence_length = sequence_length
        self.embedding_dim = embedding_dim
        self.patch_size = patch_size
        super().__init__(fl.Parameter(sequence_length, embedding_dim, device=device, dtype=dtype))


class InterpolateEmbedding(fl.Module):
    """Resamples the patch part of the position table to the grid of the input image (x: the table, input: the image)."""

    def __init__(self, mode: str, antialias: bool, patch_size: int) -> None:
        super().__init__()
        self.mode = mode
        self.antialias = antialias
        self.patch_size = patch_size

    def forward(self, x: Tensor, input: Tensor) -> Tensor:
        cls_embed, patch_embed = x[:, :1, :], x[:, 1:, :]
        b, n, d = patch_embed.shape
        m = int(sqrt(n))
        assert m * m == n, "The sequence length must be a square number."
        rows, cols = input.shape[2] // self.patch_size, input.shape[3] // self.patch_size
        grid = patch_embed.reshape(b, m, m, d).permute(0, 3, 1, 2)
        grid = interpolate(grid.to(dtype=torch.float32), torch.Size((rows, cols)), mode=self.mode, antialias=self.antialias).to(dtype=cls_embed.dtype)
        return torch.cat((cls_embed, grid.permute(0, 2, 3, 1).reshape(b, -1, d)), dim=1)


class LayerScale(fl.WeightedModule):
    """x * weight, a learned per-channel scale of a residual branch."""

    def __init__(self, embedding_dim: int, init_value: float = 1.0, dtype: Any = None, device: Any = None) -> None:
        super().__init__()
        self.embedding_dim = embedding_dim
        self.register_parameter("weight", torch.nn.Parameter(torch.full((embedding_dim,), init_value, dtype=dtype, device=device)))

    def forward(self, x: Tensor) -> Tensor:
        return x * self.weight


class FeedForward(fl.Chain):
    """Linear, activation, Linear; a GLU activation halves the first Linear's output."""

    def __init__(self, embedding_dim: int, feedforward_dim: int, activation: fl.Activation, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.feedforward_dim = feedforward_dim
        pre = feedforward_dim * 2 if isinstance(activation, fl.GLU) else feedforward_dim
        super().__init__(
            fl.Linear(embedding_dim, pre, device=device, dtype=dtype),
            activation,
            fl.Linear(feedforward_dim, embedding_dim, device=device, dtype=dtype),
        )


class PatchEncoder(fl.Chain):
    """(B, C, H, W) -> (B, (H // p) (W // p), D): the strided convolution; the image itself is kept for InterpolateEmbedding."""

    def __init__(self, in_channels: int, out_channels: int, patch_size: int, device: Any = None, dtype: Any = None) -> None:
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.patch_size = patch_size
        super().__init__(
            fl.SetContext(context="dinov2_vit", key="input"),
            fl.Conv2d(in_channels, out_channels, kernel_size=patch_size, stride=patch_size, device=device, dtype=dtype),
            fl.Reshape(out_channels, -1),
            fl.Transpose(1, 2),
        )


class TransformerLayer(fl.Chain):
    """x + LayerScale(SelfAttention(LayerNorm(x))), then x + LayerScale(FeedForward(LayerNorm(x)))."""

    def __init__(self, embedding_dim: int, num_heads: int, norm_eps: float, mlp_ratio: int, activation: fl.Activation,
                 feedforward_dim: int | None = None, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        self.norm_eps = norm_eps
        self.mlp_ratio = mlp_ratio
        self.feedforward_dim = feedforward_dim if feedforward_dim is not None else embedding_dim * mlp_ratio
        super().__init__(
            fl.Residual(
                fl.LayerNorm(embedding_dim, eps=norm_eps, device=device, dtype=dtype),
                fl.SelfAttention(embedding_dim=embedding_dim, num_heads=num_heads, device=device, dtype=dtype),
                LayerScale(embedding_dim, device=device, dtype=dtype),
            ),
            fl.Residual(
                fl.LayerNorm(embedding_dim, eps=norm_eps, device=device, dtype=dtype),
                FeedForward(embedding_dim, self.feedforward_dim, activation, device=device, dtype=dtype),
                LayerScale(embedding_dim, device=device, dtype=dtype),
            ),
        )


class Transformer(fl.Chain):
    """A Chain of TransformerLayer."""


class PositionalEncoder(fl.Residual):
    """x + positions."""


class Registers(fl.Concatenate):
    """(class token, registers, patches): the register tokens go in behind the class token."""

    def __init__(self, num_registers: int, embedding_dim: int, device: Any = None, dtype: Any = None) -> None:
        self.num_registers = num_registers
        self.embedding_dim = embedding_dim
        super().__init__(
            fl.Slicing(dim=1, end=1),
            fl.Parameter(num_registers, embedding_dim, device=device, dtype=dtype),
            fl.Slicing(dim=1, start=1),
            dim=1,
        )


class ViT(fl.Chain):
    """Vision Transformer (arXiv:2010.11929) with DINOv2's position resampling, LayerScale and optional registers."""

    def __init__(self, embedding_dim: int = 768, patch_size: int = 16, image_size: int = 224, num_layers: int = 12, num_heads: int = 12,
                 norm_eps: float = 1e-6, mlp_ratio: int = 4, num_registers: int = 0, activation: fl.Activation | None = None,
                 feedforward_dim: int | None = None, interpolate_antialias: bool = False, interpolate_mode: str = "bicubic",
                 device: Any = None, dtype: Any = None) -> None:
        activation = activation if activation is not None else fl.GeLU()
        num_patches = image_size // patch_size
        self.embedding_dim = embedding_dim
        self.patch_size = patch_size
        self.image_size = image_size
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.norm_eps = norm_eps
        self.mlp_ratio = mlp_ratio
        self.num_registers = num_registers
        self.feedforward_dim = feedforward_dim
        super().__init__(
            fl.Concatenate(
                ClassToken(embedding_dim, device=device, dtype=dtype),
                PatchEncoder(3, embedding_dim, patch_size, device=device, dtype=dtype),
                dim=1,
            ),
            PositionalEncoder(
                PositionalEmbedding(num_patches**2 + 1, embedding_dim, patch_size, device=device, dtype=dtype),
                fl.Chain(
                    fl.Parallel(fl.Identity(), fl.UseContext(context="dinov2_vit", key="input")),
                    InterpolateEmbedding(mode=interpolate_mode, antialias=interpolate_antialias, patch_size=patch_size),
                ),
            ),
            Transformer(
                TransformerLayer(embedding_dim, num_heads, norm_eps, mlp_ratio, activation, feedforward_dim=feedforward_dim, device=device, dtype=dtype)
                for _ in range(num_layers)
            ),
            fl.LayerNorm(embedding_dim, eps=norm_eps, device=device, dtype=dtype),
        )
        if num_registers > 0:
            self.insert_before_type(Transformer, Registers(num_registers, embedding_dim, device=device, dtype=dtype))

    def init_context(self) -> Contexts:
        return {"dinov2_vit": {"input": None}}


def preprocess(img: Any, dim: int = 224) -> Tensor:
    """A PIL image -> float32 (3, dim, dim): resized (no centre crop) and normalised with ImageNet's mean and standard deviation.  Host side."""
    import numpy as np

    t = torch.from_numpy(np.asarray(img.convert("RGB").resize((dim, dim))).astype(np.float32) / 255.0).permute(2, 0, 1)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(-1, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(-1, 1, 1)
    return (t - mean) / std


def _named(name: str, doc: str, **cfg: Any) -> type:
    def __init__(self: ViT, device: Any = None, dtype: Any = None) -> None:
        kw = dict(cfg)
        if kw.pop("swiglu", False):
            kw["activation"] = fl.GLU(fl.SiLU())
        ViT.__init__(self, patch_size=14, image_size=518, device=device, dtype=dtype, **kw)

    return type(name, (ViT,), {"__init__": __init__, "__doc__": doc, "__module__": __name__})


_REG = dict(num_registers=4, interpolate_antialias=True)
DINOv2_small = _named("DINOv2_small", "DINOv2 small: 384 wide, 12 layers, 6 heads.", embedding_dim=384, num_layers=12, num_heads=6)
DINOv2_base = _named("DINOv2_base", "DINOv2 base: 768 wide, 12 layers, 12 heads.", embedding_dim=768, num_layers=12, num_heads=12)
DINOv2_large = _named("DINOv2_large", "DINOv2 large: 1024 wide, 24 layers, 16 heads.", embedding_dim=1024, num_layers=24, num_heads=16)
DINOv2_giant = _named("DINOv2_giant", "DINOv2 giant: 1536 wide, 40 layers, 24 heads, SwiGLU feed-forward of 4096.", embedding_dim=1536, feedforward_dim=4096,
                      num_layers=40, num_heads=24, swiglu=True)
DINOv2_small_reg = _named("DINOv2_small_reg", "DINOv2 small with 4 registers and antialiased position resampling.", embedding_dim=384, num_layers=12, num_heads=6, **_REG)
DINOv2_base_reg = _named("DINOv2_base_reg", "DINOv2 base with 4 registers and antialiased position resampling.", embedding_dim=768, num_layers=12, num_heads=12, **_REG)
DINOv2_large_reg = _named("DINOv2_large_reg", "DINOv2 large with 4 registers and antialiased position resampling.", embedding_dim=1024, num_layers=24, num_heads=16, **_REG)
DINOv2_giant_reg = _named("DINOv2_giant_reg", "DINOv2 giant with 4 registers and antialiased position resampling.", embedding_dim=1536, feedforward_dim=4096,
                          num_layers=40, num_heads=24, swiglu=True, **_REG)
