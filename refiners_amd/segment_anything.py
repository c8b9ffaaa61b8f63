"""SegmentAnything ViT-H (image encoder, prompt encoders, mask decoder) as a Chain tree (BASELINE.json config 5).

Mirrors reference src/refiners/foundationals/segment_anything/image_encoder.py:8-368 (same class names, child order and
parameter names, hence the same state-dict keys -- checked against tests/golden/sam_vit_h_keys.json) and HQ-SAM
(segment_anything/hq_sam.py: the encoder hook `SAMViTAdapter` here, `HQSAMAdapter` and its decoder side at the end of the module).
Everything here is the unfused torch path; the MI355X engine (refiners_amd/engine/sam.py) lowers the same tree.

Shapes for ViT-H: (B, 3, 1024, 1024) -> patch conv 16x16/16 -> (B, 64, 64, 1280) channels-last tokens -> 32 layers
(14x14 windowed attention with the grid padded 64 -> 70, global attention in layers 7, 15, 23, 31, 16 heads of 80,
decomposed relative position bias) -> neck -> (B, 256, 64, 64).

The prompt side mirrors segment_anything/prompt_encoder.py:13-193 (PointEncoder, MaskEncoder), mask_decoder.py:12-300 and
transformer.py:6-135 (MaskDecoder: two two-way transformer layers over [5 + points] tokens and the 64 x 64 dense embedding,
two transposed 2x2 convolutions up to 256 x 256, three hypernetwork vectors per prompt) and model.py:27-200
(SegmentAnything.predict / normalize / postprocess_masks, one prompt set per call).  refiners_amd/engine/sam_decoder.py
lowers the decoder.
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum, auto
from typing import Any, Sequence, cast

import torch
import torch.nn.functional as F
from torch import Size, Tensor, nn

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.adapters import Adapter
from refiners_amd.fluxion.tree import Contexts


class PatchEncoder(fl.Chain):
    """Non-overlapping patch convolution, output channels-last."""

    def __init__(self, in_channels: int, out_channels: int, patch_size: int = 16, use_bias: bool = True, device: Any = None, dtype: Any = None) -> None:
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.patch_size = patch_size
        self.use_bias = use_bias
        super().__init__(
            fl.Conv2d(in_channels, out_channels, kernel_size=(patch_size, patch_size), stride=(patch_size, patch_size), use_bias=use_bias, device=device, dtype=dtype),
            fl.Permute(0, 2, 3, 1),
        )


class PositionalEncoder(fl.Residual):
    """x + learned (H, W, C) position table."""

    def __init__(self, embedding_dim: int, image_embedding_size: tuple[int, int], device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.image_embedding_size = image_embedding_size
        super().__init__(fl.Parameter(image_embedding_size[0], image_embedding_size[1], embedding_dim, device=device, dtype=dtype))


class RelativePositionAttention(fl.WeightedModule):
    """softmax(q k^T / sqrt(d) + rel_h + rel_w) v on a packed (B, H, W, 3C) qkv tensor; the bias is the decomposed
    relative position term rel_h[q, kh] = q . Rh[qh - kh], rel_w[q, kw] = q . Rw[qw - kw] of the UNSCALED query."""

    def __init__(self, embedding_dim: int, num_heads: int, spatial_size: tuple[int, int], device: Any = None, dtype: Any = None) -> None:
        super().__init__()
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        self.head_dim = embedding_dim // num_heads
        self.spatial_size = spatial_size
        self.horizontal_embedding = nn.Parameter(torch.zeros(2 * spatial_size[0] - 1, self.head_dim, device=device, dtype=dtype))
        self.vertical_embedding = nn.Parameter(torch.zeros(2 * spatial_size[1] - 1, self.head_dim, device=device, dtype=dtype))

    @property
    def device(self) -> torch.device:
        return self.horizontal_embedding.device

    @property
    def dtype(self) -> torch.dtype:
        return self.horizontal_embedding.dtype

    @staticmethod
    def relative_index(size: int) -> Tensor:
        i = torch.arange(size)
        return i[:, None] - i[None, :] + size - 1

    def bias_terms(self, q: Tensor) -> tuple[Tensor, Tensor]:
        """q: (N, L, d) -> (horizontal (N, h, w, 1, w'), vertical (N, h, w, h', 1)).  NB: the reference unpacks
        `width, height = spatial_size` and reshapes q to (N, width, height, d); spatial sizes are square in every SAM
        configuration, which is what makes that consistent."""
        width, height = self.spatial_size
        hor = self.horizontal_embedding[self.relative_index(width)]
        ver = self.vertical_embedding[self.relative_index(height)]
        q4 = q.reshape(q.shape[0], width, height, -1)
        rel_hor = torch.einsum("bhwc,wkc->bhwk", q4, hor).unsqueeze(-2)
        rel_ver = torch.einsum("bhwc,hkc->bhwk", q4, ver).unsqueeze(-1)
        return rel_hor, rel_ver

    def forward(self, x: Tensor) -> Tensor:
        batch, height, width, _ = x.shape
        qkv = x.reshape(batch, width * height, 3, self.num_heads, -1).permute(2, 0, 3, 1, 4).reshape(3, batch * self.num_heads, width * height, -1)
        q, k, v = qkv.unbind(0)
        rel_hor, rel_ver = self.bias_terms(q)
        att = (q * self.head_dim ** -0.5) @ k.transpose(-2, -1)
        att = ((att.reshape(-1, height, width, height, width) + rel_ver) + rel_hor).reshape(att.shape)
        out = att.softmax(dim=-1) @ v
        return out.reshape(batch, self.num_heads, height, width, -1).permute(0, 2, 3, 1, 4).reshape(batch, height, width, -1)


class FusedSelfAttention(fl.Chain):
    """Linear(C -> 3C) -> RelativePositionAttention -> Linear(C -> C)."""

    def __init__(self, embedding_dim: int = 768, spatial_size: tuple[int, int] = (64, 64), num_heads: int = 1, use_bias: bool = True,
                 is_causal: bool = False, device: Any = None, dtype: Any = None) -> None:
        assert embedding_dim % num_heads == 0, f"Embedding dim (embedding_dim={embedding_dim}) must be divisible by num heads (num_heads={num_heads})"
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        self.use_bias = use_bias
        self.is_causal = is_causal
        super().__init__(
            fl.Linear(embedding_dim, 3 * embedding_dim, bias=use_bias, device=device, dtype=dtype),
            RelativePositionAttention(embedding_dim, num_heads, spatial_size, device=device, dtype=dtype),
            fl.Linear(embedding_dim, embedding_dim, bias=True, device=device, dtype=dtype),
        )


class FeedForward(fl.Chain):
    def __init__(self, embedding_dim: int, feedforward_dim: int, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.feedforward_dim = feedforward_dim
        super().__init__(
            fl.Linear(embedding_dim, feedforward_dim, bias=True, device=device, dtype=dtype),
            fl.GeLU(),
            fl.Linear(feedforward_dim, embedding_dim, bias=True, device=device, dtype=dtype),
        )


class WindowPartition(fl.ContextModule):
    """(B, H, W, C) -> (B * nH * nW, ws, ws, C), zero padding H and W up to multiples of the window size (kept in context)."""

    def __init__(self) -> None:
        super().__init__()

    def forward(self, x: Tensor) -> Tensor:
        b, h, w, c = x.shape
        ctx = self.use_context("window_partition")
        ws = ctx["window_size"]
        ph, pw = (ws - h % ws) % ws, (ws - w % ws) % ws
        if ph or pw:
            x = F.pad(x, (0, 0, 0, pw, 0, ph))
        ctx.update({"original_height": h, "original_width": w, "padded_height": h + ph, "padded_width": w + pw})
        x = x.view(b, (h + ph) // ws, ws, (w + pw) // ws, ws, c)
        return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, c)


class WindowMerge(fl.ContextModule):
    def __init__(self) -> None:
        super().__init__()

    def forward(self, x: Tensor) -> Tensor:
        ctx = self.use_context("window_partition")
        ws, ph, pw = ctx["window_size"], ctx["padded_height"], ctx["padded_width"]
        h, w = ctx["original_height"], ctx["original_width"]
        b = x.shape[0] // (ph * pw // ws // ws)
        x = x.view(b, ph // ws, pw // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).contiguous().view(b, ph, pw, -1)
        return x[:, :h, :w, :].contiguous() if (ph > h or pw > w) else x


class TransformerLayer(fl.Chain):
    def __init__(self, embedding_dim: int, num_heads: int, feedforward_dim: int, image_embedding_size: tuple[int, int],
                 window_size: int | None = None, layer_norm_eps: float = 1e-6, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        self.feedforward_dim = feedforward_dim
        self.window_size = window_size
        self.layer_norm_eps = layer_norm_eps
        self.image_embedding_size = image_embedding_size
        kw = dict(device=device, dtype=dtype)
        windowed = window_size is not None
        super().__init__(
            fl.Residual(
                fl.LayerNorm(embedding_dim, eps=layer_norm_eps, **kw),
                WindowPartition() if windowed else fl.Identity(),
                FusedSelfAttention(embedding_dim=embedding_dim, num_heads=num_heads,
                                   spatial_size=(window_size, window_size) if windowed else image_embedding_size, **kw),
                WindowMerge() if windowed else fl.Reshape(image_embedding_size[0], image_embedding_size[1], embedding_dim),
            ),
            fl.Residual(
                fl.LayerNorm(embedding_dim, eps=layer_norm_eps, **kw),
                FeedForward(embedding_dim=embedding_dim, feedforward_dim=feedforward_dim, **kw),
            ),
        )

    def init_context(self) -> Contexts:
        return {"window_partition": {"window_size": self.window_size}}


class Neck(fl.Chain):
    def __init__(self, in_channels: int = 768, device: Any = None, dtype: Any = None) -> None:
        self.in_channels = in_channels
        kw = dict(device=device, dtype=dtype)
        super().__init__(
            fl.Permute(0, 3, 1, 2),
            fl.Conv2d(in_channels, 256, kernel_size=1, use_bias=False, **kw),
            fl.LayerNorm2d(256, **kw),
            fl.Conv2d(256, 256, kernel_size=3, padding=1, use_bias=False, **kw),
            fl.LayerNorm2d(256, **kw),
        )


class Transformer(fl.Chain):
    pass


class SAMViT(fl.Chain):
    def __init__(self, embedding_dim: int, num_layers: int, num_heads: int, global_attention_indices: tuple[int, ...] | None = None,
                 device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.image_size = (1024, 1024)
        self.patch_size = 16
        self.window_size = 14
        self.image_embedding_size = (self.image_size[0] // self.patch_size, self.image_size[1] // self.patch_size)
        self.feed_forward_dim = 4 * embedding_dim
        self.global_attention_indices = global_attention_indices or tuple()
        kw = dict(device=device, dtype=dtype)
        super().__init__(
            PatchEncoder(in_channels=3, out_channels=embedding_dim, patch_size=self.patch_size, **kw),
            PositionalEncoder(embedding_dim=embedding_dim, image_embedding_size=self.image_embedding_size, **kw),
            Transformer(
                TransformerLayer(embedding_dim=embedding_dim, num_heads=num_heads, feedforward_dim=self.feed_forward_dim,
                                 window_size=None if i in self.global_attention_indices else self.window_size,
                                 image_embedding_size=self.image_embedding_size, **kw)
                for i in range(num_layers)
            ),
            Neck(in_channels=embedding_dim, **kw),
        )


class SAMViTH(SAMViT):
    def __init__(self, device: Any = None, dtype: Any = None) -> None:
        super().__init__(embedding_dim=1280, num_layers=32, num_heads=16, global_attention_indices=(7, 15, 23, 31), device=device, dtype=dtype)


class SAMViTAdapter(fl.Chain, Adapter[SAMViT]):
    """HQ-SAM's encoder hook: stores the output of the first global-attention layer in context "hq_sam".early_vit_embedding."""

    def __init__(self, target: SAMViT) -> None:
        with self.setup_adapter(target):
            super().__init__(target)
        layer = next((t for t in target.layers(TransformerLayer) if t.window_size is None), None)
        assert layer is not None
        self._transformer_layer = [layer]
        self._set_early_vit_embedding_context = [fl.SetContext("hq_sam", "early_vit_embedding")]

    @property
    def target_transformer_layer(self) -> TransformerLayer:
        return self._transformer_layer[0]

    @property
    def set_early_vit_embedding_context(self) -> fl.SetContext:
        return self._set_early_vit_embedding_context[0]

    def inject(self, parent: fl.Chain | None = None) -> "SAMViTAdapter":
        self.target_transformer_layer.append(self.set_early_vit_embedding_context)
        return super().inject(parent)

    def eject(self) -> None:
        self.target_transformer_layer.remove(self.set_early_vit_embedding_context)
        super().eject()


# ==================================================================================================================== prompt side
class CoordinateEncoder(fl.Chain):
    """Random Fourier features of (x, y) in [0, 1]: sin / cos of 2 pi scale (2 p - 1) G (reference prompt_encoder.py:13-31)."""

    def __init__(self, num_positional_features: int = 64, scale: float = 1, device: Any = None, dtype: Any = None) -> None:
        self.num_positional_features = num_positional_features
        self.scale = scale
        super().__init__(
            fl.Multiply(scale=2, bias=-1),
            fl.Linear(in_features=2, out_features=num_positional_features, bias=False, device=device, dtype=dtype),
            fl.Multiply(scale=2 * torch.pi * self.scale),
            fl.Concatenate(fl.Sin(), fl.Cos(), dim=-1),
        )


class PointType(Enum):
    BACKGROUND = auto()
    FOREGROUND = auto()
    BOX_TOP_LEFT = auto()
    BOX_BOTTOM_RIGHT = auto()
    NOT_A_POINT = auto()


class PointTypeEmbedding(fl.WeightedModule, fl.ContextModule):
    def __init__(self, embedding_dim: int, device: Any = None, dtype: Any = None) -> None:
        super().__init__()
        self.embedding_dim = embedding_dim
        self.weight = nn.Parameter(data=torch.randn(len(PointType), self.embedding_dim, device=device, dtype=dtype))

    def forward(self, type_mask: Tensor) -> Tensor:
        assert isinstance(type_mask, Tensor), "type_mask must be a Tensor."
        embeddings = torch.zeros(*type_mask.shape, self.embedding_dim).to(device=type_mask.device)
        for type_id in PointType:
            mask = type_mask == type_id.value
            embeddings[mask] = self.weight[type_id.value - 1]
        return embeddings


class PointEncoder(fl.Chain):
    """Points + type mask -> [1, points (+1 NOT_A_POINT pad when no box), 256] sparse embedding (prompt_encoder.py:56-160)."""

    def __init__(self, embedding_dim: int = 256, scale: float = 1, device: Any = None, dtype: Any = None) -> None:
        assert embedding_dim % 2 == 0, "embedding_dim must be divisible by 2."
        self.embedding_dim = embedding_dim
        self.scale = scale
        super().__init__(
            CoordinateEncoder(num_positional_features=embedding_dim // 2, scale=scale, device=device, dtype=dtype),
            fl.Lambda(func=self.pad),
            fl.Residual(
                fl.UseContext(context="point_encoder", key="type_mask"),
                PointTypeEmbedding(embedding_dim=embedding_dim, device=device, dtype=dtype),
            ),
        )

    def pad(self, x: Tensor) -> Tensor:
        type_mask: Tensor = self.use_context("point_encoder")["type_mask"]
        if torch.any((type_mask == PointType.BOX_TOP_LEFT.value) | (type_mask == PointType.BOX_BOTTOM_RIGHT.value)):
            return x  # some boxes have been passed: no padding
        type_mask = torch.cat([type_mask, torch.full((type_mask.shape[0], 1), PointType.NOT_A_POINT.value, device=type_mask.device)], dim=1)
        self.set_context(context="point_encoder", value={"type_mask": type_mask})
        return torch.cat([x, torch.zeros((x.shape[0], 1, x.shape[-1]), device=x.device)], dim=1)

    def init_context(self) -> Contexts:
        return {"point_encoder": {"type_mask": None}}

    def set_type_mask(self, type_mask: Tensor) -> None:
        self.set_context(context="point_encoder", value={"type_mask": type_mask})

    def get_dense_positional_embedding(self, image_embedding_size: tuple[int, int]) -> Tensor:
        coordinate_encoder = self.ensure_find(layer_type=CoordinateEncoder)
        height, width = image_embedding_size
        grid = torch.ones((height, width), device=self.device, dtype=self.dtype)
        y_embedding = (grid.cumsum(dim=0) - 0.5) / height
        x_embedding = (grid.cumsum(dim=1) - 0.5) / width
        return coordinate_encoder(torch.stack(tensors=[x_embedding, y_embedding], dim=-1)).permute(2, 0, 1).unsqueeze(dim=0)

    def points_to_tensor(
        self,
        foreground_points: Sequence[tuple[float, float]] | None = None,
        background_points: Sequence[tuple[float, float]] | None = None,
        not_a_points: Sequence[tuple[float, float]] | None = None,
        box_points: Sequence[Sequence[tuple[float, float]]] | None = None,
    ) -> tuple[Tensor, Tensor]:
        foreground_points = foreground_points or []
        background_points = background_points or []
        not_a_points = not_a_points or []
        box_points = box_points or []
        top_left_points = [box[0] for box in box_points]
        bottom_right_points = [box[1] for box in box_points]
        coordinates: list[Tensor] = []
        type_ids: list[Tensor] = []
        # in the order of the PointType enum
        for type_id, coords_seq in zip(PointType, [background_points, foreground_points, top_left_points, bottom_right_points, not_a_points]):
            if len(coords_seq) > 0:
                coordinates.append(torch.tensor(data=list(coords_seq), dtype=torch.float, device=self.device))
                type_ids.append(torch.tensor(data=[type_id.value] * len(coords_seq), dtype=torch.int, device=self.device))
        return torch.cat(tensors=coordinates, dim=0).unsqueeze(dim=0), torch.cat(tensors=type_ids, dim=0).unsqueeze(dim=0)


class MaskEncoder(fl.Chain):
    """[B, 1, 256, 256] mask logits -> [B, 256, 64, 64] dense embedding; `no_mask_embedding` otherwise (prompt_encoder.py:163-193)."""

    def __init__(self, embedding_dim: int = 256, intermediate_channels: int = 16, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.intermediate_channels = intermediate_channels
        kw = dict(device=device, dtype=dtype)
        super().__init__(
            fl.Conv2d(in_channels=1, out_channels=self.intermediate_channels // 4, kernel_size=2, stride=2, **kw),
            fl.LayerNorm2d(channels=self.intermediate_channels // 4, **kw),
            fl.GeLU(),
            fl.Conv2d(in_channels=self.intermediate_channels // 4, out_channels=self.intermediate_channels, kernel_size=2, stride=2, **kw),
            fl.LayerNorm2d(channels=self.intermediate_channels, **kw),
            fl.GeLU(),
            fl.Conv2d(in_channels=self.intermediate_channels, out_channels=self.embedding_dim, kernel_size=1, **kw),
        )
        self.register_parameter("no_mask_embedding", nn.Parameter(torch.randn(1, embedding_dim, device=device, dtype=dtype)))

    def get_no_mask_dense_embedding(self, image_embedding_size: tuple[int, int], batch_size: int = 1) -> Tensor:
        no_mask_embedding = cast(Tensor, self.no_mask_embedding)
        return no_mask_embedding.reshape(1, -1, 1, 1).expand(batch_size, -1, image_embedding_size[0], image_embedding_size[1])


# ==================================================================================================================== mask decoder
class _DecoderFeedForward(fl.Residual):
    def __init__(self, embedding_dim: int, feed_forward_dim: int, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.feed_forward_dim = feed_forward_dim
        super().__init__(
            fl.Linear(in_features=embedding_dim, out_features=feed_forward_dim, device=device, dtype=dtype),
            fl.ReLU(),
            fl.Linear(in_features=feed_forward_dim, out_features=embedding_dim, device=device, dtype=dtype),
        )


# transformer.py:6-16 and mask_decoder.py:38-39 name these `FeedForward` and `Transformer`, like two different classes of the image
# encoder above: same class names (the engine and the state-dict keys go by them), other Python names in this module
_DecoderFeedForward.__name__ = _DecoderFeedForward.__qualname__ = "FeedForward"


class SparseSelfAttention(fl.Residual):
    """x + Attention(x + sparse, x + sparse, x) (transformer.py:19-40)."""

    def __init__(self, embedding_dim: int, inner_dim: int | None = None, num_heads: int = 1, device: Any = None, dtype: Any = None) -> None:
        add_sparse_embedding = fl.Residual(fl.UseContext(context="mask_decoder", key="sparse_embedding"))
        super().__init__(
            fl.Parallel(add_sparse_embedding, add_sparse_embedding, fl.Identity()),
            fl.Attention(embedding_dim=embedding_dim, inner_dim=inner_dim, num_heads=num_heads, is_optimized=False, device=device, dtype=dtype),
        )


class SparseCrossDenseAttention(fl.Residual):
    """Token -> image: x + Attention(x + sparse, dense + pe, dense) (transformer.py:43-68)."""

    def __init__(self, embedding_dim: int, num_heads: int = 8, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        super().__init__(
            fl.Parallel(
                fl.Residual(fl.UseContext(context="mask_decoder", key="sparse_embedding")),
                fl.Sum(
                    fl.UseContext(context="mask_decoder", key="dense_embedding"),
                    fl.UseContext(context="mask_decoder", key="dense_positional_embedding"),
                ),
                fl.UseContext(context="mask_decoder", key="dense_embedding"),
            ),
            fl.Attention(embedding_dim=embedding_dim, inner_dim=embedding_dim // 2, num_heads=num_heads, is_optimized=False, device=device, dtype=dtype),
        )


class DenseCrossSparseAttention(fl.Chain):
    """Image -> token: Attention(dense + pe, x + sparse, x) (transformer.py:71-94)."""

    def __init__(self, embedding_dim: int, num_heads: int = 8, device: Any = None, dtype: Any = None) -> None:
        super().__init__(
            fl.Parallel(
                fl.Sum(
                    fl.UseContext(context="mask_decoder", key="dense_embedding"),
                    fl.UseContext(context="mask_decoder", key="dense_positional_embedding"),
                ),
                fl.Residual(fl.UseContext(context="mask_decoder", key="sparse_embedding")),
                fl.Identity(),
            ),
            fl.Attention(embedding_dim=embedding_dim, inner_dim=embedding_dim // 2, num_heads=num_heads, is_optimized=False, device=device, dtype=dtype),
        )


class TwoWayTransformerLayer(fl.Chain):
    """transformer.py:97-135."""

    def __init__(self, embedding_dim: int, num_heads: int = 8, feed_forward_dim: int = 2048, use_residual_self_attention: bool = True,
                 device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        self.feed_forward_dim = feed_forward_dim
        kw = dict(device=device, dtype=dtype)
        self_attention = (
            SparseSelfAttention(embedding_dim=embedding_dim, num_heads=num_heads, **kw)
            if use_residual_self_attention
            else fl.SelfAttention(embedding_dim=embedding_dim, num_heads=num_heads, is_optimized=False, **kw)
        )
        super().__init__(
            self_attention,
            fl.LayerNorm(normalized_shape=embedding_dim, **kw),
            SparseCrossDenseAttention(embedding_dim=embedding_dim, num_heads=num_heads, **kw),
            fl.LayerNorm(normalized_shape=embedding_dim, **kw),
            _DecoderFeedForward(embedding_dim=embedding_dim, feed_forward_dim=feed_forward_dim, **kw),
            fl.LayerNorm(normalized_shape=embedding_dim, **kw),
            fl.Passthrough(
                fl.Sum(
                    fl.UseContext(context="mask_decoder", key="dense_embedding"),
                    DenseCrossSparseAttention(embedding_dim=embedding_dim, num_heads=num_heads, **kw),
                ),
                fl.LayerNorm(normalized_shape=embedding_dim, **kw),
                fl.SetContext(context="mask_decoder", key="dense_embedding"),
            ),
        )


class EmbeddingsAggregator(fl.ContextModule):
    """tokens -> sparse = [tokens | point embedding]; publishes the flattened dense embedding (mask_decoder.py:12-35)."""

    def forward(self, tokens: Tensor) -> Tensor:
        mask_decoder = self.ensure_parent
        ctx = mask_decoder.use_context(context_name="mask_decoder")
        image_embedding, point_embedding = ctx["image_embedding"], ctx["point_embedding"]
        mask_embedding, dense_positional_embedding = ctx["mask_embedding"], ctx["dense_positional_embedding"]
        sparse_embedding = torch.cat(tensors=(tokens, point_embedding), dim=1)
        dense_embedding = (image_embedding + mask_embedding).flatten(start_dim=2).transpose(1, 2)
        if dense_positional_embedding.shape != dense_embedding.shape:
            dense_positional_embedding = dense_positional_embedding.flatten(start_dim=2).transpose(1, 2)
        ctx.update({"dense_embedding": dense_embedding, "dense_positional_embedding": dense_positional_embedding, "sparse_embedding": sparse_embedding})
        mask_decoder.set_context(context="mask_decoder", value=ctx)
        return sparse_embedding


class _DecoderTransformer(fl.Chain):
    pass


_DecoderTransformer.__name__ = _DecoderTransformer.__qualname__ = "Transformer"


class Hypernetworks(fl.Concatenate):
    """One 3-layer MLP (256 -> 256 -> 256 -> 32) per mask token (mask_decoder.py:42-72)."""

    def __init__(self, embedding_dim: int = 256, num_layers: int = 3, num_mask_tokens: int = 4, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_layers = num_layers
        self.num_mask_tokens = num_mask_tokens
        super().__init__(
            *[
                fl.Chain(
                    fl.Slicing(dim=1, start=i, end=i + 1),
                    fl.MultiLinear(input_dim=embedding_dim, output_dim=embedding_dim // 8, inner_dim=embedding_dim, num_layers=num_layers, device=device, dtype=dtype),
                )
                for i in range(num_mask_tokens)
            ],
            dim=1,
        )


class DenseEmbeddingUpscaling(fl.Chain):
    """[B, 4096, 256] -> ConvT 2x2/2 -> LayerNorm2d -> GELU -> ConvT 2x2/2 -> GELU -> [B, 32, 65536] (mask_decoder.py:75-112)."""

    def __init__(self, embedding_dim: int = 256, dense_embedding_side_dim: int = 64, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.dense_embedding_side_dim = dense_embedding_side_dim
        kw = dict(device=device, dtype=dtype)
        super().__init__(
            fl.UseContext(context="mask_decoder", key="dense_embedding"),
            fl.Transpose(dim0=1, dim1=2),
            fl.Reshape(embedding_dim, dense_embedding_side_dim, dense_embedding_side_dim),
            fl.ConvTranspose2d(in_channels=embedding_dim, out_channels=embedding_dim // 4, kernel_size=2, stride=2, **kw),
            fl.LayerNorm2d(channels=embedding_dim // 4, **kw),
            fl.GeLU(),
            fl.ConvTranspose2d(in_channels=embedding_dim // 4, out_channels=embedding_dim // 8, kernel_size=2, stride=2, **kw),
            fl.GeLU(),
            fl.Flatten(start_dim=2),
            fl.SetContext(context="mask_decoder", key="upscaled_dense_embedding"),
        )


class MaskDecoderTokens(fl.Chain):
    """The IoU token + 4 mask tokens, broadcast to the batch of the image embedding (mask_decoder.py:115-129)."""

    def __init__(self, embedding_dim: int = 256, num_mask_tokens: int = 4, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_mask_tokens = num_mask_tokens
        super().__init__(
            fl.UseContext(context="mask_decoder", key="image_embedding"),
            fl.Parameter(num_mask_tokens + 1, embedding_dim, device=device, dtype=dtype),
        )


class MaskPrediction(fl.Chain):
    """hypernetwork vectors @ upscaled embedding, kept masks (3 with multimask output, else the first) (mask_decoder.py:132-164)."""

    def __init__(self, embedding_dim: int, num_mask_tokens: int, multimask_output: bool, num_layers: int = 3, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_mask_tokens = num_mask_tokens
        self.num_layers = num_layers
        self.multimask_output = multimask_output
        start_mask, num_masks = (1, num_mask_tokens - 1) if multimask_output else (0, 1)
        super().__init__(
            fl.Slicing(dim=1, start=1, end=num_mask_tokens + 1),  # drop the IoU token and the prompt tokens
            fl.Matmul(
                input=Hypernetworks(embedding_dim=embedding_dim, num_layers=num_layers, num_mask_tokens=num_mask_tokens, device=device, dtype=dtype),
                other=DenseEmbeddingUpscaling(embedding_dim=embedding_dim, device=device, dtype=dtype),
            ),
            fl.Slicing(dim=1, start=start_mask, end=start_mask + num_masks),
            fl.Reshape(num_masks, embedding_dim, embedding_dim),
        )


class IOUPrediction(fl.Chain):
    """mask_decoder.py:167-194."""

    def __init__(self, embedding_dim: int, num_layers: int, num_mask_tokens: int, multimask_output: bool, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_layers = num_layers
        self.multimask_output = multimask_output
        super().__init__(
            fl.Slicing(dim=1, start=0, end=1),  # the IoU token
            fl.Squeeze(dim=1),
            fl.MultiLinear(input_dim=embedding_dim, output_dim=num_mask_tokens, inner_dim=embedding_dim, num_layers=num_layers, device=device, dtype=dtype),
            fl.Slicing(dim=-1, start=1) if multimask_output else fl.Slicing(dim=-1, start=0, end=1),
        )


class Predictions(fl.Parallel):
    """mask_decoder.py:197-226."""

    def __init__(self, embedding_dim: int, num_mask_tokens: int, multimask_output: bool, num_layers: int = 3, device: Any = None, dtype: Any = None) -> None:
        self.embedding_dim = embedding_dim
        self.num_mask_tokens = num_mask_tokens
        self.num_layers = num_layers
        super().__init__(
            MaskPrediction(embedding_dim=embedding_dim, num_mask_tokens=num_mask_tokens, multimask_output=multimask_output, device=device, dtype=dtype),
            IOUPrediction(embedding_dim=embedding_dim, num_layers=num_layers, num_mask_tokens=num_mask_tokens, multimask_output=multimask_output, device=device, dtype=dtype),
        )


class MaskDecoder(fl.Chain):
    """mask_decoder.py:229-300."""

    def __init__(self, multimask_output: bool = True, embedding_dim: int = 256, feed_forward_dim: int = 2048, num_layers: int = 2,
                 num_multimask_outputs: int = 3, device: Any = None, dtype: Any = None) -> None:
        self.multimask_output = multimask_output
        self.embedding_dim = embedding_dim
        self.feed_forward_dim = feed_forward_dim
        self.num_layers = num_layers
        self.num_multimask_outputs = num_multimask_outputs
        num_mask_tokens = self.num_multimask_outputs + 1  # + the single-output mask token
        kw = dict(device=device, dtype=dtype)
        super().__init__(
            MaskDecoderTokens(embedding_dim=embedding_dim, num_mask_tokens=num_mask_tokens, **kw),
            EmbeddingsAggregator(),
            _DecoderTransformer(
                *(
                    TwoWayTransformerLayer(embedding_dim=embedding_dim, num_heads=8, feed_forward_dim=feed_forward_dim, use_residual_self_attention=i > 0, **kw)
                    for i in range(num_layers)
                ),
                SparseCrossDenseAttention(embedding_dim=embedding_dim, **kw),
                fl.LayerNorm(normalized_shape=embedding_dim, **kw),
            ),
            Predictions(embedding_dim=embedding_dim, num_mask_tokens=num_mask_tokens, multimask_output=multimask_output, **kw),
        )

    def init_context(self) -> Contexts:
        return {"mask_decoder": {"image_embedding": None, "point_embedding": None, "mask_embedding": None, "dense_positional_embedding": None}}

    def set_image_embedding(self, image_embedding: Tensor) -> None:
        self.use_context(context_name="mask_decoder")["image_embedding"] = image_embedding

    def set_point_embedding(self, point_embedding: Tensor) -> None:
        self.use_context(context_name="mask_decoder")["point_embedding"] = point_embedding

    def set_mask_embedding(self, mask_embedding: Tensor) -> None:
        self.use_context(context_name="mask_decoder")["mask_embedding"] = mask_embedding

    def set_dense_positional_embedding(self, dense_positional_embedding: Tensor) -> None:
        self.use_context(context_name="mask_decoder")["dense_positional_embedding"] = dense_positional_embedding


# ==================================================================================================================== the model
def compute_scaled_size(size: tuple[int, int], image_encoder_resolution: int) -> tuple[int, int]:
    """(h, w) scaled to fit the encoder's square, aspect kept (reference utils.py:7-24)."""
    oldh, oldw = size
    scale = image_encoder_resolution * 1.0 / max(oldh, oldw)
    newh, neww = oldh * scale, oldw * scale
    return (int(newh + 0.5), int(neww + 0.5))


def postprocess_masks(low_res_masks: Tensor, original_size: tuple[int, int], image_encoder_resolution: int) -> Tensor:
    """Bilinear resize to the encoder's square, crop the padding, bilinear resize to the original size (utils.py:93-110)."""
    scaled_size = compute_scaled_size(original_size, image_encoder_resolution)
    masks = F.interpolate(low_res_masks, size=Size((image_encoder_resolution, image_encoder_resolution)), mode="bilinear")
    masks = masks[..., : scaled_size[0], : scaled_size[1]]
    return F.interpolate(masks, size=Size(original_size), mode="bilinear")


def normalize_coordinates(coordinates: Tensor, original_size: tuple[int, int], image_encoder_resolution: int) -> Tensor:
    """(x, y) pixel coordinates of the original image -> [0, 1] coordinates of the padded encoder input (utils.py:113-129)."""
    scaled_size = compute_scaled_size(original_size, image_encoder_resolution)
    coordinates[:, :, 0] = ((coordinates[:, :, 0] * (scaled_size[1] / original_size[1])) + 0.5) / image_encoder_resolution
    coordinates[:, :, 1] = ((coordinates[:, :, 1] * (scaled_size[0] / original_size[0])) + 0.5) / image_encoder_resolution
    return coordinates


def preprocess_image(image: Any, image_encoder_resolution: int, device: Any = None, dtype: Any = None) -> Tensor:
    """PIL image -> normalised [1, 3, R, R] tensor, resized with its aspect kept and zero padded (utils.py:27-90)."""
    import numpy as np
    from PIL import Image

    h, w = compute_scaled_size((image.height, image.width), image_encoder_resolution)
    resized = image.resize((w, h), resample=Image.Resampling.BILINEAR)
    t = torch.tensor(np.array(resized).astype(np.float32) / 255.0, device=device, dtype=dtype)
    t = (t.unsqueeze(0) if resized.mode == "L" else t.permute(2, 0, 1)) * 255.0
    mean = torch.tensor([123.675, 116.28, 103.53], dtype=t.dtype, device=t.device).view(-1, 1, 1)
    std = torch.tensor([58.395, 57.12, 57.375], dtype=t.dtype, device=t.device).view(-1, 1, 1)
    t = ((t - mean) / std).unsqueeze(0)
    return F.pad(t, (0, image_encoder_resolution - w, 0, image_encoder_resolution - h))


@dataclass
class ImageEmbedding:
    features: Tensor
    original_image_size: tuple[int, int]  # (height, width)


class SegmentAnything(fl.Chain):
    """model.py:27-200.  mask_threshold = 0."""

    mask_threshold: float = 0.0

    def __init__(self, image_encoder: SAMViT, point_encoder: PointEncoder, mask_encoder: MaskEncoder, mask_decoder: MaskDecoder,
                 device: Any = "cpu", dtype: Any = torch.float32) -> None:
        super().__init__(image_encoder, point_encoder, mask_encoder, mask_decoder)
        self.to(device=device, dtype=dtype)

    @property
    def image_encoder(self) -> SAMViT:
        return self.ensure_find(SAMViT)

    @property
    def point_encoder(self) -> PointEncoder:
        return self.ensure_find(PointEncoder)

    @property
    def mask_encoder(self) -> MaskEncoder:
        return self.ensure_find(MaskEncoder)

    @property
    def mask_decoder(self) -> MaskDecoder:
        return self.ensure_find(MaskDecoder)

    @torch.no_grad()
    def compute_image_embedding(self, image: Any) -> ImageEmbedding:
        return ImageEmbedding(features=self.image_encoder(self.preprocess_image(image)), original_image_size=(image.height, image.width))

    @torch.no_grad()
    def predict(
        self,
        input: Any,
        foreground_points: Sequence[tuple[float, float]] | None = None,
        background_points: Sequence[tuple[float, float]] | None = None,
        box_points: Sequence[Sequence[tuple[float, float]]] | None = None,
        low_res_mask: Tensor | None = None,
        binarize: bool = True,
    ) -> tuple[Tensor, Tensor, Tensor]:
        """(masks [1, k, H, W] (bool when binarize), iou_predictions [1, k], low_res_masks [1, k, 256, 256]) for ONE prompt set."""
        if isinstance(input, ImageEmbedding):
            original_size, image_embedding = input.original_image_size, input.features
        else:
            original_size = (input.height, input.width)
            image_embedding = self.image_encoder(self.preprocess_image(input))
        coordinates, type_mask = self.point_encoder.points_to_tensor(foreground_points=foreground_points, background_points=background_points, box_points=box_points)
        self.point_encoder.set_type_mask(type_mask=type_mask)
        if low_res_mask is not None:
            mask_embedding = self.mask_encoder(low_res_mask)
        else:
            mask_embedding = self.mask_encoder.get_no_mask_dense_embedding(image_embedding_size=self.image_encoder.image_embedding_size)
        point_embedding = self.point_encoder(self.normalize(coordinates, original_size=original_size))
        dense_positional_embedding = self.point_encoder.get_dense_positional_embedding(image_embedding_size=self.image_encoder.image_embedding_size)
        self.mask_decoder.set_image_embedding(image_embedding=image_embedding)
        self.mask_decoder.set_mask_embedding(mask_embedding=mask_embedding)
        self.mask_decoder.set_point_embedding(point_embedding=point_embedding)
        self.mask_decoder.set_dense_positional_embedding(dense_positional_embedding=dense_positional_embedding)
        low_res_masks, iou_predictions = self.mask_decoder()
        high_res_masks = self.postprocess_masks(low_res_masks, original_size)
        if binarize:
            high_res_masks = high_res_masks > self.mask_threshold
        return high_res_masks, iou_predictions, low_res_masks

    @property
    def image_encoder_resolution(self) -> int:
        w, h = self.image_encoder.image_size
        assert w == h
        return w

    def preprocess_image(self, image: Any) -> Tensor:
        return preprocess_image(image, self.image_encoder_resolution, self.device, self.dtype)

    def normalize(self, coordinates: Tensor, original_size: tuple[int, int]) -> Tensor:
        return normalize_coordinates(coordinates, original_size, self.image_encoder_resolution)

    def postprocess_masks(self, low_res_masks: Tensor, original_size: tuple[int, int]) -> Tensor:
        return postprocess_masks(low_res_masks, original_size, self.image_encoder_resolution)


class SegmentAnythingH(SegmentAnything):
    """model.py:203-279."""

    def __init__(self, image_encoder: SAMViTH | None = None, point_encoder: PointEncoder | None = None, mask_encoder: MaskEncoder | None = None,
                 mask_decoder: MaskDecoder | None = None, multimask_output: bool | None = None, device: Any = "cpu", dtype: Any = torch.float32) -> None:
        image_encoder = image_encoder or SAMViTH()
        point_encoder = point_encoder or PointEncoder()
        mask_encoder = mask_encoder or MaskEncoder()
        if mask_decoder:
            assert multimask_output is None or mask_decoder.multimask_output == multimask_output, (
                f"mask_decoder.multimask_output {mask_decoder.multimask_output} should match multimask_output ({multimask_output})")
        else:
            mask_decoder = MaskDecoder(multimask_output) if multimask_output is not None else MaskDecoder()
        # (the reference lets SegmentAnything.__init__ move everything to "cpu" first, which a meta-device model cannot survive)
        super().__init__(image_encoder, point_encoder, mask_encoder, mask_decoder, device=device, dtype=dtype)

    @property
    def image_encoder(self) -> SAMViTH:
        return self.ensure_find(SAMViTH)


# ==================================================================================================================== HQ-SAM (decoder side)
# Mirrors segment_anything/hq_sam.py:16-229, 267-412 (arXiv:2306.01567): one more output token whose 3-layer MLP gives a 32-vector h, and
# 32-channel "HQ features" at 256 x 256 = conv(upscaled dense embedding) + upscale(image embedding) + upscale(early ViT embedding); the HQ
# mask is h . features, returned alone or added to the base SAM mask.  refiners_amd/engine/sam_hq.py lowers it.
def _convt(cin: int, cout: int, kw: dict) -> fl.ConvTranspose2d:
    return fl.ConvTranspose2d(in_channels=cin, out_channels=cout, kernel_size=2, stride=2, **kw)


class CompressViTFeat(fl.Chain):
    """context hq_sam.early_vit_embedding [B, 64, 64, vit_dim] -> [B, 32, 256, 256]."""

    def __init__(self, transformer_dim: int = 256, vit_dim: int = 1024, device: Any = None, dtype: Any = None) -> None:
        kw = dict(device=device, dtype=dtype)
        super().__init__(
            fl.UseContext(context="hq_sam", key="early_vit_embedding"),
            fl.Permute(0, 3, 1, 2),
            _convt(vit_dim, transformer_dim, kw),
            fl.LayerNorm2d(transformer_dim, **kw),
            fl.GeLU(),
            _convt(transformer_dim, transformer_dim // 8, kw),
        )


class EmbeddingEncoder(fl.Chain):
    """context mask_decoder.image_embedding [B, 256, 64, 64] -> [B, 32, 256, 256]."""

    def __init__(self, transformer_dim: int = 256, device: Any = None, dtype: Any = None) -> None:
        kw = dict(device=device, dtype=dtype)
        super().__init__(
            fl.UseContext(context="mask_decoder", key="image_embedding"),
            _convt(transformer_dim, transformer_dim // 4, kw),
            fl.LayerNorm2d(transformer_dim // 4, **kw),
            fl.GeLU(),
            _convt(transformer_dim // 4, transformer_dim // 8, kw),
        )


class HQFeatures(fl.Sum):
    def __init__(self, vit_dim: int = 1024, transformer_dim: int = 256, device: Any = None, dtype: Any = None) -> None:
        super().__init__(EmbeddingEncoder(transformer_dim, device, dtype), CompressViTFeat(transformer_dim, vit_dim, device, dtype))


class EmbeddingMaskfeature(fl.Chain):
    """context mask_decoder.upscaled_dense_embedding [B, 32, 65536] -> 3x3 conv, LayerNorm2d, GELU, 3x3 conv -> [B, 32, 256, 256]."""

    def __init__(self, transformer_dim: int = 256, device: Any = None, dtype: Any = None) -> None:
        kw = dict(device=device, dtype=dtype)
        super().__init__(
            fl.UseContext(context="mask_decoder", key="upscaled_dense_embedding"),
            fl.Reshape(-1, transformer_dim, transformer_dim),
            fl.Conv2d(transformer_dim // 8, transformer_dim // 4, 3, 1, 1, **kw),
            fl.LayerNorm2d(transformer_dim // 4, **kw),
            fl.GeLU(),
            fl.Conv2d(transformer_dim // 4, transformer_dim // 8, 3, 1, 1, **kw),
        )


class DenseEmbeddingUpscalingHQ(fl.Sum):
    def __init__(self, vit_dim: int = 1024, transformer_dim: int = 256, device: Any = None, dtype: Any = None) -> None:
        super().__init__(EmbeddingMaskfeature(transformer_dim, device, dtype), HQFeatures(vit_dim, transformer_dim, device, dtype))


class HQTokenMLP(fl.Chain):
    """The HQ token (index target_num_mask_tokens of the decoder's output tokens) -> [B, 1, embedding_dim / 8]."""

    def __init__(self, embedding_dim: int, num_layers: int = 3, target_num_mask_tokens: int = 5, device: Any = None, dtype: Any = None) -> None:
        super().__init__(
            fl.Slicing(dim=1, start=target_num_mask_tokens, end=target_num_mask_tokens + 1),
            fl.MultiLinear(input_dim=embedding_dim, output_dim=embedding_dim // 8, inner_dim=embedding_dim, num_layers=num_layers, device=device, dtype=dtype),
        )


class HQSAMMaskPrediction(fl.Matmul):
    def __init__(self, embedding_dim: int, vit_dim: int = 1024, target_num_mask_tokens: int = 5, num_layers: int = 3, device: Any = None, dtype: Any = None) -> None:
        super().__init__(
            HQTokenMLP(embedding_dim, num_layers=num_layers, target_num_mask_tokens=target_num_mask_tokens, device=device, dtype=dtype),
            fl.Chain(DenseEmbeddingUpscalingHQ(vit_dim=vit_dim, transformer_dim=256, device=device, dtype=dtype), fl.Flatten(start_dim=2)),
        )


class MaskPredictionAdapter(fl.Concatenate, Adapter[MaskPrediction]):
    """[base mask | HQ mask] along dim 1."""

    def __init__(self, target: MaskPrediction, vit_dim: int = 1024, target_num_mask_tokens: int = 5, device: Any = None, dtype: Any = None) -> None:
        with self.setup_adapter(target):
            super().__init__(
                target,
                fl.Chain(
                    HQSAMMaskPrediction(embedding_dim=target.embedding_dim, vit_dim=vit_dim, target_num_mask_tokens=target_num_mask_tokens, num_layers=3,
                                        device=device, dtype=dtype),
                    fl.Reshape(-1, target.embedding_dim, target.embedding_dim),
                ),
                dim=1,
            )

    @property
    def hq_sam_mask_prediction(self) -> HQSAMMaskPrediction:
        return self.ensure_find(HQSAMMaskPrediction)


class MaskDecoderTokensExtender(fl.Concatenate, Adapter[MaskDecoderTokens]):
    """[the 5 regular tokens ; hq_token]: the new token is a weight of the adapter."""

    def __init__(self, target: MaskDecoderTokens) -> None:
        self._hq_token = [fl.Parameter(1, target.embedding_dim, device=target.device, dtype=target.dtype)]
        with self.setup_adapter(target):
            super().__init__(
                target,
                fl.Chain(fl.UseContext(context="mask_decoder", key="image_embedding"), self.hq_token),  # (the context gives the batch size)
                dim=1,
            )

    @property
    def regular_tokens(self) -> fl.Parameter:
        return self.target.ensure_find(fl.Parameter)

    @property
    def hq_token(self) -> fl.Parameter:
        return self._hq_token[0]


class PredictionsPostProc(fl.Module):
    """(masks [B, 2, 256, 256], iou) -> the HQ mask alone (hq_mask_only) or HQ + base, section 3.3 of the paper."""

    def __init__(self, hq_mask_only: bool = False) -> None:
        super().__init__()
        self.hq_mask_only = hq_mask_only

    def forward(self, masks_predictions: Tensor, iou_predictions: Tensor) -> tuple[Tensor, Tensor]:
        hq = masks_predictions[:, -1:, ...]
        if self.hq_mask_only:
            return hq, iou_predictions
        base = masks_predictions[:, :-1, ...]
        assert base.shape[1] == 1
        return hq + base, iou_predictions


class HQSAMAdapter(fl.Chain, Adapter[SegmentAnything]):
    """HQ-SAM on a single-mask SegmentAnything: `HQSAMAdapter(sam, weights=...).inject()`, then use `sam` as usual.  Weight keys:
    `Chain.HQSAMMaskPrediction.*` and `MaskDecoderTokensExtender.hq_token.*`."""

    def init_context(self) -> Contexts:
        return {"hq_sam": {"early_vit_embedding": None}}

    def __init__(self, target: SegmentAnything, hq_mask_only: bool = False, weights: dict[str, Tensor] | None = None) -> None:
        # weight-key prefix -> the module that holds those weights (per adapter: the reference keeps ONE class-level dict, so that a second
        # adapter's modules replace the first's in `weights` / `load_weights`)
        self._adapter_modules: dict[str, fl.Module] = {}
        self.vit_embedding_dim = target.image_encoder.embedding_dim
        self.target_num_mask_tokens = target.mask_decoder.num_multimask_outputs + 2
        with self.setup_adapter(target):
            super().__init__(target)
        if target.mask_decoder.multimask_output:
            raise NotImplementedError("Multi-mask mode is not supported in HQSAMAdapter.")
        dec = target.mask_decoder
        self._mask_prediction_adapter = [MaskPredictionAdapter(dec.ensure_find(MaskPrediction), self.vit_embedding_dim, self.target_num_mask_tokens, dec.device, dec.dtype)]
        self._adapter_modules["Chain.HQSAMMaskPrediction"] = self.mask_prediction_adapter.hq_sam_mask_prediction
        self._image_encoder_adapter = [SAMViTAdapter(target.image_encoder)]
        self._predictions_post_proc = [PredictionsPostProc(hq_mask_only)]
        self._mask_decoder_tokens_extender = [MaskDecoderTokensExtender(dec.ensure_find(MaskDecoderTokens))]
        self._adapter_modules["MaskDecoderTokensExtender.hq_token"] = self.mask_decoder_tokens_extender.hq_token
        if weights is not None:
            self.load_weights(weights)
        if dec.device.type != "meta":  # (the reference moves the whole target; a model whose ViT stays on "meta" cannot be: only what was added)
            for module in self._adapter_modules.values():
                module.to(device=dec.device, dtype=dec.dtype)

    @property
    def weights(self) -> dict[str, Tensor]:
        return {f"{name}.{k}": v for name, module in self._adapter_modules.items() for k, v in module.state_dict().items()}

    def load_weights(self, weights: dict[str, Tensor], assign: bool = False) -> None:
        for name, module in self._adapter_modules.items():
            module.load_state_dict({k.removeprefix(f"{name}."): v for k, v in weights.items() if k.startswith(f"{name}.")}, **({"assign": True} if assign else {}))

    @property
    def mask_decoder_tokens_extender(self) -> MaskDecoderTokensExtender:
        return self._mask_decoder_tokens_extender[0]

    @property
    def mask_prediction_adapter(self) -> MaskPredictionAdapter:
        return self._mask_prediction_adapter[0]

    @property
    def image_encoder_adapter(self) -> SAMViTAdapter:
        return self._image_encoder_adapter[0]

    @property
    def predictions_post_proc(self) -> PredictionsPostProc:
        return self._predictions_post_proc[0]

    @property
    def hq_mask_only(self) -> bool:
        return self.predictions_post_proc.hq_mask_only

    @hq_mask_only.setter
    def hq_mask_only(self, value: bool) -> None:
        self.predictions_post_proc.hq_mask_only = value

    def inject(self, parent: fl.Chain | None = None) -> "HQSAMAdapter":
        self.mask_decoder_tokens_extender.inject()
        self.mask_prediction_adapter.inject()
        self.image_encoder_adapter.inject()
        self.target.mask_decoder.insert_after_type(Predictions, self.predictions_post_proc)
        return super().inject(parent)

    def eject(self) -> None:
        self.mask_decoder_tokens_extender.eject()
        self.mask_prediction_adapter.eject()
        self.image_encoder_adapter.eject()
        self.target.mask_decoder.remove(self.predictions_post_proc)
        super().eject()
