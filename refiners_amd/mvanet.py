"""MVANet (arXiv:2404.07445), the model behind `solutions.BoxSegmenter`, as a Chain tree.

Mirrors reference src/refiners/foundationals/swin/mvanet/{mvanet,mclm,mcrm,utils}.py: same class names, child order and parameter names,
hence the same state-dict keys (checked against tests/golden/mvanet_keys.json).  Everything here is the unfused torch path, which is
also the CPU path and the fallback of the MI355X engine (refiners_amd/engine/mvanet.py lowers the same tree).

Geometry (hard-wired by the reference: Interpolate((256, 256)), Unflatten(0, (2, 8, 2, 8)), the pyramid's 32 / 64 / 128): one
1 x 3 x 1024 x 1024 image -> five 512 x 512 views (the four quadrants, view 2 qy + qx, then the half-size image) -> Swin maps at 128, 64,
32, 16 -> MCLM on the 16 x 16 level, an MCRM per pyramid level -> the four local views merged with the global one at 256 x 256, three
convolutions, two upscaling convolutions fed with a 3 -> E convolution of the image ("shallow"), Conv2d(E -> n_logits) at 1024 x 1024.

Facts of the reference the lowering honours as well:
  * every attention is torch.nn.MultiheadAttention with one head over sequence-first (L, 1, E) tensors; in GlobalAttention Q and K
    carry the sine position embedding, V does not;
  * MCRM multiplies the local views by sigmoid(conv1x1(global)) upsampled 2x (nearest) and split into quadrants, takes its keys from
    the quadrants of the UNCHANGED global view pooled at ratios 1, 2, 4, and only then adds nearest_down(PatchMerge(local)) to the global view;
  * the position embedding is float32: under bfloat16 it is cast to the activation dtype before the sum (the reference would promote).
"""
import math
from typing import Any

import torch
import torch.nn.functional as F
from torch import Size, Tensor

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.tree import Contexts
from refiners_amd.swin import SwinTransformer


class Unflatten(fl.Module):
    def __init__(self, dim: int, sizes: tuple[int, ...]) -> None:
        super().__init__()
        self.dim = dim
        self.sizes = Size(sizes)

    def forward(self, x: Tensor) -> Tensor:
        return x.unflatten(self.dim, self.sizes)


class Interpolate(fl.Module):
    """To a fixed size; bilinear is torch's align_corners=False without antialiasing."""

    def __init__(self, size: tuple[int, ...], mode: str = "bilinear") -> None:
        super().__init__()
        self.size = Size(size)
        self.mode = mode

    def forward(self, x: Tensor) -> Tensor:
        return F.interpolate(x, size=self.size, mode=self.mode)


class Rescale(fl.Module):
    def __init__(self, scale_factor: float, mode: str = "nearest") -> None:
        super().__init__()
        self.scale_factor = scale_factor
        self.mode = mode

    def forward(self, x: Tensor) -> Tensor:
        return F.interpolate(x, scale_factor=self.scale_factor, mode=self.mode)


class BatchNorm2d(torch.nn.BatchNorm2d, fl.WeightedModule):
    def __init__(self, num_features: int, device: Any = None) -> None:
        super().__init__(num_features=num_features, device=device)


class PReLU(torch.nn.PReLU, fl.WeightedModule, fl.Activation):
    def __init__(self, device: Any = None) -> None:
        super().__init__(device=device)


class PatchSplit(fl.Chain):
    """(B, C, H, W) -> (B, 4, C, H / 2, W / 2), quadrant 2 qy + qx."""

    def __init__(self) -> None:
        super().__init__(Unflatten(-2, (2, -1)), Unflatten(-1, (2, -1)), fl.Permute(0, 2, 4, 1, 3, 5), fl.Flatten(1, 2))


class PatchMerge(fl.Chain):
    """(B, 4, C, H, W) -> (B, C, 2 H, 2 W): the inverse of PatchSplit."""

    def __init__(self) -> None:
        super().__init__(Unflatten(1, (2, 2)), fl.Permute(0, 3, 1, 4, 2, 5), fl.Flatten(-2, -1), fl.Flatten(-3, -2))


class FeedForward(fl.Residual):
    def __init__(self, emb_dim: int, device: Any = None) -> None:
        super().__init__(fl.Linear(emb_dim, 2 * emb_dim, device=device), fl.ReLU(), fl.Linear(2 * emb_dim, emb_dim, device=device))


class _GetArgs(fl.Parallel):
    """(queries, keys) stacked per view -> (q, k, v) of view n."""

    def __init__(self, n: int) -> None:
        super().__init__(*(fl.Chain(fl.GetArg(i), fl.Slicing(dim=0, start=n, end=n + 1), fl.Squeeze(0)) for i in (0, 1, 1)))


class MultiheadAttention(torch.nn.MultiheadAttention, fl.WeightedModule):
    """torch's own module: packed in_proj_weight [3E, E] + in_proj_bias, out_proj, sequence-first (L, B, E) tensors."""

    def __init__(self, embedding_dim: int, num_heads: int, device: Any = None) -> None:
        super().__init__(embed_dim=embedding_dim, num_heads=num_heads, device=device)

    @property
    def weight(self) -> Tensor:  # type: ignore[override]
        return self.in_proj_weight

    def forward(self, q: Tensor, k: Tensor, v: Tensor) -> Tensor:  # type: ignore[override]
        return super().forward(q, k, v)[0]


class PatchwiseCrossAttention(fl.Chain):
    """(4, L, B, E) queries and (4, L', B, E) keys -> (4, L, B, E): one MultiheadAttention, with weights of its own, per local view."""

    def __init__(self, d_model: int, num_heads: int, device: Any = None) -> None:
        super().__init__(
            fl.Concatenate(*(fl.Chain(_GetArgs(n), MultiheadAttention(d_model, num_heads, device=device)) for n in range(4))),
            Unflatten(0, (4, -1)),
        )


class Pool(fl.Module):
    def __init__(self, ratio: int) -> None:
        super().__init__()
        self.ratio = ratio

    def forward(self, x: Tensor) -> Tensor:
        b, _, h, w = x.shape
        assert h % self.ratio == 0 and w % self.ratio == 0
        return F.adaptive_avg_pool2d(x, (h // self.ratio, w // self.ratio)).unflatten(0, (b, -1))


class MultiPool(fl.Concatenate):
    """(B, E, H, W) -> (1, sum_r (H / r)(W / r), B, E): the average pools at every ratio as token rows, one after the other."""

    def __init__(self, pool_ratios: list[int]) -> None:
        super().__init__(*(fl.Chain(Pool(r), fl.Flatten(-2, -1), fl.Permute(0, 3, 1, 2)) for r in pool_ratios), dim=1)


# ---------------------------------------------------------------------------------------------------------------- MCLM
class PerPixel(fl.Chain):
    """(B, C, H, W) -> (H W, B, C)"""

    def __init__(self) -> None:
        super().__init__(fl.Permute(2, 3, 0, 1), fl.Flatten(0, 1))


class PositionEmbeddingSine(fl.Module):
    """DETR's fixed sine embedding of an h x w grid -> (h w, 1, 2 num_pos_feats) float32, columns (y features | x features)."""

    def __init__(self, num_pos_feats: int) -> None:
        super().__init__()
        i = torch.arange(0, num_pos_feats, dtype=torch.float32)
        self.dim_t = 10000 ** (2 * (i // 2) / num_pos_feats)

    def __call__(self, h: int, w: int) -> Tensor:
        ones = torch.ones([1, h, w, 1], dtype=torch.bool)
        y, x = ones.cumsum(dim=1, dtype=torch.float32), ones.cumsum(dim=2, dtype=torch.float32)
        y = (y - 0.5) / (y[:, -1:, :] + 1e-6) * (2 * math.pi)
        x = (x - 0.5) / (x[:, :, -1:] + 1e-6) * (2 * math.pi)
        px, py = x / self.dim_t, y / self.dim_t
        px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=4).flatten(3)
        py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=4).flatten(3)
        return torch.cat((py, px), dim=3).permute(1, 2, 0, 3).flatten(0, 1)


class MultiPoolPos(fl.Module):
    def __init__(self, pool_ratios: list[int], positional_embedding: PositionEmbeddingSine) -> None:
        super().__init__()
        self.pool_ratios = pool_ratios
        self.positional_embedding = positional_embedding

    def forward(self, *args: int) -> Tensor:
        h, w = args
        return torch.cat([self.positional_embedding(h // r, w // r) for r in self.pool_ratios])


class Repeat(fl.Module):
    """The position embedding repeated over the batch of `like` and cast to its dtype."""

    def __init__(self, dim: int = 0) -> None:
        self.dim = dim
        super().__init__()

    def forward(self, x: Tensor, like: Tensor) -> Tensor:
        return torch.repeat_interleave(x.to(like.dtype), like.size(self.dim), dim=self.dim)


class _MHA_Arg(fl.Sum):  # noqa: N801 -- (the reference's name)
    def __init__(self, offset: int) -> None:
        self.offset = offset
        super().__init__(
            fl.GetArg(offset),
            fl.Chain(fl.Parallel(fl.GetArg(offset + 1), fl.Lambda(self._value)), Repeat(1)),
        )

    def _value(self, *args: Tensor) -> Tensor:
        return args[self.offset]


class GlobalAttention(fl.Chain):
    """(global, its position embedding, pools, their position embedding) -> global + MHA(global + pos, pools + pos, pools)."""

    def __init__(self, emb_dim: int, num_heads: int = 1, device: Any = None) -> None:
        super().__init__(
            fl.Sum(
                fl.GetArg(0),
                fl.Chain(fl.Parallel(_MHA_Arg(0), _MHA_Arg(2), fl.GetArg(2)), MultiheadAttention(emb_dim, num_heads, device=device)),
            ),
        )


class MCLM(fl.Chain):
    """Multi-view complementary localization: (1, 5, E, 16, 16) -> (1, 5, E, 16, 16).  The global view attends to pools of the merged local
    views; each local view then attends to its quadrant of the refined global view.  Its two LayerNorms are each used twice."""

    def __init__(self, emb_dim: int, num_heads: int = 1, pool_ratios: list[int] | None = None, device: Any = None) -> None:
        pool_ratios = [2, 8, 16] if pool_ratios is None else pool_ratios
        pos = PositionEmbeddingSine(num_pos_feats=emb_dim // 2)
        ln1, ln2 = fl.LayerNorm(emb_dim, device=device), fl.LayerNorm(emb_dim, device=device)

        def proxy(m: fl.Module) -> fl.Module:  # the same LayerNorm a second time, without a second entry in the tree
            return fl.Lambda(lambda x: m(x))

        super().__init__(
            fl.Parallel(
                fl.Chain(
                    fl.Slicing(dim=1, start=4),
                    fl.Squeeze(1),
                    fl.Parallel(PerPixel(), fl.Chain(fl.Lambda(lambda x: x.shape[-2:]), pos)),
                ),
                fl.Chain(
                    fl.Slicing(dim=1, end=4),
                    fl.SetContext("mclm", "local"),
                    PatchMerge(),
                    fl.Parallel(
                        fl.Chain(MultiPool(pool_ratios), fl.Squeeze(0)),
                        fl.Chain(fl.Lambda(lambda x: x.shape[-2:]), MultiPoolPos(pool_ratios, pos)),
                    ),
                ),
            ),
            fl.Lambda(lambda t1, t2: (*t1, *t2)),
            fl.Converter(set_dtype=False),
            GlobalAttention(emb_dim, num_heads, device=device),
            ln1,
            FeedForward(emb_dim, device=device),
            ln2,
            fl.SetContext("mclm", "global"),
            fl.UseContext("mclm", "local"),
            fl.Flatten(-2, -1),
            fl.Permute(1, 3, 0, 2),
            fl.Residual(
                fl.Parallel(
                    fl.Identity(),
                    fl.Chain(fl.UseContext("mclm", "global"), Unflatten(0, (2, 8, 2, 8)), fl.Permute(0, 2, 1, 3, 4, 5), fl.Flatten(0, 1), fl.Flatten(1, 2)),
                ),
                PatchwiseCrossAttention(emb_dim, num_heads, device=device),
            ),
            proxy(ln1),
            FeedForward(emb_dim, device=device),
            proxy(ln2),
            fl.Concatenate(fl.Identity(), fl.Chain(fl.UseContext("mclm", "global"), fl.Unsqueeze(0))),
            Unflatten(1, (16, 16)),
            fl.Permute(3, 0, 4, 1, 2),
        )

    def init_context(self) -> Contexts:
        return {"mclm": {"global": None, "local": None}}


# ---------------------------------------------------------------------------------------------------------------- MCRM
class Multiply(fl.Chain):
    def __init__(self, o1: fl.Module, o2: fl.Module) -> None:
        super().__init__(o1, o2)

    def forward(self, *args: Tensor) -> Tensor:
        return torch.mul(self[0](*args), self[1](*args))


class TiledCrossAttention(fl.Chain):
    """(local (1, 4, E, S, S), global (1, E, S, S)) -> (1, 4, E, S, S): view v attends to quadrant v of the global view, pooled."""

    def __init__(self, emb_dim: int, dim: int, num_heads: int = 1, pool_ratios: list[int] | None = None, device: Any = None) -> None:
        pool_ratios = [1, 2, 4] if pool_ratios is None else pool_ratios
        super().__init__(
            fl.Distribute(
                fl.Chain(fl.Flatten(-2, -1), fl.Permute(1, 3, 0, 2)),
                fl.Chain(PatchSplit(), fl.Squeeze(0), MultiPool(pool_ratios)),
            ),
            fl.Sum(
                fl.Chain(fl.GetArg(0), fl.Permute(2, 1, 0, 3)),
                fl.Chain(PatchwiseCrossAttention(emb_dim, num_heads, device=device), fl.Permute(2, 1, 0, 3)),
            ),
            fl.LayerNorm(emb_dim, device=device),
            FeedForward(emb_dim, device=device),
            fl.LayerNorm(emb_dim, device=device),
            fl.Permute(0, 2, 3, 1),
            Unflatten(-1, (dim, dim)),
        )


class MCRM(fl.Chain):
    """Multi-view complementary refinement: (1, 5, E, S, S) -> (1, 5, E, S, S), S divisible by 8."""

    def __init__(self, emb_dim: int, size: int, num_heads: int = 1, pool_ratios: list[int] | None = None, device: Any = None) -> None:
        pool_ratios = [1, 2, 4] if pool_ratios is None else pool_ratios
        super().__init__(
            fl.Parallel(
                fl.Chain(fl.Slicing(dim=1, end=4)),
                fl.Chain(fl.Slicing(dim=1, start=4), fl.Squeeze(1)),
            ),
            fl.Parallel(
                Multiply(
                    fl.GetArg(0),
                    fl.Chain(fl.GetArg(1), fl.Conv2d(emb_dim, 1, 1, device=device), fl.Sigmoid(), Interpolate((size * 2, size * 2), "nearest"), PatchSplit()),
                ),
                fl.GetArg(1),
            ),
            fl.Parallel(
                TiledCrossAttention(emb_dim, size, num_heads, pool_ratios, device=device),
                fl.GetArg(1),
            ),
            fl.Concatenate(
                fl.GetArg(0),
                fl.Chain(
                    fl.Sum(fl.GetArg(1), fl.Chain(fl.GetArg(0), PatchMerge(), Interpolate((size, size), "nearest"))),
                    fl.Unsqueeze(1),
                ),
                dim=1,
            ),
        )


# ---------------------------------------------------------------------------------------------------------------- the network
class CBG(fl.Chain):
    """Conv3x3 + BatchNorm + erf-GELU"""

    def __init__(self, in_dim: int, out_dim: int | None = None, device: Any = None) -> None:
        out_dim = out_dim or in_dim
        super().__init__(fl.Conv2d(in_dim, out_dim, kernel_size=3, padding=1, device=device), BatchNorm2d(out_dim, device=device), fl.GeLU())


class CBR(fl.Chain):
    """Conv3x3 + BatchNorm + single-slope PReLU"""

    def __init__(self, in_dim: int, out_dim: int | None = None, device: Any = None) -> None:
        out_dim = out_dim or in_dim
        super().__init__(fl.Conv2d(in_dim, out_dim, kernel_size=3, padding=1, device=device), BatchNorm2d(out_dim, device=device), PReLU(device=device))


class SplitMultiView(fl.Chain):
    """(B, C, H, W) -> (B, 5, C, H / 2, W / 2): the four quadrants, then the image at half size."""

    def __init__(self) -> None:
        super().__init__(fl.Concatenate(PatchSplit(), fl.Chain(Rescale(scale_factor=0.5, mode="bilinear"), fl.Unsqueeze(1)), dim=1))


class ShallowUpscaler(fl.Chain):
    """(B, E, 256, 256) -> (B, E, 1024, 1024): two (nearest 2x, CBG) steps, the shallow image features added before each."""

    def __init__(self, embedding_dim: int = 128, device: Any = None) -> None:
        super().__init__(
            fl.Sum(fl.Identity(), fl.Chain(fl.UseContext("mvanet", "shallow"), Interpolate((256, 256)))),
            fl.Sum(
                fl.Chain(Rescale(2), CBG(embedding_dim, device=device)),
                fl.Chain(fl.UseContext("mvanet", "shallow"), Interpolate((512, 512))),
            ),
            Rescale(2),
            CBG(embedding_dim, device=device),
        )


def _lateral(index: int, width: int, embedding_dim: int, device: Any) -> fl.Chain:
    return fl.Chain(fl.GetArg(index), fl.Flatten(0, 1), CBR(width, embedding_dim, device=device), Unflatten(0, (-1, 5)))


class PyramidL5(fl.Chain):
    def __init__(self, embedding_dim: int = 128, device: Any = None) -> None:
        super().__init__(
            fl.GetArg(0),
            fl.Flatten(0, 1),
            CBR(1024, embedding_dim, device=device),
            Unflatten(0, (-1, 5)),
            MCLM(embedding_dim, device=device),
            fl.Flatten(0, 1),
            Interpolate((32, 32)),
        )


class PyramidL4(fl.Chain):
    def __init__(self, embedding_dim: int = 128, device: Any = None) -> None:
        super().__init__(
            fl.Sum(PyramidL5(embedding_dim=embedding_dim, device=device), _lateral(1, 512, embedding_dim, device)),
            MCRM(embedding_dim, 32, device=device),
            fl.Flatten(0, 1),
            CBR(embedding_dim, device=device),
            Interpolate((64, 64)),
        )


class PyramidL3(fl.Chain):
    def __init__(self, embedding_dim: int = 128, device: Any = None) -> None:
        super().__init__(
            fl.Sum(PyramidL4(embedding_dim=embedding_dim, device=device), _lateral(2, 256, embedding_dim, device)),
            MCRM(embedding_dim, 64, device=device),
            fl.Flatten(0, 1),
            CBR(embedding_dim, device=device),
            Interpolate((128, 128)),
        )


class PyramidL2(fl.Chain):
    def __init__(self, embedding_dim: int = 128, device: Any = None) -> None:
        embedding_dim = 128  # (the reference pins it here)
        super().__init__(
            fl.Sum(PyramidL3(embedding_dim=embedding_dim, device=device), _lateral(3, 128, embedding_dim, device)),
            MCRM(embedding_dim, 128, device=device),
            fl.Flatten(0, 1),
            CBR(embedding_dim, device=device),
            Interpolate((128, 128)),
        )


class Pyramid(fl.Chain):
    """The five Swin maps ((1, 5, C_i, S_i, S_i), deepest first) -> (1, 5, E, 128, 128): a feature pyramid whose levels are MCLM / MCRM blocks."""

    def __init__(self, embedding_dim: int = 128, device: Any = None) -> None:
        super().__init__(
            fl.Sum(PyramidL2(embedding_dim=embedding_dim, device=device), _lateral(4, 128, embedding_dim, device)),
            MCRM(embedding_dim, 128, device=device),
            fl.Flatten(0, 1),
            CBR(embedding_dim, device=device),
            Unflatten(0, (-1, 5)),
        )


class RearrangeMultiView(fl.Chain):
    """(B, 5, E, H, W) -> (B, E, 2 H, 2 W): the merged local views plus the upsampled global view, through three convolutions."""

    def __init__(self, embedding_dim: int = 128, device: Any = None) -> None:
        super().__init__(
            fl.Sum(
                fl.Chain(fl.Slicing(dim=1, end=4), PatchMerge()),
                fl.Chain(fl.Slicing(dim=1, start=4), fl.Squeeze(1), Interpolate((256, 256))),
            ),
            fl.Chain(
                CBR(embedding_dim, 384, device=device),
                CBR(384, device=device),
                fl.Conv2d(384, embedding_dim, kernel_size=3, padding=1, device=device),
            ),
        )


class ComputeShallow(fl.Passthrough):
    def __init__(self, embedding_dim: int = 128, device: Any = None) -> None:
        super().__init__(fl.Conv2d(3, embedding_dim, kernel_size=3, padding=1, device=device), fl.SetContext("mvanet", "shallow"))


class MVANet(fl.Chain):
    """`MVANet(...).eval()(image)`: (1, 3, 1024, 1024) -> logits (1, n_logits, 1024, 1024).  No other input shape runs."""

    def __init__(self, embedding_dim: int = 128, n_logits: int = 1, depths: list[int] | None = None, num_heads: list[int] | None = None,
                 window_size: int = 12, device: Any = None) -> None:
        depths = [2, 2, 18, 2] if depths is None else depths
        num_heads = [4, 8, 16, 32] if num_heads is None else num_heads
        super().__init__(
            ComputeShallow(embedding_dim=embedding_dim, device=device),
            SplitMultiView(),
            fl.Flatten(0, 1),
            SwinTransformer(embedding_dim=embedding_dim, depths=depths, num_heads=num_heads, window_size=window_size, device=device),
            fl.Distribute(*(Unflatten(0, (-1, 5)) for _ in range(5))),
            Pyramid(embedding_dim=embedding_dim, device=device),
            RearrangeMultiView(embedding_dim=embedding_dim, device=device),
            ShallowUpscaler(embedding_dim, device=device),
            fl.Conv2d(embedding_dim, n_logits, kernel_size=3, padding=1, device=device),
        )

    def init_context(self) -> Contexts:
        return {"mvanet": {"shallow": None}}
