"""Swin Transformer backbone (arXiv:2103.14030) as a Chain tree: the feature extractor of MVANet / `solutions.BoxSegmenter`.

Mirrors reference src/refiners/foundationals/swin/swin_transformer.py (same class names, child order and parameter names, hence
the same state-dict keys and repr -- checked against tests/golden/swin_keys.json).  Everything here is the unfused torch path,
which is also the CPU path and the fallback of the MI355X engine (refiners_amd/engine/swin.py lowers the same tree).

Shapes: (B, 3, S, S), square inputs only -> 4x4 patch convolution + LayerNorm -> (B, (S/4)^2, C) tokens -> per stage `depth` blocks of
window attention over ws x ws windows (every second block on the grid rolled by ws // 2, with the -100 shift mask) and an MLP, then
PatchMerging (2x2 neighbours -> 4C -> LayerNorm -> 2C).  The forward returns (stage_n, ..., stage_1, patch_embedding) as NCHW maps.

Three facts of the reference that the lowering has to honour as well:
  * a grid that is no multiple of ws is zero-padded AFTER the block's LayerNorm: the padded tokens are exact zero rows, their
    q / k / v are the projection's bias, and they take part in attention as keys (nothing masks them);
  * the shift mask is built on the padded, rolled grid: along each axis a position p has region id 0 for p < Sp - ws, 1 for
    p < Sp - ws // 2, else 2, and pairs of tokens whose (row id, column id) differ get -100 ADDED to their score (not -inf);
  * PatchMerging zero-pads an odd grid to even BEFORE its LayerNorm(4C); the 4C channel blocks are (y & 1, x & 1) = (0, 0), (1, 0), (0, 1), (1, 1).
"""
import functools
from math import isqrt
from typing import Any

import torch
import torch.nn.functional as F
from torch import Tensor, nn

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.tree import Contexts


def canonical_relative_position_index(window_size: int) -> Tensor:
    """[ws^2, ws^2] int64: entry (i, j) = (y_i - y_j + ws - 1) (2 ws - 1) + (x_i - x_j + ws - 1) for tokens i, j at (y, x) of a window.
    Checkpoints carry this buffer; the MI355X kernel computes it as arithmetic and refuses anything else."""
    t = torch.arange(window_size * window_size)
    y, x = t // window_size, t % window_size
    dy = y[:, None] - y[None, :] + window_size - 1
    dx = x[:, None] - x[None, :] + window_size - 1
    return dy * (2 * window_size - 1) + dx


def partition_windows(x: Tensor, window_size: int) -> Tensor:
    """(B, S, S, C) -> (B, (S / ws)^2, ws^2, C), windows in row-major order, tokens of a window in row-major order."""
    b, s, s2, c = x.shape
    assert s == s2 and s % window_size == 0
    n = s // window_size
    return x.view(b, n, window_size, n, window_size, c).transpose(2, 3).reshape(b, n * n, window_size * window_size, c)


def region_ids(side: int, window_size: int, device: Any = None) -> Tensor:
    """[side, side] ids 3 r(y) + r(x), r(p) = 0 for p < side - ws, 1 for p < side - ws // 2, else 2."""
    p = torch.arange(side, device=device)
    r = (p >= side - window_size).long() + (p >= side - window_size // 2).long()
    return 3 * r[:, None] + r[None, :]


@functools.cache
def shift_mask(side: int, window_size: int, device: Any = None) -> Tensor:
    """[(side / ws)^2, ws^2, ws^2] float32: -100 where two tokens of a window of the rolled grid come from different regions, else 0."""
    assert side % window_size == 0
    ids = partition_windows(region_ids(side, window_size, device).view(1, side, side, 1), window_size).squeeze()
    # (the squeeze is the reference's: a grid of ONE window loses its window axis here, and the reshape in WindowSDPA then raises)
    differ = ids.unsqueeze(1) != ids.unsqueeze(2)
    return torch.where(differ, -100.0, 0.0).to(torch.float32)


class ToWindows(fl.Module):
    def __init__(self, window_size: int) -> None:
        super().__init__()
        self.window_size = window_size

    def forward(self, x: Tensor) -> Tensor:
        return partition_windows(x, self.window_size)


class FromWindows(fl.Module):
    """(B, n^2, ws^2, C) -> (B, n ws, n ws, C): the inverse of ToWindows."""

    def forward(self, x: Tensor) -> Tensor:
        b, windows, tokens, c = x.shape
        ws, n = isqrt(tokens), isqrt(windows)
        return x.view(b, n, n, ws, ws, c).transpose(2, 3).reshape(b, n * ws, n * ws, c)


class Pad(fl.Module):
    """Zero-pad a square channels-last grid at the bottom / right to the next multiple of `step`."""

    def __init__(self, step: int) -> None:
        super().__init__()
        self.step = step

    def forward(self, x: Tensor) -> Tensor:
        assert x.shape[1] == x.shape[2]
        extra = -x.shape[1] % self.step
        return F.pad(x, (0, 0, 0, extra, 0, extra)) if extra else x


class StatefulPad(fl.Chain):
    """Pad that pushes the unpadded side onto a context list, for the StatefulUnpad further down the same Residual."""

    def __init__(self, context: str, key: str, step: int) -> None:
        super().__init__(
            fl.SetContext(context=context, key=key, callback=self._push),
            Pad(step=step),
        )

    def _push(self, sizes: list[int], x: Tensor) -> None:
        sizes.append(x.shape[1])


class StatefulUnpad(fl.Chain):
    def __init__(self, context: str, key: str) -> None:
        super().__init__(
            fl.Parallel(
                fl.Identity(),
                fl.UseContext(context=context, key=key).compose(lambda sizes: sizes.pop()),
            ),
            fl.Lambda(self._unpad),
        )

    @staticmethod
    def _unpad(x: Tensor, size: int) -> Tensor:
        return x[:, :size, :size, :]


class SquareUnflatten(fl.Module):
    """(..., L^2, ...) -> (..., L, L, ...) at `dim`."""

    def __init__(self, dim: int = 0) -> None:
        super().__init__()
        self.dim = dim

    def forward(self, x: Tensor) -> Tensor:
        side = isqrt(x.shape[self.dim])
        return x.unflatten(self.dim, (side, side))


class WindowUnflatten(fl.Module):
    """(..., H, ...) -> (..., H / ws, ws, ...) at `dim`."""

    def __init__(self, window_size: int, dim: int = 0) -> None:
        super().__init__()
        self.window_size = window_size
        self.dim = dim

    def forward(self, x: Tensor) -> Tensor:
        h = x.shape[self.dim]
        assert h % self.window_size == 0
        return x.unflatten(self.dim, (h // self.window_size, self.window_size))


class Roll(fl.Module):
    """torch.roll by (dim, shift) pairs."""

    def __init__(self, *shifts: tuple[int, int]) -> None:
        super().__init__()
        self.shifts = shifts
        self._dims = tuple(d for d, _ in shifts)
        self._shifts = tuple(s for _, s in shifts)

    def forward(self, x: Tensor) -> Tensor:
        return torch.roll(x, self._shifts, self._dims)


class RelativePositionBias(fl.Module):
    """The free (2 ws - 1)^2 x heads bias table and the index buffer that spreads it over the ws^2 x ws^2 token pairs.  Both are part
    of the state dict (empty until loaded, like the reference's)."""

    relative_position_index: Tensor

    def __init__(self, window_size: int, num_heads: int, device: Any = None, dtype: Any = None) -> None:
        super().__init__()
        side = 2 * window_size - 1
        self.relative_position_bias_table = nn.Parameter(torch.empty(side * side, num_heads, device=device, dtype=dtype))
        self.register_buffer("relative_position_index", torch.empty(window_size**2, window_size**2, device=device, dtype=torch.int64))

    def forward(self) -> Tensor:
        return self.relative_position_bias_table[self.relative_position_index].permute(2, 0, 1).unsqueeze(0)  # (1, heads, N, N)


class WindowSDPA(fl.Module):
    """Attention inside each window over a packed (B, windows, N, 3 C) tensor, columns ordered (3, heads, head_dim)."""

    def __init__(self, window_size: int, num_heads: int, shift: bool = False, device: Any = None, dtype: Any = None) -> None:
        super().__init__()
        self.window_size = window_size
        self.num_heads = num_heads
        self.shift = shift
        self.rpb = RelativePositionBias(window_size, num_heads, device=device, dtype=dtype)

    def forward(self, x: Tensor) -> Tensor:
        b, windows, n, c3 = x.shape
        assert c3 % (3 * self.num_heads) == 0
        c = c3 // 3
        q, k, v = x.reshape(b * windows, n, 3, self.num_heads, c // self.num_heads).permute(2, 0, 3, 1, 4)
        bias = self.rpb()
        if self.shift:
            mask = shift_mask(isqrt(windows * n), self.window_size, x.device).to(bias.dtype)
            bias = bias + mask.reshape(1, windows, 1, n, n).expand(b, -1, self.num_heads, -1, -1).reshape(-1, self.num_heads, n, n)
        y = F.scaled_dot_product_attention(q, k, v, bias)
        return y.transpose(1, 2).reshape(b, windows, n, c)


class WindowAttention(fl.Chain):
    """(S)W-MSA: one Linear for q | k | v, the windowed attention with its relative position bias, the output projection."""

    def __init__(self, dim: int, window_size: int, num_heads: int, shift: bool = False, device: Any = None, dtype: Any = None) -> None:
        super().__init__(
            fl.Linear(dim, dim * 3, bias=True, device=device, dtype=dtype),
            WindowSDPA(window_size, num_heads, shift, device=device, dtype=dtype),
            fl.Linear(dim, dim, device=device, dtype=dtype),
        )


class SwinTransformerBlock(fl.Chain):
    def __init__(self, dim: int, num_heads: int, window_size: int = 7, shift_size: int = 0, mlp_ratio: float = 4.0, device: Any = None, dtype: Any = None) -> None:
        assert 0 <= shift_size < window_size, "shift_size must in [0, window_size["
        hidden = int(dim * mlp_ratio)
        super().__init__(
            fl.Residual(
                fl.LayerNorm(dim, device=device, dtype=dtype),
                SquareUnflatten(1),
                StatefulPad(context="padding", key="sizes", step=window_size),
                Roll((1, -shift_size), (2, -shift_size)),
                ToWindows(window_size),
                WindowAttention(dim, window_size=window_size, num_heads=num_heads, shift=shift_size > 0, device=device, dtype=dtype),
                FromWindows(),
                Roll((1, shift_size), (2, shift_size)),
                StatefulUnpad(context="padding", key="sizes"),
                fl.Flatten(1, 2),
            ),
            fl.Residual(
                fl.LayerNorm(dim, device=device, dtype=dtype),
                fl.Linear(dim, hidden, device=device, dtype=dtype),
                fl.GeLU(),
                fl.Linear(hidden, dim, device=device, dtype=dtype),
            ),
        )

    def init_context(self) -> Contexts:
        return {"padding": {"sizes": []}}


class PatchMerging(fl.Chain):
    """2x2 neighbours of the (zero-padded to even) grid side by side -> LayerNorm(4 dim) -> Linear(4 dim -> 2 dim, no bias)."""

    def __init__(self, dim: int, device: Any = None, dtype: Any = None) -> None:
        super().__init__(
            SquareUnflatten(1),
            Pad(2),
            WindowUnflatten(2, 2),
            WindowUnflatten(2, 1),
            fl.Permute(0, 1, 3, 4, 2, 5),
            fl.Flatten(3),
            fl.Flatten(1, 2),
            fl.LayerNorm(4 * dim, device=device, dtype=dtype),
            fl.Linear(4 * dim, 2 * dim, bias=False, device=device, dtype=dtype),
        )


class BasicLayer(fl.Chain):
    """One stage: `depth` blocks, the odd ones shifted by ws // 2."""

    def __init__(self, dim: int, depth: int, num_heads: int, window_size: int = 7, mlp_ratio: float = 4.0, device: Any = None, dtype: Any = None) -> None:
        super().__init__(
            SwinTransformerBlock(dim=dim, num_heads=num_heads, window_size=window_size, shift_size=(i % 2) * (window_size // 2), mlp_ratio=mlp_ratio,
                                 device=device, dtype=dtype)
            for i in range(depth)
        )


class PatchEmbedding(fl.Chain):
    def __init__(self, patch_size: tuple[int, int] = (4, 4), in_chans: int = 3, embedding_dim: int = 96, device: Any = None, dtype: Any = None) -> None:
        super().__init__(
            fl.Conv2d(in_chans, embedding_dim, kernel_size=patch_size, stride=patch_size, device=device, dtype=dtype),
            fl.Flatten(2),
            fl.Transpose(1, 2),
            fl.LayerNorm(embedding_dim, device=device, dtype=dtype),
        )


class SwinTransformer(fl.Chain):
    """Swin backbone as MVANet uses it (square inputs only).  `swin(x)` -> (stage_n, ..., stage_1, patch_embedding), NCHW."""

    def __init__(self, patch_size: tuple[int, int] = (4, 4), in_chans: int = 3, embedding_dim: int = 96, depths: list[int] | None = None,
                 num_heads: list[int] | None = None, window_size: int = 7, mlp_ratio: float = 4.0, device: Any = None, dtype: Any = None) -> None:
        depths = [2, 2, 6, 2] if depths is None else depths
        num_heads = [3, 6, 12, 24] if num_heads is None else num_heads
        self.num_layers = len(depths)
        assert len(num_heads) == self.num_layers

        def stage(i: int) -> fl.Chain:
            width = int(embedding_dim * 2**i)
            return fl.Chain(
                BasicLayer(dim=width, depth=depths[i], num_heads=num_heads[i], window_size=window_size, mlp_ratio=mlp_ratio, device=device, dtype=dtype),
                fl.Passthrough(
                    fl.LayerNorm(width, device=device, dtype=dtype),
                    fl.Transpose(1, 2),
                    SquareUnflatten(2),
                    fl.SetContext("swin", "outputs", callback=lambda outputs, x: outputs.insert(0, x)),
                ),
                PatchMerging(dim=width, device=device, dtype=dtype) if i < self.num_layers - 1 else fl.UseContext("swin", "outputs").compose(lambda outputs: tuple(outputs)),
            )

        super().__init__(
            PatchEmbedding(patch_size=patch_size, in_chans=in_chans, embedding_dim=embedding_dim, device=device, dtype=dtype),
            fl.Passthrough(
                fl.Transpose(1, 2),
                SquareUnflatten(2),
                fl.SetContext("swin", "outputs", callback=lambda outputs, x: outputs.append(x)),
            ),
            *(stage(i) for i in range(self.num_layers)),
        )

    def init_context(self) -> Contexts:
        return {"swin": {"outputs": []}}
