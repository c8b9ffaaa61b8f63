"""MI355X lowering of InformativeDrawings, the lineart preprocessor (refiners_amd.latent_diffusion.preprocessors, or refiners' own class).

The Chain tree is walked once, by class name, into a launch program over channels-last pixel rows [B H W][C].  An activation is in one of the
three layouts of include/mi355x_refiners_lineart.h (ROWS, the interior of a PADDED image, QUAD), and three identities let every 3x3
convolution run on mi355x_gemm's zero-padded implicit-GEMM path unchanged:

  * reflection in front of a 3x3 convolution: conv_valid(reflect_pad1(x)) is the interior of conv_same_zero_pad(reflect_pad1(x)).  The apply
    kernel writes the (h + 2) x (w + 2) image with its reflected ring, the convolution runs over all of it, the next statistics / apply read
    the interior (PADDED, pad 1).  (1 + 2 / h)(1 + 2 / w) of the convolution's work, at quarter resolution only.
  * ConvTranspose2d(C -> C', 3, stride 2, padding 1, output_padding 1): output pixel (2a + py, 2b + px) reads inputs (a .. a + 1, b .. b + 1)
    only, so it is a zero-padded 3x3 convolution to 4 C' channels whose column group 2 py + px holds weight[:, :, ky, kx]^T at the taps on and
    to the right of / below the centre (pack_convt_phases).  Its output is the QUAD layout, un-shuffled by its readers' index arithmetic.
  * a bias in front of InstanceNorm2d(affine=False) cancels: every convolution but the last runs without its bias.

  stem                           mi355x_lineart_stem | in_stats | in_apply(ReLU)
  each of the two downsamples    convolution (stride 2) | in_stats | in_apply(ReLU); the second writes the reflected ring when a residual block follows
  each residual block            convolution over the ringed image | in_stats(PADDED) | in_apply(ReLU, ring 1) | convolution | in_stats(PADDED) |
                                 in_apply(+ block input, ring 1; the last block's writes ROWS)
  the two transposed convolutions  convolution to 4 C' | in_stats(QUAD) | in_apply(ReLU) for the first; convolution | in_stats(QUAD) for the second
  head                           mi355x_lineart_head: InstanceNorm2d + ReLU on the way into LDS, reflect-padded 7x7 to one channel, bias, Sigmoid

33 launches for the default three blocks, one graph replay.  Refused (Unsupported: the stock forward runs instead, behind a RuntimeWarning):
out_channels != 1, in_channels > 4, an InstanceNorm2d with affine parameters or running statistics, a tree of another shape.
"""
from __future__ import annotations

import warnings
from typing import Any, Optional

import torch
from torch import Tensor

from .. import native
from ..fluxion.tree import ChainError, tree_epoch
from .compiled import Program
from .lowering import Lowering
from .packing import Act, ConvSpec, PackCache, Unsupported, _expect, cname, isa, kids, launches

MAX_PROGRAMS = 8  # lowered shapes kept per CompiledInformativeDrawings


# ------------------------------------------------------------------------------------------------ host helpers
def reflect_index(n: int, p: int) -> Tensor:
    """Source index of every position of an axis of n padded by p on both sides, by ReflectionPad2d's rule (p < n): what the ring of the
    apply kernel and the halo loads of the stem and the head compute."""
    assert 0 <= p < n, f"a reflection of {p} needs an axis longer than {p}, got {n}"
    i = torch.arange(-p, n + p)
    i = i.abs()
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def pack_convt_phases(w: Tensor) -> Tensor:
    """ConvTranspose2d(C -> C', 3, stride 2, padding 1, output_padding 1) weight [C, C', 3, 3] -> the weight [4 C', C, 3, 3] of the zero-padded
    3x3 convolution whose output channel (2 py + px) C' + c' at pixel (a, b) is output pixel (2a + py, 2b + px), channel c'.
    Tap (1 + dy, 1 + dx) of phase (py, px) holds weight[:, :, ky, kx]^T with ky = 1 for py = 0 (dy = 0 only), ky = 2 for (py = 1, dy = 0),
    ky = 0 for (py = 1, dy = 1), and kx by the same rule; everything else is zero."""
    C, Cp, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    out = w.new_zeros(4, Cp, C, 3, 3)
    taps = {0: [(0, 1)], 1: [(0, 2), (1, 0)]}  # phase -> [(d, k)]
    for py in (0, 1):
        for px in (0, 1):
            for dy, ky in taps[py]:
                for dx, kx in taps[px]:
                    out[2 * py + px, :, :, 1 + dy, 1 + dx] = w[:, :, ky, kx].t()
    return out.reshape(4 * Cp, C, 3, 3)


def out_size(H: int, W: int) -> tuple[int, int]:
    """H' = 4 ceil(ceil(H / 2) / 2): two stride-2 convolutions round up, two transposed convolutions double."""
    q = lambda n: ((n + 1) // 2 + 1) // 2  # noqa: E731
    return 4 * q(H), 4 * q(W)


def check_size(H: int, W: int, n_residual_blocks: int) -> None:
    """The sizes the reference itself refuses, as the same kind of error, before anything is launched: ReflectionPad2d(3) needs H, W >= 4, a
    residual block's ReflectionPad2d(1) needs quarter-resolution sides >= 2, and InstanceNorm2d more than one pixel per image."""
    h, w = out_size(H, W)[0] // 4, out_size(H, W)[1] // 4
    if H < 4 or W < 4:
        raise ChainError(f"InformativeDrawings: ReflectionPad2d(3) needs an input of at least 4 x 4, got {H} x {W}")
    if h * w < 2 or (n_residual_blocks > 0 and (h < 2 or w < 2)):
        raise ChainError(f"InformativeDrawings: an input of {H} x {W} is {h} x {w} at quarter resolution, too small for "
                         + ("ReflectionPad2d(1)" if h * w >= 2 else "InstanceNorm2d"))


def _pad_of(node: Any) -> int:
    p = node.padding if isinstance(node.padding, (tuple, list)) else (node.padding,) * 4
    _expect(isa(node, "ReflectionPad2d") and len(set(p)) == 1, f"expected a uniform ReflectionPad2d, got {cname(node)}")
    return int(p[0])


def _pair(v: Any) -> tuple:
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


# ------------------------------------------------------------------------------------------------ lowering
class LineartLowering(Lowering):
    def lower(self, model: Any, image: Tensor, out: Tensor) -> None:
        """image [B, Cin, H, W] (static) -> out [B, 1, H', W'] (static)."""
        ch = kids(model)
        _expect(len(ch) >= 6 and all(isa(c, "Chain") for c in ch[:3] + ch[-3:]) and all(isa(c, "Residual") for c in ch[3:-3]), "unexpected InformativeDrawings layout")
        blocks = ch[3:-3]
        B, Cin, H, W = image.shape
        _expect(tuple(out.shape) == (B, 1) + out_size(H, W) and out.is_contiguous(), "output of another shape")
        self.gn_stats = False  # (no consumer of the convolutions' column statistics here: the general statistics kernel serves every size)
        # one float32 scratch for the statistics partials, shared by every statistics launch of the (sequential) program
        self._scratch = torch.empty(max(getattr(self, "_scratch_floats", 0), 4), device=self.device, dtype=torch.float32)
        self._keep: list = []
        with self.in_step():
            t, lay = self.stem(ch[0], image), (native.LINEART_ROWS, 0)
            a = self.norm(t, lay, kids(ch[0])[2], relu=True)
            self.pool.put(t.t)
            for i, down in enumerate(ch[1:3]):
                dc = kids(down)
                _expect(len(dc) == 3 and isa(dc[0], "Conv2d") and isa(dc[2], "ReLU"), "unexpected downsampling layout")
                t = self.conv3(a, dc[0], stride=2, padding=1)
                self.pool.put(a.t)
                a = self.norm(t, lay, dc[1], relu=True, ring=1 if (i == 1 and blocks) else 0)
                self.pool.put(t.t)
            for k, blk in enumerate(blocks):
                a = self.residual(blk, a, last=k == len(blocks) - 1)
            quad = (native.LINEART_QUAD, 0)
            uc = kids(ch[-3])
            _expect(len(uc) == 3 and isa(uc[2], "ReLU"), "unexpected upsampling layout")
            t = self.conv_transpose(a, uc[0])
            self.pool.put(a.t)
            a = self.norm(t, quad, uc[1], relu=True)
            self.pool.put(t.t)
            uc = kids(ch[-2])
            _expect(len(uc) == 3 and isa(uc[2], "ReLU"), "unexpected upsampling layout")
            t = self.conv_transpose(a, uc[0])
            self.pool.put(a.t)
            self.head(ch[-1], t, uc[1], out)
            self.pool.put(t.t)

    # ---------------------------------------------------------------------------------------------------------------
    def check_norm(self, node: Any, C: int) -> float:
        _expect(isa(node, "InstanceNorm2d"), f"expected an InstanceNorm2d, got {cname(node)}")
        _expect(not node.affine and not node.track_running_stats, "an InstanceNorm2d with affine parameters or running statistics (the convolution biases are dropped against a plain one)")
        _expect(node.num_features == C, f"InstanceNorm2d({node.num_features}) behind {C} channels")
        return float(node.eps)

    def in_stats(self, t: Act, lay: tuple[int, int], node: Any) -> Tensor:
        """The statistics table of the LOGICAL image `t` describes (t.t holds it in layout `lay`)."""
        C = t.C // 4 if lay[0] == native.LINEART_QUAD else t.C
        eps = self.check_norm(node, C)
        tab = torch.empty(t.B, C, 2, device=self.device, dtype=torch.float32)
        self._keep.append(tab)
        native.lineart_in_stats(t.t, t.B, t.H, t.W, C, eps, tab, layout=lay[0], pad=lay[1], ws=self._scratch)
        return tab

    def norm(self, t: Act, lay: tuple[int, int], node: Any, relu: bool, ring: int = 0, res: Optional[Tensor] = None, res_pad: int = 0) -> Act:
        """InstanceNorm2d [+ ReLU] [+ res] of the logical image of `t` -> a ROWS activation, or with ring > 0 the image with its reflected ring
        (an Act of (H + 2 ring) x (W + 2 ring): what the next convolution runs over)."""
        tab = self.in_stats(t, lay, node)
        C = tab.shape[1]
        out = self.pool.get(native.lineart_rows(t.B, t.H, t.W, native.LINEART_PADDED, ring), C)
        native.lineart_in_apply(t.t, t.B, t.H, t.W, C, tab, out, layout=lay[0], pad=lay[1], relu=relu, res=res, res_pad=res_pad, ring=ring)
        return Act(out, t.B, t.H + 2 * ring, t.W + 2 * ring)

    def stem(self, node: Any, image: Tensor) -> Act:
        sc = kids(node)
        _expect(len(sc) == 4 and isa(sc[1], "Conv2d") and isa(sc[3], "ReLU") and _pad_of(sc[0]) == 3, "unexpected initial convolution layout")
        conv = sc[1]
        B, Cin, H, W = image.shape
        _expect(tuple(conv.weight.shape) == (64, Cin, 7, 7) and _pair(conv.stride) == (1, 1) and _pair(conv.padding) == (0, 0) and _pair(conv.dilation) == (1, 1) and conv.groups == 1,
                "unexpected initial convolution")
        _expect(Cin <= native.LINEART_MAX_CIN, f"in_channels {Cin} (the stem kernel holds the weights of up to {native.LINEART_MAX_CIN} in LDS)")
        self.check_norm(sc[2], 64)  # (before the bias is dropped)
        w = self.cache.get(("lineart_stem_w",) + PackCache.ident(conv.weight), lambda: native.lineart_pack_stem(conv.weight).to(self.device))
        out = self.pool.get(B * H * W, 64)
        native.lineart_stem(image, w, None, out)
        return Act(out, B, H, W)

    def conv_weight(self, w: Tensor, tag: str, pack: Any) -> Tensor:
        return self.cache.get((tag,) + PackCache.ident(w), lambda: native.pack_conv_weight(pack(w.detach().float()).to(self.device, self.dtype)))

    def conv3(self, a: Act, conv: Any, stride: int, padding: int) -> Act:
        """A 3x3 Conv2d over the image of `a` on the zero-padded implicit-GEMM path, without its bias (an InstanceNorm2d follows)."""
        C = a.C
        _expect(isa(conv, "Conv2d") and tuple(conv.weight.shape)[1:] == (C, 3, 3) and _pair(conv.stride) == (stride, stride) and _pair(conv.padding) == (padding, padding)
                and _pair(conv.dilation) == (1, 1) and conv.groups == 1 and getattr(conv, "padding_mode", "zeros") == "zeros", f"unexpected 3x3 convolution {conv!r}")
        wp = self.conv_weight(conv.weight, "lineart_convw", lambda w: w)
        return self.conv(a, ConvSpec(wp, None, C, conv.weight.shape[0], 3, stride), bias=None)

    def conv_transpose(self, a: Act, conv: Any) -> Act:
        """ConvTranspose2d(3, stride 2, padding 1, output_padding 1) of a ROWS activation as a 3x3 convolution to 4 C' channels: an Act of the
        logical 2 H x 2 W image whose tensor is in QUAD layout."""
        C = a.C
        _expect(isa(conv, "ConvTranspose2d") and tuple(conv.weight.shape)[0] == C and tuple(conv.weight.shape)[2:] == (3, 3) and _pair(conv.stride) == (2, 2)
                and _pair(conv.padding) == (1, 1) and _pair(conv.output_padding) == (1, 1) and _pair(conv.dilation) == (1, 1) and conv.groups == 1, f"unexpected transposed convolution {conv!r}")
        Cp = conv.weight.shape[1]
        wp = self.conv_weight(conv.weight, "lineart_convt", pack_convt_phases)
        t = self.conv(a, ConvSpec(wp, None, C, 4 * Cp, 3, 1), bias=None)
        return Act(t.t, a.B, 2 * a.H, 2 * a.W)

    def residual(self, blk: Any, a: Act, last: bool) -> Act:
        """`a`: the block's input with its reflected ring, (h + 2) x (w + 2).  Returns the block's output, ringed again, or as ROWS for the last."""
        rc = kids(blk)
        _expect(len(rc) == 7 and _pad_of(rc[0]) == 1 and _pad_of(rc[4]) == 1 and isa(rc[3], "ReLU"), "unexpected residual block layout")
        h, w = a.H - 2, a.W - 2
        inner = (native.LINEART_PADDED, 1)
        t = self.conv3(a, rc[1], stride=1, padding=0)  # over the ringed image: its interior is the valid convolution
        m = self.norm(Act(t.t, a.B, h, w), inner, rc[2], relu=True, ring=1)
        self.pool.put(t.t)
        t = self.conv3(m, rc[5], stride=1, padding=0)
        self.pool.put(m.t)
        o = self.norm(Act(t.t, a.B, h, w), inner, rc[6], relu=False, ring=0 if last else 1, res=a.t, res_pad=1)
        self.pool.put(t.t)
        self.pool.put(a.t)
        return o

    def head(self, node: Any, t: Act, norm: Any, out: Tensor) -> None:
        hc = kids(node)
        _expect(len(hc) == 3 and isa(hc[1], "Conv2d") and isa(hc[2], "Sigmoid") and _pad_of(hc[0]) == 3, "unexpected output layer layout")
        conv = hc[1]
        _expect(t.C == 256, f"{t.C // 4} channels in front of the output layer (the head kernel takes 64)")
        _expect(conv.weight.shape[0] == 1, f"out_channels {conv.weight.shape[0]} (the head kernel contracts to one channel)")
        _expect(tuple(conv.weight.shape) == (1, 64, 7, 7) and _pair(conv.stride) == (1, 1) and _pair(conv.padding) == (0, 0) and _pair(conv.dilation) == (1, 1), "unexpected output convolution")
        tab = self.in_stats(t, (native.LINEART_QUAD, 0), norm)
        w = self.cache.get(("lineart_head_w",) + PackCache.ident(conv.weight), lambda: native.lineart_pack_head(conv.weight).to(self.device))
        bias = 0.0 if conv.bias is None or self.device.type == "meta" else self.cache.get(("lineart_head_b",) + PackCache.ident(conv.bias), lambda: float(conv.bias.detach().float().item()))
        native.lineart_head(t.t, t.B, t.H, t.W, tab, w, bias, out, layout=native.LINEART_QUAD)


def scratch_floats(B: int, H: int, W: int) -> int:
    """The largest statistics scratch a program of this input size asks for (lowering order: full, half, quarter resolution, then QUAD)."""
    h1, w1 = (H + 1) // 2, (W + 1) // 2
    h2, w2 = (h1 + 1) // 2, (w1 + 1) // 2
    need = [native.lineart_in_stats_ws_floats(B, H, W, 64), native.lineart_in_stats_ws_floats(B, h1, w1, 128), native.lineart_in_stats_ws_floats(B, h2, w2, 256),
            native.lineart_in_stats_ws_floats(B, 2 * h2, 2 * w2, 128, native.LINEART_QUAD), native.lineart_in_stats_ws_floats(B, 4 * h2, 4 * w2, 64, native.LINEART_QUAD)]
    return max(need)


def lower(model: Any, image: Tensor, out: Tensor, cache: Optional[PackCache] = None) -> LineartLowering:
    low = LineartLowering(image.device, image.dtype, cache, "merged")
    low._scratch_floats = scratch_floats(image.shape[0], image.shape[2], image.shape[3]) if image.device.type != "meta" else 4
    low.lower(model, image, out)
    return low


class _Entry:
    """One lowered shape: its static input / output buffers, lowering and program."""

    def __init__(self, x: Tensor, out: Tensor, low: LineartLowering, program: Program) -> None:
        self.x, self.out, self.low, self.program = x, out, low, program


class CompiledInformativeDrawings:
    """`fast = CompiledInformativeDrawings(model); y = fast(image)` == `model(image)`: [B, in_channels, H, W] -> [B, 1, H', W'], H' = 4 ceil(ceil(H / 2) / 2).
    One lowered program and one HIP graph per (B, H, W, dtype), the last MAX_PROGRAMS kept: a repeat call of a shape replays its graph.  `dtype`
    (default: the tree's) is the compute dtype.  An in-place edit of a weight re-lowers (only what changed is re-packed).  A size the model itself
    refuses raises before anything is launched; a tree the lowering does not cover runs its stock forward behind a RuntimeWarning
    (`stats["whole_fallback"]`)."""

    def __init__(self, model: Any, use_graph: bool = True, dtype: Optional[torch.dtype] = None) -> None:
        native.load()
        self.model = model
        self.dtype = dtype
        self.use_graph = use_graph
        self.cache = PackCache()
        self.entries: dict[Any, _Entry] = {}
        self.version: Any = None
        self.bad_keys: set = set()
        self.lowerings = 0
        self.stats: dict[str, Any] = {"fallback_nodes": [], "step_ops": 0, "whole_fallback": False}
        self.program: Optional[Program] = None

    def _tree_dtype(self) -> torch.dtype:
        return next(p.dtype for p in self.model.parameters())

    def _weights_version(self) -> tuple:
        """Every program holds packed copies of the weights: an in-place edit of any of them, or a change of the tree, drops the programs."""
        return (tree_epoch(), sum(p._version for p in self.model.parameters()))

    @torch.no_grad()
    def __call__(self, image: Tensor) -> Tensor:
        dtype = self.dtype or self._tree_dtype()
        version = self._weights_version()
        edited = version != self.version
        if edited:  # every program goes; the first lowering after it sweeps the packs nothing uses any more
            self.entries.clear()
            self.bad_keys.clear()
            self.cache.used.clear()
            self.version = version
        key = (tuple(image.shape), dtype, image.device)
        if key in self.bad_keys:
            return self._stock(image)
        e = self.entries.get(key)
        if e is None:
            try:
                _expect(image.dim() == 4, f"input of shape {tuple(image.shape)}")
                B, _c, H, W = image.shape
                check_size(H, W, sum(1 for c in kids(self.model) if isa(c, "Residual")))
                x = torch.empty(tuple(image.shape), device=image.device, dtype=dtype)
                out = torch.empty((B, 1) + out_size(H, W), device=image.device, dtype=dtype)
                low = lower(self.model, x, out, self.cache)
            except Unsupported as err:
                warnings.warn(f"CompiledInformativeDrawings: {err}; running the stock forward", RuntimeWarning, stacklevel=2)
                self.bad_keys.add(key)
                return self._stock(image)
            if edited:  # (a further shape of the same weights adds packs and must not sweep the other programs' away)
                self.cache.sweep()
            self.lowerings += 1
            e = _Entry(x, out, low, Program(low.step, self.use_graph, low=low))
            while len(self.entries) >= MAX_PROGRAMS:
                self.entries.pop(next(iter(self.entries)))
            self.entries[key] = e
        self.program = e.program
        self.stats = dict(e.low.stats, step_ops=launches(e.low.step), pool_bytes=e.low.step_pool.bytes(), lowerings=self.lowerings, whole_fallback=False)
        e.x.copy_(image)
        e.program.run()
        return e.out.clone()

    def _stock(self, image: Tensor) -> Tensor:
        self.program = None
        self.stats = {"fallback_nodes": [cname(self.model)], "step_ops": 0, "whole_fallback": True, "lowerings": self.lowerings}
        return self.model(image.to(self._tree_dtype()))
