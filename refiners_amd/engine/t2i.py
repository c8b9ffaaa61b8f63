"""MI355X lowering of the T2I-Adapter's condition encoder (refiners_amd.latent_diffusion.t2i ConditionEncoder / ConditionEncoderXL, or
refiners' own classes): the conv net that turns the conditioning picture into the four feature maps the UNet's T2IFeatures taps add.

The Chain tree is walked once, by class name, into a launch program over channels-last pixel rows [B h w][C]:

  PixelUnshuffle(r) + Conv2d 3x3      mi355x_t2i_stem: one launch straight off the NCHW picture, the unshuffled tensor is never written
  Downsample2d                        mi355x_t2i_pool
  the 1x1 shortcut of a stage         one mi355x_gemm
  ResidualBlock                       x + conv1x1(relu(conv3x3(x))): the implicit-GEMM convolution with the ReLU epilogue, then the 1x1
                                      convolution as a GEMM with the block's input as its residual operand
  each stage's output                 mi355x_nhwc_to_nchw into the NCHW map the adapter hands to the UNet

1 + 2 * blocks + shortcuts + pools + 4 launches (24 for the default SDXL encoder), one graph replay.  Refused (Unsupported: the stock forward
runs instead, behind a RuntimeWarning): a tree of another shape, a downscale factor other than 8 or 16, in_channels other than 1 or 3, a
picture side the factor does not divide, channel counts whose rows are not whole 128-byte blocks.
"""
from __future__ import annotations

from typing import Any, Optional

import torch
from torch import Tensor

from .. import native
from ..fluxion.tree import tree_epoch
from .lowering import Lowering
from .packing import Act, PackCache, _expect, cname, isa, kids
from .program import MAX_PROGRAMS, Entry, HasPrograms, ProgramCache


def _pair(v: Any) -> tuple:
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def stage_plan(encoder: Any) -> tuple[int, int, list[tuple[int, bool]]]:
    """(downscale factor, in_channels, [(channels, downsamples) per stage]) of a condition encoder, from the tree alone."""
    ch = kids(encoder)
    _expect(isa(encoder, "ConditionEncoder", "ConditionEncoderXL") and len(ch) == 7 and isa(ch[0], "PixelUnshuffle") and isa(ch[1], "Conv2d")
            and all(isa(c, "StatefulResidualBlocks") for c in ch[2:6]) and isa(ch[6], "UseContext"), f"unexpected condition encoder layout ({cname(encoder)})")
    r = int(ch[0].downscale_factor)
    stages = []
    for st in ch[2:6]:
        sc = kids(st)
        _expect(len(sc) == 2 and isa(sc[0], "ResidualBlocks") and isa(sc[1], "SetContext") and len(kids(sc[0])) == 3, "unexpected StatefulResidualBlocks layout")
        pre, short, chain = kids(sc[0])
        blocks = kids(chain)
        _expect(isa(pre, "AvgPool2d", "Identity") and isa(short, "Conv2d", "Identity") and isa(chain, "Chain") and all(isa(b, "Residual") for b in blocks), "unexpected ResidualBlocks layout")
        width = short.weight.shape[0] if isa(short, "Conv2d") else (kids(blocks[0])[0].weight.shape[0] if blocks else ch[1].weight.shape[0])
        stages.append((int(width), isa(pre, "AvgPool2d")))
    return r, ch[1].weight.shape[1] // (r * r), stages


def feature_shapes(encoder: Any, B: int, Hp: int, Wp: int) -> list[tuple[int, int, int, int]]:
    r, _cin, stages = stage_plan(encoder)
    _expect(r in (8, 16), f"downscale factor {r} (the stem kernel takes 8 or 16)")
    _expect(Hp % r == 0 and Wp % r == 0 and Hp >= r and Wp >= r, f"a {Hp} x {Wp} picture is not a multiple of the downscale factor {r}")
    h, w, out = Hp // r, Wp // r, []
    for width, down in stages:
        if down:
            _expect(h >= 2 and w >= 2, f"a {h} x {w} map cannot be downsampled")
            h, w = h // 2, w // 2
        out.append((B, width, h, w))
    return out


class T2ILowering(Lowering):
    def lower(self, encoder: Any, picture: Tensor, outs: list[Tensor]) -> None:
        """picture [B, cin, r h, r w] (static) -> outs: the four NCHW contiguous feature maps (static)."""
        B, cin, Hp, Wp = picture.shape
        shapes = feature_shapes(encoder, B, Hp, Wp)
        r, cin_tree, stages = stage_plan(encoder)
        _expect(cin == cin_tree and cin in (1, 3), f"in_channels {cin_tree} with a picture of {cin} (the stem kernel takes 1 or 3)")
        _expect([tuple(o.shape) for o in outs] == shapes and all(o.is_contiguous() for o in outs), "outputs of another shape")
        ch = kids(encoder)
        conv = ch[1]
        C0 = conv.weight.shape[0]
        _expect(tuple(conv.weight.shape) == (C0, cin * r * r, 3, 3) and _pair(conv.stride) == (1, 1) and _pair(conv.padding) == (1, 1) and _pair(conv.dilation) == (1, 1)
                and conv.groups == 1 and getattr(conv, "padding_mode", "zeros") == "zeros", "unexpected first convolution")
        for width in [C0] + [s[0] for s in stages]:
            _expect((width * self.es) % 128 == 0, f"{width} channels are not whole 128-byte blocks")
        self.gn_stats = False  # (no GroupNorm reads these convolutions' outputs)
        with self.in_step():
            wp = self.cache.get(("t2i_stem_w", r, self.dtype) + PackCache.ident(conv.weight), lambda: native.t2i_pack_stem(conv.weight, r, self.dtype).to(self.device))
            a = Act(self.pool.get(B * (Hp // r) * (Wp // r), C0), B, Hp // r, Wp // r)
            native.t2i_stem(picture, wp, self._w(conv.bias), a.t, r)
            for node, out in zip(ch[2:6], outs):
                a = self.stage(kids(node)[0], a)
                native.nhwc_to_nchw(a.tokens(), out, a.C)
            self.pool.put(a.t)

    def stage(self, node: Any, a: Act) -> Act:
        pre, short, chain = kids(node)
        if isa(pre, "AvgPool2d"):
            _expect(_pair(pre.kernel_size) == (2, 2) and _pair(pre.stride) == (2, 2) and _pair(pre.padding) == (0, 0) and not pre.ceil_mode, f"unexpected downsampling {pre!r}")
            o = Act(self.pool.get(a.B * (a.H // 2) * (a.W // 2), a.C), a.B, a.H // 2, a.W // 2)
            native.t2i_pool(a.t, a.B, a.H, a.W, o.t)
            self.pool.put(a.t)
            a = o
        if isa(short, "Conv2d"):
            _expect(short.weight.shape[1] == a.C and _pair(short.padding) == (0, 0), "unexpected shortcut convolution")
            t = self.linear(a.t, self.linear_spec(short))
            self.pool.put(a.t)
            a = Act(t, a.B, a.H, a.W)
        for blk in kids(chain):
            a = self.block(blk, a)
        return a

    def block(self, blk: Any, a: Act) -> Act:
        """x + conv1x1(relu(conv3x3(x))): the ReLU is the convolution's epilogue, the sum the 1x1 GEMM's residual operand."""
        rc = kids(blk)
        _expect(len(rc) == 3 and isa(rc[0], "Conv2d") and isa(rc[1], "ReLU") and isa(rc[2], "Conv2d"), "unexpected ResidualBlock layout")
        spec = self.conv_spec(rc[0])
        _expect(spec.ksize == 3 and spec.stride == 1 and spec.lora is None and spec.time is None and spec.cin == a.C and spec.cout == a.C, f"unexpected 3x3 convolution {rc[0]!r}")
        _expect(rc[2].weight.shape[:2] == (a.C, a.C) and _pair(rc[2].padding) == (0, 0), f"unexpected 1x1 convolution {rc[2]!r}")
        t = self.pool.get(a.M, a.C)
        native.conv_gemm([(a.image(), self.kblocked(spec.w), 3, 1, 1, 0)], t, a.B, a.H, a.W, bias=spec.b, relu=True)
        o = self.linear(t, self.linear_spec(rc[2]), res=a.t)
        self.pool.put(t)
        self.pool.put(a.t)
        return Act(o, a.B, a.H, a.W)


def lower(encoder: Any, picture: Tensor, outs: list[Tensor], dtype: Optional[torch.dtype] = None, cache: Optional[PackCache] = None) -> T2ILowering:
    low = T2ILowering(picture.device, dtype or outs[0].dtype, cache, "merged")
    low.lower(encoder, picture, outs)
    return low


class CompiledT2IConditionEncoder(HasPrograms):
    """`fast = CompiledT2IConditionEncoder(adapter.condition_encoder); features = fast(condition)` == `adapter.compute_condition_features(condition)`:
    [B, in_channels, H, W] -> the tuple of four NCHW contiguous feature maps that `adapter.set_condition_features` and
    `CompiledUNet.set_inputs(t2i_features=)` take.  One lowered program and one HIP graph per (B, H, W, dtype), the last MAX_PROGRAMS kept.
    `dtype` (default: the tree's) is the compute dtype; a float32 picture is read as it is.  A tree or a picture size the lowering does not
    cover runs the stock forward behind a RuntimeWarning (`stats["whole_fallback"]`)."""

    def __init__(self, encoder: Any, use_graph: bool = True, dtype: Optional[torch.dtype] = None) -> None:
        native.load()
        self.encoder = encoder
        self.dtype = dtype
        self.use_graph = use_graph
        self.programs = ProgramCache("CompiledT2IConditionEncoder", MAX_PROGRAMS, fallback=True)
        self.stats: dict[str, Any] = {"fallback_nodes": [], "step_ops": 0, "whole_fallback": False}

    def _tree_dtype(self) -> torch.dtype:
        return next(p.dtype for p in self.encoder.parameters())

    def _weights_version(self) -> tuple:
        """Every program holds packed copies of the weights: an in-place edit of any of them, or a change of the tree, drops the programs."""
        return (tree_epoch(), sum(p._version for p in self.encoder.parameters()))

    @torch.no_grad()
    def __call__(self, condition: Tensor) -> tuple[Tensor, ...]:
        dtype = self.dtype or self._tree_dtype()

        def build(cache: PackCache) -> Entry:
            _expect(condition.dim() == 4, f"input of shape {tuple(condition.shape)}")
            B, _c, Hp, Wp = condition.shape
            shapes = feature_shapes(self.encoder, B, Hp, Wp)
            e = Entry(use_graph=self.use_graph)
            e.x = torch.empty(tuple(condition.shape), device=condition.device, dtype=torch.float32 if condition.dtype == torch.float32 else dtype)
            e.outs = [torch.empty(s, device=condition.device, dtype=dtype) for s in shapes]
            e.low = lower(self.encoder, e.x, e.outs, dtype, cache)
            return e

        e = self.programs.get(self._weights_version(), (tuple(condition.shape), condition.dtype, dtype, condition.device), build)
        if e is None:
            return self._stock(condition)
        self.stats = dict(e.stats, lowerings=self.lowerings, whole_fallback=False)
        e.x.copy_(condition)
        e.program.run()
        return tuple(o.clone() for o in e.outs)

    def _stock(self, condition: Tensor) -> tuple[Tensor, ...]:
        self.stats = {"fallback_nodes": [cname(self.encoder)], "step_ops": 0, "whole_fallback": True, "lowerings": self.lowerings}
        return tuple(self.encoder(condition.to(self._tree_dtype())))
