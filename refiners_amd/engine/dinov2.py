"""MI355X lowering of the DINOv2 encoder (refiners_amd.dinov2, or refiners' own foundationals.dinov2 classes).

Same engine as the SAM ViT and Swin: the Chain tree is walked once, by class name, into a launch program over channels-last token rows.
Every image owns Tp = T rounded up to 64 rows of the token matrix [B * Tp, D], T = 1 + registers + n: the padding rows are written as
zeros by the token kernel, take part as queries only (the attention kernel masks keys >= T) and are cut off the result.  With 64-row
samples the three projections are ONE launch that stores V transposed, whatever T is.

  prologue (once per lowered shape, again after an edit of the table):
    mi355x_dinov2_pos_resample   the patch part of the position table [M * M, D] -> float32 [h * w, D], a separable filter whose tap
                                 tables (bicubic A = -0.75 | antialiased bicubic A = -0.5 | bilinear) are built here in float64
  step (the input is copied into the program's static image cropped to whole patches, as the strided convolution reads it):
    patchify | ONE patch GEMM over all B * n rows (bias; K = 3 * 14 * 14 = 588 zero-padded to the K block)
    mi355x_dinov2_tokens         class row + position 0 | register rows | patch rows + resampled positions | zero rows
    per TransformerLayer         LayerNorm folded into the Q|K|V GEMM (the first layer's is a launch: nothing produced its row
                                 statistics) | mi355x_attention_general, non-causal, Lk = T | out-projection + residual with LayerScale
                                 folded into its weight rows and bias | LayerNorm folded into FF1 + erf-GELU epilogue (or the GEGLU
                                 epilogue, or a plain FF1 and mi355x_glu_silu) | FF2 + residual with LayerScale folded
    final LayerNorm

LayerScale: res + g * (x W^T + b) = res + x (diag(g) W)^T + g b, formed in float32 before the cast; the pack is keyed on the LayerScale weight
too, so an in-place edit re-packs.

Refused (Unsupported: the stock forward runs instead, behind a RuntimeWarning): an interpolation mode other than bicubic / bilinear, an
activation other than GELU, GLU(SiLU()) or GLU(GeLU()), a head dim that is no multiple of 8 or above 160, widths that are no multiple of
the GEMM K block, LoRA on a Linear, inputs smaller than one patch.
"""
from __future__ import annotations

import math
import warnings
from typing import Any, Optional

import numpy as np
import torch
from torch import Tensor

from .. import native
from ..fluxion.tree import tree_epoch
from .compiled import Program
from .lowering_blocks import BlockLowering as Lowering
from .packing import LinSpec, PackCache, Unsupported, _expect, cname, isa, kids, launches

MODES = ("bicubic", "bilinear")
MAX_PROGRAMS = 8  # lowered shapes kept per CompiledDINOv2


# ------------------------------------------------------------------------------------------------ tap tables (host, float64)
def _cubic(x: float, A: float) -> float:
    x = abs(x)
    if x <= 1.0:
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * A
    return 0.0


def _triangle(x: float) -> float:
    return max(0.0, 1.0 - abs(x))


def axis_taps(n_in: int, n_out: int, mode: str, antialias: bool) -> list[tuple[int, list[float]]]:
    """Per output index (first source index, weights of consecutive source indices) of torch.nn.functional.interpolate(mode=mode,
    align_corners=False, antialias=antialias) along one axis, weights in float64.  Indices torch clamps at the border are merged into the border tap;
    taps of weight exactly 0 at either end are dropped (the native grid is then ONE tap of weight 1: the identity, bit for bit)."""
    assert mode in MODES and n_in >= 1 and n_out >= 1
    # torch takes the source coordinate in float32 (scale = float(n_in) / n_out, then scale * (i + 0.5) - 0.5): at 37 cells the rounding of
    # that coordinate moves a weight by 1e-6, so the coordinate is taken the same way here; everything after it is float64
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    taps = []
    for i in range(n_out):
        acc: dict[int, float] = {}
        if antialias:
            half = 2.0 if mode == "bicubic" else 1.0
            support = f32(half) * scale if scale >= 1 else f32(half)
            inv = float(f32(1.0) / scale) if scale >= 1 else 1.0
            center = scale * f32(i + 0.5)
            lo = max(int(center - support + f32(0.5)), 0)
            hi = min(int(center + support + f32(0.5)), n_in)
            ws = [(_cubic((j - float(center) + 0.5) * inv, -0.5) if mode == "bicubic" else _triangle((j - float(center) + 0.5) * inv)) for j in range(lo, hi)]
            total = sum(ws)
            for j, wv in zip(range(lo, hi), ws):
                acc[j] = wv / total
        elif mode == "bicubic":
            src = scale * f32(i + 0.5) - f32(0.5)
            i0 = math.floor(src)
            t = float(src - f32(i0))
            for k, wv in zip(range(i0 - 1, i0 + 3), (_cubic(t + 1.0, -0.75), _cubic(t, -0.75), _cubic(1.0 - t, -0.75), _cubic(2.0 - t, -0.75))):
                j = min(max(k, 0), n_in - 1)
                acc[j] = acc.get(j, 0.0) + wv
        else:
            src = max(scale * f32(i + 0.5) - f32(0.5), f32(0.0))
            i0 = min(math.floor(src), n_in - 1)
            i1 = min(i0 + 1, n_in - 1)
            l1 = float(src - f32(i0))
            acc[i0] = acc.get(i0, 0.0) + 1.0 - l1
            acc[i1] = acc.get(i1, 0.0) + l1
        lo, hi = min(acc), max(acc)
        ws = [acc.get(j, 0.0) for j in range(lo, hi + 1)]
        while len(ws) > 1 and ws[-1] == 0.0:
            ws.pop()
        while len(ws) > 1 and ws[0] == 0.0:
            ws.pop(0)
            lo += 1
        taps.append((lo, ws))
    return taps


def axis_table(n_in: int, n_out: int, mode: str, antialias: bool, device: Any = "cpu") -> native.Dinov2Axis:
    taps = axis_taps(n_in, n_out, mode, antialias)
    first = torch.tensor([lo for lo, _ in taps], dtype=torch.int32)
    count = torch.tensor([len(ws) for _, ws in taps], dtype=torch.int32)
    offset = torch.cumsum(count, 0, dtype=torch.int32) - count
    weight = torch.tensor([wv for _, ws in taps for wv in ws], dtype=torch.float64).to(torch.float32)
    return native.Dinov2Axis(first, count, offset, weight, n_in, device)


def axis_matrix(t: native.Dinov2Axis) -> Tensor:
    """The table as a dense float32 [n_out, n_src] matrix (tests apply it with plain matmuls)."""
    first, count, offset, weight = t.host
    m = torch.zeros(t.n_out, t.n_src, dtype=torch.float32)
    for i in range(t.n_out):
        m[i, int(first[i]) : int(first[i]) + int(count[i])] = weight[int(offset[i]) : int(offset[i]) + int(count[i])]
    return m


def resample_host(grid: Tensor, ty: native.Dinov2Axis, tx: native.Dinov2Axis) -> Tensor:
    """grid [Hs, Ws, D] float32 -> [h, w, D]: what the kernel computes, as two float32 matmuls."""
    return torch.einsum("ia,jb,abd->ijd", axis_matrix(ty), axis_matrix(tx), grid.float())


def fold_layer_scale(w: Tensor, b: Optional[Tensor], g: Tensor) -> tuple[Tensor, Optional[Tensor]]:
    """(diag(g) W, g b): res + g * (x W^T + b) == res + x W'^T + b'.  In the dtype of its arguments (the lowering passes float32)."""
    return w * g.unsqueeze(1), None if b is None else b * g


def token_rows(T: int) -> int:
    return (T + 63) // 64 * 64


def cropped_shape(shape: tuple, P: int) -> tuple:
    """The part of a [B, C, H, W] input the strided patch convolution reads: H and W floored to whole patches."""
    B, C, H, W = shape
    return (B, C, H // P * P, W // P * P)


class DINOv2Lowering(Lowering):
    def lower(self, vit: Any, image: Tensor, out: Tensor) -> None:
        """image [B, 3, H, W] (static) -> out [B * Tp, D] (static), Tp = token_rows(T): image b's T tokens are rows b * Tp ... b * Tp + T - 1."""
        ch = kids(vit)
        _expect(len(ch) in (4, 5) and isa(ch[0], "Concatenate") and isa(ch[1], "PositionalEncoder") and isa(ch[-2], "Transformer") and isa(ch[-1], "LayerNorm"), "unexpected ViT layout")
        _expect(len(ch) == 4 or isa(ch[2], "Registers"), f"unexpected {cname(ch[2])} in front of the Transformer")
        B, _c, H, W = image.shape
        with self.in_step():
            x, T, Tp = self.embed(ch[0], ch[1], ch[2] if len(ch) == 5 else None, image)
            _expect(tuple(out.shape) == (B * Tp, x.shape[1]) and out.is_contiguous(), "output rows of another shape")
            stats = None
            for layer in kids(ch[-2]):
                stats = self.transformer_layer(layer, x, B, T, Tp, stats)
            ln = ch[-1]
            _expect(tuple(ln.normalized_shape) == (x.shape[1],), "final LayerNorm shape mismatch")
            native.layernorm(x, self._w(ln.weight), self._w(ln.bias), ln.eps, out)
            self.pool.put(x)
        self.T, self.Tp = T, Tp

    def plain_linear(self, node: Any) -> Any:
        _expect(not isa(node, "LoraAdapter"), "LoRA on a DINOv2 Linear is not lowered")
        _expect(isa(node, "Linear"), f"expected a Linear, got {cname(node)}")
        _expect(node.weight.shape[1] % self.kblk == 0, f"width {node.weight.shape[1]} is not a multiple of the GEMM K block {self.kblk}")
        return node

    # ---------------------------------------------------------------------------------------------------------------
    def embed(self, cat: Any, penc: Any, regs: Any, image: Tensor) -> tuple[Tensor, int, int]:
        cc = kids(cat)
        _expect(len(cc) == 2 and cat.dim == 1 and isa(cc[0], "ClassToken") and isa(cc[1], "PatchEncoder"), "unexpected class token / patch encoder layout")
        pe = kids(cc[1])
        _expect(len(pe) == 4 and isa(pe[0], "SetContext") and isa(pe[1], "Conv2d") and isa(pe[2], "Reshape") and isa(pe[3], "Transpose"), "unexpected PatchEncoder layout")
        conv = pe[1]
        P = conv.kernel_size[0]
        _expect(tuple(conv.kernel_size) == tuple(conv.stride) == (P, P) and tuple(conv.padding) == (0, 0) and conv.bias is not None, "unexpected patch convolution")
        B, Ci, H, W = image.shape
        D = conv.out_channels
        h, w = H // P, W // P
        _expect(h >= 1 and w >= 1, f"an input of {H} x {W} is smaller than one {P} x {P} patch")
        _expect(H == h * P and W == w * P, f"an input of {H} x {W} that the caller did not crop to whole patches")  # (CompiledDINOv2 copies the cropped image in)
        _expect(D % self.kblk == 0, f"embedding width {D} is not a multiple of the GEMM K block {self.kblk}")
        n = h * w
        pc = kids(penc)
        _expect(len(pc) == 2 and isa(pc[0], "PositionalEmbedding") and isa(pc[1], "Chain"), "unexpected PositionalEncoder layout")
        ic = kids(pc[1])
        _expect(len(ic) == 2 and isa(ic[0], "Parallel") and isa(ic[1], "InterpolateEmbedding") and ic[1].patch_size == P, "unexpected position interpolation layout")
        mode, aa = ic[1].mode, bool(ic[1].antialias)
        _expect(mode in MODES, f"interpolation mode {mode!r} (bicubic and bilinear are lowered)")
        table = kids(pc[0])[0].weight
        cls = kids(cc[0])[0].weight
        Mg = math.isqrt(table.shape[0] - 1)
        _expect(table.dim() == 2 and table.shape[1] == D and Mg >= 1 and Mg * Mg == table.shape[0] - 1 and tuple(cls.shape) == (1, D), "unexpected class token / position table")
        reg = None
        if regs is not None:
            rc = kids(regs)
            _expect(len(rc) == 3 and regs.dim == 1 and isa(rc[0], "Slicing") and isa(rc[1], "Parameter") and isa(rc[2], "Slicing") and (rc[0].dim, rc[0].start, rc[0].end) == (1, 0, 1)
                    and (rc[2].dim, rc[2].start, rc[2].end, rc[2].step) == (1, 1, None, 1), "unexpected Registers layout")
            reg = self._w(rc[1].weight)
            _expect(reg.dim() == 2 and reg.shape[1] == D, "unexpected register tokens")
        R = 0 if reg is None else reg.shape[0]
        T = 1 + R + n
        Tp = token_rows(T)

        # positions: the table's own storage when it already is a tensor of the compute dtype; resampled once, in the prologue
        tab = self._w(table)
        pos = torch.empty(n, D, device=self.device, dtype=torch.float32)
        ty = self.cache.get(("dinov2_taps", Mg, h, mode, aa, str(self.device)), lambda: axis_table(Mg, h, mode, aa, self.device))
        tx = self.cache.get(("dinov2_taps", Mg, w, mode, aa, str(self.device)), lambda: axis_table(Mg, w, mode, aa, self.device))
        with self.in_prologue():
            native.dinov2_pos_resample(tab[1:], ty, tx, pos)

        K = Ci * P * P
        Kp = (K + self.kblk - 1) // self.kblk * self.kblk  # 588 -> 640 (bf16) / 608 (float32): zero columns against zero weight columns

        def pack_w() -> Tensor:
            wp = torch.zeros(D, Kp, device=self.device, dtype=self.dtype)
            if self.device.type != "meta":
                wp[:, :K] = conv.weight.detach().reshape(D, K).to(self.device, self.dtype)
            return wp

        wp = self.cache.get(("dinov2_patch_w", Kp) + PackCache.ident(conv.weight), pack_w)
        cols = torch.zeros(B * n, Kp, device=self.device, dtype=self.dtype)  # columns >= K stay zero: patchify writes K per row
        self.__dict__.setdefault("_keep", []).extend([cols, pos])
        native.patchify_nchw(image, P, cols)
        y = self.pool.get(B * n, D)
        native.gemm([(cols, wp)], y, bias=self._w(conv.bias))
        x = self.pool.get(B * Tp, D)
        native.dinov2_tokens(y, pos, self._w(cls).view(-1), tab[0], reg, x, B, rows=Tp)
        self.pool.put(y)
        return x, T, Tp

    # ---------------------------------------------------------------------------------------------------------------
    def scaled_spec(self, lin: Any, scale: Any) -> LinSpec:
        """LinSpec of `LayerScale(Linear(x))`: weight rows and bias scaled in float32, then cast."""
        _expect(isa(scale, "LayerScale") and tuple(scale.weight.shape) == (lin.weight.shape[0],), "unexpected LayerScale")

        def make() -> tuple[Tensor, Optional[Tensor]]:
            if self.device.type == "meta":
                return (torch.empty(tuple(lin.weight.shape), device=self.device, dtype=self.dtype),
                        None if lin.bias is None else torch.empty(tuple(lin.bias.shape), device=self.device, dtype=self.dtype))
            f32 = lambda t: None if t is None else t.detach().to(self.device, torch.float32)  # noqa: E731
            w, b = fold_layer_scale(f32(lin.weight), f32(lin.bias), f32(scale.weight))
            return w.to(self.dtype).contiguous(), None if b is None else b.to(self.dtype).contiguous()

        w, b = self.cache.get(("dinov2_layer_scale",) + PackCache.ident(lin.weight, lin.bias, scale.weight), make)
        return LinSpec(w, b)

    def transformer_layer(self, layer: Any, x: Tensor, B: int, T: int, Tp: int, stats: Optional[Tensor]) -> Optional[Tensor]:
        """x updated in place; `stats`: the row statistics of x when its producer wrote them.  Returns the statistics of the updated x (or None)."""
        ch = kids(layer)
        _expect(isa(layer, "TransformerLayer") and len(ch) == 2 and all(isa(c, "Residual") for c in ch), "unexpected TransformerLayer layout")
        r1, r2 = kids(ch[0]), kids(ch[1])
        _expect(len(r1) == 3 and isa(r1[0], "LayerNorm") and isa(r1[1], "SelfAttention") and isa(r1[2], "LayerScale"), "unexpected attention residual")
        _expect(len(r2) == 3 and isa(r2[0], "LayerNorm") and isa(r2[1], "FeedForward") and isa(r2[2], "LayerScale"), "unexpected feed-forward residual")
        M, C = x.shape
        (qn, kn, vn), sd, on, ip = self._split_attention(r1[1])
        _expect(ip is None, "expected a plain SelfAttention")
        heads = sd.num_heads
        d = C // heads
        _expect(C % heads == 0 and d % 8 == 0 and d <= 160, f"head dim {d if C % heads == 0 else C / heads} (the attention kernel serves multiples of 8 up to 160)")
        _expect(C % 64 == 0, f"embedding width {C} is no multiple of 64 (the transposed V group of the Q|K|V launch starts at column 2 C)")
        ql, kl, vl, ol = (self.plain_linear(nd) for nd in (qn, kn, vn, on))
        _expect(all(tuple(l.weight.shape) == (C, C) for l in (ql, kl, vl, ol)), "unexpected attention projections")

        def qkv() -> tuple[Tensor, Optional[Tensor]]:
            w = torch.cat([self.cvt(l.weight) for l in (ql, kl, vl)], 0).contiguous()
            if all(l.bias is None for l in (ql, kl, vl)):
                return w, None
            z = lambda l: self.cvt(l.bias) if l.bias is not None else torch.zeros(C, device=self.device, dtype=self.dtype)  # noqa: E731
            return w, torch.cat([z(l) for l in (ql, kl, vl)]).contiguous()

        wqkv = LinSpec(*self.cache.get(("dinov2_qkv",) + PackCache.ident(ql.weight, kl.weight, vl.weight, ql.bias, kl.bias, vl.bias), qkv))
        ln1 = r1[0]
        _expect(tuple(ln1.normalized_shape) == (C,) and tuple(r2[0].normalized_shape) == (C,), "LayerNorm shape mismatch")
        qk = self.pool.get(M, 2 * C)
        vt = self.pool.get(C, M)
        if self.ln_fusable(stats, wqkv):
            wl, ls, lc = self.ln_fold(wqkv, ln1)
            native.gemm([(x, self.kblocked(wl))], qk, out_t=vt, nt_begin=2 * C, ln=(stats, ls, lc, float(ln1.eps)))
        else:
            hn = self.layernorm(x, ln1)
            native.gemm([(hn, self.kblocked(wqkv.w))], qk, bias=wqkv.b, out_t=vt, nt_begin=2 * C)
            self.pool.put(hn)
        o = self.pool.get(M, C)
        q3 = qk.as_strided((B, Tp, C), (Tp * qk.stride(0), qk.stride(0), 1))
        k3 = qk[:, C:].as_strided((B, Tp, C), (Tp * qk.stride(0), qk.stride(0), 1))
        native.attention_general(q3, k3, vt.view(C, B, Tp), o.view(B, Tp, C), heads, T)
        self.pool.put(qk)
        self.pool.put(vt)
        buf = self.row_stats(M, C)
        self.linear(o, self.scaled_spec(ol, r1[2]), res=x, out=x, stats_out=buf)
        self.pool.put(o)

        ff = kids(r2[1])
        _expect(len(ff) == 3 and isa(ff[1], "Activation"), "unexpected FeedForward layout")
        l1, act, l2 = self.plain_linear(ff[0]), ff[1], self.plain_linear(ff[2])
        gelu = isa(act, "GeLU") and act.approximation.value == "none"
        swiglu = isa(act, "GLU") and isa(act.activation, "SiLU")
        geglu = isa(act, "GLU") and isa(act.activation, "GeLU") and act.activation.approximation.value == "none"
        _expect(gelu or swiglu or geglu, f"activation {act!r} (GELU, GLU(SiLU()) and GLU(GeLU()) are lowered)")
        s1 = self.linear_spec(l1, geglu=geglu)
        s2 = self.scaled_spec(l2, r2[2])
        _expect(s2.K == (s1.N if gelu else s1.N // 2) and s1.K == C and s2.N == C, "unexpected feed-forward widths")
        fold = self.ln_fusable(buf, s1)
        h2 = x if fold else self.layernorm(x, r2[0])
        f = self.linear(h2, s1, gelu=gelu, ln=(buf, r2[0]) if fold else None)
        if not fold:
            self.pool.put(h2)
        if swiglu:
            g = self.pool.get(M, s1.N // 2)
            native.glu_silu(f, g)
            self.pool.put(f)
            f = g
        self.linear(f, s2, res=x, out=x, stats_out=buf)
        self.pool.put(f)
        return buf


class _Entry:
    """One lowered shape: its static input / output buffers, lowering and program."""

    def __init__(self, x: Tensor, out: Tensor, low: DINOv2Lowering, program: Program) -> None:
        self.x, self.out, self.low, self.program = x, out, low, program


class CompiledDINOv2:
    """`fast = CompiledDINOv2(model); y = fast(images)` == `model(images)`: [B, 3, H, W] -> [B, 1 + registers + (H // p) (W // p), D].
    One lowered program and one HIP graph per (B, H, W), the last MAX_PROGRAMS shapes kept: a repeat call of a shape replays its graph.
    `dtype` (default: the tree's) is the compute dtype.  An in-place edit of a weight re-lowers (only what changed is re-packed).  A tree the
    lowering does not cover runs its stock forward behind a RuntimeWarning."""

    def __init__(self, model: Any, dtype: Optional[torch.dtype] = None, use_graph: bool = True) -> None:
        native.load()
        self.model = model
        self.dtype = dtype
        self.use_graph = use_graph
        self.cache = PackCache()
        self.entries: dict[Any, _Entry] = {}
        self.version: Any = None
        self.bad_keys: set = set()
        self.lowerings = 0
        self.stats: dict[str, Any] = {}
        self.program: Optional[Program] = None

    def _tree_dtype(self) -> torch.dtype:
        return next(p.dtype for p in self.model.parameters())

    def _weights_version(self) -> tuple:
        """Every program holds copies of the weights (K-blocked, folded, converted) and a resampled copy of the position table: an in-place edit
        of any of them, or a change of the tree, drops the programs."""
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
                P, D = self.model.patch_size, self.model.embedding_dim
                x = torch.empty(cropped_shape(tuple(image.shape), P), device=image.device, dtype=dtype)
                low = DINOv2Lowering(image.device, dtype, self.cache, "merged")
                T = 1 + self.model.num_registers + (image.shape[2] // P) * (image.shape[3] // P)
                out = torch.empty(image.shape[0] * token_rows(T), D, device=image.device, dtype=dtype)
                low.lower(self.model, x, out)
            except Unsupported as err:
                warnings.warn(f"CompiledDINOv2: {err}; running the stock forward", RuntimeWarning, stacklevel=2)
                self.bad_keys.add(key)
                return self._stock(image)
            if edited:  # (a further shape of the same weights adds packs and must not sweep the other programs' away)
                self.cache.sweep()
            native.replay(low.prologue)  # the position table, resampled to this grid
            self.lowerings += 1
            e = _Entry(x, out, low, Program(low.step, self.use_graph, low=low))
            while len(self.entries) >= MAX_PROGRAMS:
                self.entries.pop(next(iter(self.entries)))
            self.entries[key] = e
        self.program = e.program
        self.stats = dict(e.low.stats, step_ops=launches(e.low.step), prologue_ops=launches(e.low.prologue), pool_bytes=e.low.step_pool.bytes(), lowerings=self.lowerings,
                          tokens=e.low.T, token_rows=e.low.Tp)
        e.x.copy_(image[:, :, : e.x.shape[2], : e.x.shape[3]])  # the strided convolution drops a remainder of H, W: so does this copy
        e.program.run()
        return e.out.view(image.shape[0], e.low.Tp, -1)[:, : e.low.T].clone()

    def _stock(self, image: Tensor) -> Tensor:
        return self.model(image.to(self._tree_dtype()))
