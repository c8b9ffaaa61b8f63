"""MI355X lowering of the Swin Transformer backbone (refiners_amd.swin, or refiners' own foundationals.swin classes: MVANet's encoder).

Same engine as the SAM ViT: the Chain tree is walked once and turned into a launch program; tokens stay channels-last [B*g*g, C].

  PatchEmbedding        -> patchify kernel + ONE GEMM (K = 3*4*4 = 48 zero-padded to the GEMM's K block) + LayerNorm
  SwinTransformerBlock  -> LayerNorm (standalone: the padded rows must be exact zeros AFTER it)
                           | row gather = Pad + Roll(-shift) + ToWindows as ONE static index table, -1 = zero row
                           | QKV GEMM + bias | mi355x_window_attention (relative position bias from the compact table in LDS, the -100
                           shift mask from (nw, ws, shift) and the window's position: neither an N x N bias nor a mask tensor exists)
                           | row gather = FromWindows + Roll(+shift) + Unpad, BEFORE the output projection (padded rows are never projected)
                           | out-proj GEMM + residual | LayerNorm folded into the GEMM + erf-GELU epilogue | GEMM + residual
  PatchMerging          -> four row gathers into the four column blocks of [B*ceil(g/2)^2, 4C] (-1 = the zero row / column an odd grid
                           is padded with; blocks (y&1, x&1) = (0,0), (1,0), (0,1), (1,1)) | LayerNorm(4C) | GEMM (no bias)
  stage outputs         -> LayerNorm + nhwc_to_nchw into the output map

Refused (Unsupported: the stock forward runs instead, behind a RuntimeWarning): head dim != 32, ws^2 > 144, a relative_position_index that
is not the canonical one, non-square inputs or a side the patch does not divide, widths that are no multiple of the GEMM K block, a stage
with fewer than 2 windows per side (the reference itself raises on a shifted stage of one window), LoRA on a Swin Linear.
"""
from __future__ import annotations

import warnings
from typing import Any, Optional

import torch
from torch import Tensor

from .. import native
from ..fluxion.tree import tree_epoch
from .compiled import Program
from .lowering_blocks import BlockLowering as Lowering
from .packing import PackCache, Unsupported, _expect, cname, isa, kids, launches

HEAD_DIM = 32    # the only head width mi355x_window_attention instantiates
MAX_TOKENS = 144  # tokens per window (ws <= 12)


def canonical_index(ws: int) -> Tensor:
    t = torch.arange(ws * ws)
    y, x = t // ws, t % ws
    return (y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)


def window_tables(B: int, g: int, ws: int, shift: int) -> tuple[Tensor, Tensor, int]:
    """(part, merge, nw) of a g x g grid: part[row of the window layout] = source token or -1 (a padded position), for
    Pad(ws) + Roll(-shift) + ToWindows; merge[token] = its row of the window layout, for FromWindows + Roll(+shift) + Unpad.  int32, CPU."""
    nw = -(-g // ws)
    Sp = nw * ws
    b, wy, wx, ty, tx = torch.meshgrid(torch.arange(B), torch.arange(nw), torch.arange(nw), torch.arange(ws), torch.arange(ws), indexing="ij")
    sy, sx = (wy * ws + ty + shift) % Sp, (wx * ws + tx + shift) % Sp  # rolled[p] = padded[(p + shift) mod Sp]
    part = torch.where((sy < g) & (sx < g), (b * g + sy) * g + sx, torch.full_like(sy, -1)).reshape(-1)
    gb, gy, gx = torch.meshgrid(torch.arange(B), torch.arange(g), torch.arange(g), indexing="ij")
    ry, rx = (gy - shift) % Sp, (gx - shift) % Sp  # where token (gy, gx) sits on the rolled grid
    merge = (((gb * nw + ry // ws) * nw + rx // ws) * ws + ry % ws) * ws + rx % ws
    return part.to(torch.int32), merge.reshape(-1).to(torch.int32), nw


def merging_tables(B: int, g: int) -> tuple[list[Tensor], int]:
    """Four int32 tables (one per column block of PatchMerging's [B * g2 * g2, 4C] rows, g2 = ceil(g / 2)): block j holds the token at
    (2 hy + (j & 1), 2 wx + (j >> 1)), -1 where an odd grid was padded."""
    g2 = -(-g // 2)
    b, hy, wx = torch.meshgrid(torch.arange(B), torch.arange(g2), torch.arange(g2), indexing="ij")
    out = []
    for j in range(4):
        y, x = 2 * hy + (j & 1), 2 * wx + (j >> 1)
        out.append(torch.where((y < g) & (x < g), (b * g + y) * g + x, torch.full_like(y, -1)).reshape(-1).to(torch.int32))
    return out, g2


def shift_mask_model(nw: int, ws: int, shift: int) -> Tensor:
    """Host restatement of the kernel's mask arithmetic -> [nw * nw, N, N] float32 (tests compare it with the mirror's mask): window
    (wy, wx) gives token (y, x) the region 3 r(wy, y) + r(wx, x), r(w, p) = 0 unless w == nw - 1, then 1 for p < ws - shift, else 2."""
    N = ws * ws
    t = torch.arange(N)
    y, x = t // ws, t % ws
    out = torch.zeros(nw * nw, N, N)
    for w in range(nw * nw):
        wy, wx = w // nw, w % nw
        ry = torch.where(y < ws - shift, 1, 2) if wy == nw - 1 else torch.zeros_like(y)
        rx = torch.where(x < ws - shift, 1, 2) if wx == nw - 1 else torch.zeros_like(x)
        reg = 3 * ry + rx
        out[w] = torch.where(reg[:, None] != reg[None, :], -100.0, 0.0)
    return out


class SwinLowering(Lowering):
    def lower(self, swin: Any, image: Tensor, outs: list[Tensor], as_tokens: bool = False) -> None:
        """image [B, 3, S, S] (static) -> outs, the static NCHW maps in the order the forward returns them (stage_n, ..., stage_1, patch_embedding).
        as_tokens (MVANet's decoder reads the maps channels-last): outs are the [B * g * g, C] token rows of the same maps, no nhwc_to_nchw."""
        self.as_tokens = as_tokens
        ch = kids(swin)
        _expect(len(ch) >= 3 and isa(ch[0], "PatchEmbedding") and isa(ch[1], "Passthrough") and all(isa(c, "Chain") for c in ch[2:]), "unexpected SwinTransformer layout")
        stages = ch[2:]
        B, _c, H, W = image.shape
        _expect(H == W, f"non-square input {H} x {W}")
        _expect(len(outs) == len(stages) + 1, "one output map per stage and one for the patch embedding")
        with self.in_step():
            tok, g = self.patch_embedding(ch[0], image)
            self.emit_output(tok, None, B, g, outs[-1])
            for i, st in enumerate(stages):
                sc = kids(st)
                _expect(len(sc) == 3 and isa(sc[0], "BasicLayer") and isa(sc[1], "Passthrough"), "unexpected stage layout")
                for blk in kids(sc[0]):
                    tok = self.block(blk, tok, B, g)
                pc = kids(sc[1])
                _expect(len(pc) == 4 and isa(pc[0], "LayerNorm") and isa(pc[1], "Transpose") and isa(pc[2], "SquareUnflatten") and isa(pc[3], "SetContext"), "unexpected stage output layout")
                self.emit_output(tok, pc[0], B, g, outs[len(stages) - 1 - i])
                last = i == len(stages) - 1
                _expect(isa(sc[2], "UseContext") if last else isa(sc[2], "PatchMerging"), "unexpected end of a stage")
                if not last:
                    tok, g = self.patch_merging(sc[2], tok, B, g)
            self.pool.put(tok)

    def plain_linear(self, node: Any) -> Any:
        _expect(not isa(node, "LoraAdapter"), "LoRA on a Swin Linear is not lowered")
        _expect(isa(node, "Linear"), f"expected a Linear, got {cname(node)}")
        return self.linear_spec(node)

    # ---------------------------------------------------------------------------------------------------------------
    def patch_embedding(self, pe: Any, image: Tensor) -> tuple[Tensor, int]:
        ch = kids(pe)
        _expect(len(ch) == 4 and isa(ch[0], "Conv2d") and isa(ch[1], "Flatten") and isa(ch[2], "Transpose") and isa(ch[3], "LayerNorm"), "unexpected PatchEmbedding layout")
        conv = ch[0]
        P = conv.kernel_size[0]
        _expect(tuple(conv.kernel_size) == tuple(conv.stride) == (P, P) and conv.bias is not None, "unexpected patch convolution")
        B, C, S, _ = image.shape
        _expect(S % P == 0, f"input side {S} is not divisible by the patch size {P}")
        _expect(conv.out_channels % self.kblk == 0, f"embedding width {conv.out_channels} is not a multiple of the GEMM K block {self.kblk}")
        g = S // P
        K = C * P * P
        Kp = (K + self.kblk - 1) // self.kblk * self.kblk

        def pack() -> Tensor:
            w = torch.zeros(conv.out_channels, Kp, device=self.device, dtype=self.dtype)
            w[:, :K] = conv.weight.detach().reshape(conv.out_channels, K).to(device=self.device, dtype=self.dtype)
            return w

        w = self.cache.get(("swin_patch_w", Kp) + PackCache.ident(conv.weight), pack)
        cols = torch.zeros(B * g * g, Kp, device=self.device, dtype=self.dtype)  # columns >= K stay zero: patchify writes K per row
        self.__dict__.setdefault("_keep", []).append(cols)
        native.patchify_nchw(image, P, cols)
        y = self.pool.get(B * g * g, conv.out_channels)
        native.gemm([(cols, w)], y, bias=self._w(conv.bias))
        tok = self.layernorm(y, ch[3])
        self.pool.put(y)
        return tok, g

    def emit_output(self, tok: Tensor, ln: Any, B: int, g: int, out: Tensor) -> None:
        C = tok.shape[1]
        if getattr(self, "as_tokens", False):
            _expect(tuple(out.shape) == (B * g * g, C) and out.is_contiguous(), "output rows of another shape")
            if ln is None:
                native.axpby(tok, 1.0, tok, 0.0, out)  # (a copy: the blocks go on updating tok in place)
            else:
                native.layernorm(tok, self._w(ln.weight), self._w(ln.bias), ln.eps, out)
            return
        _expect(tuple(out.shape) == (B, C, g, g), "output map of another shape")
        y = tok if ln is None else self.layernorm(tok, ln)
        native.nhwc_to_nchw(y.view(B, g * g, C), out, C)
        if ln is not None:
            self.pool.put(y)

    def _tables(self, B: int, g: int, ws: int, shift: int) -> tuple[Tensor, Tensor, int]:
        def make() -> tuple[Tensor, Tensor, int]:
            part, merge, nw = window_tables(B, g, ws, shift)
            return part.to(self.device), merge.to(self.device), nw

        return self.cache.get(("swin_windows", B, g, ws, shift), make)

    def bias_table(self, rpb: Any, ws: int, heads: int) -> Tensor:
        table, index = rpb.relative_position_bias_table, rpb.relative_position_index
        _expect(tuple(table.shape) == ((2 * ws - 1) ** 2, heads) and tuple(index.shape) == (ws * ws, ws * ws), "unexpected relative position bias shapes")

        def check() -> bool:  # at pack time: once per (index tensor, version)
            return index.device.type == "meta" or bool(torch.equal(index.detach().cpu().long(), canonical_index(ws)))

        _expect(self.cache.get(("swin_index", ws) + PackCache.ident(index), check), "relative_position_index is not the canonical index the kernel computes")
        if table.dtype == torch.float32 and table.device == self.device and table.is_contiguous():
            return table.detach()  # the tree's own storage: an in-place edit is seen by the next replay
        return self.cache.get(("swin_table",) + PackCache.ident(table), lambda: table.detach().to(device=self.device, dtype=torch.float32).contiguous())

    def block(self, blk: Any, tok: Tensor, B: int, g: int) -> Tensor:
        ch = kids(blk)
        _expect(isa(blk, "SwinTransformerBlock") and len(ch) == 2 and isa(ch[0], "Residual") and isa(ch[1], "Residual"), "unexpected SwinTransformerBlock layout")
        r1, r2 = kids(ch[0]), kids(ch[1])
        names = ["LayerNorm", "SquareUnflatten", "StatefulPad", "Roll", "ToWindows", "WindowAttention", "FromWindows", "Roll", "StatefulUnpad", "Flatten"]
        _expect([cname(c) for c in r1] == names, "unexpected attention residual")
        wa = kids(r1[5])
        _expect(len(wa) == 3 and isa(wa[1], "WindowSDPA"), "unexpected WindowAttention layout")
        sd = wa[1]
        ws, heads = sd.window_size, sd.num_heads
        M, C = tok.shape
        shift = -r1[3]._shifts[0]
        _expect(tuple(r1[3]._dims) == (1, 2) and tuple(r1[3]._shifts) == (-shift, -shift) and tuple(r1[7]._dims) == (1, 2) and tuple(r1[7]._shifts) == (shift, shift)
                and 0 <= shift < ws and bool(sd.shift) == (shift > 0) and r1[4].window_size == ws and kids(r1[2])[1].step == ws, "inconsistent roll / window / pad parameters")
        _expect(C == heads * HEAD_DIM, f"head dim {C // heads if C % heads == 0 else C / heads} (the window attention kernel serves {HEAD_DIM})")
        _expect(ws * ws <= MAX_TOKENS, f"windows of {ws * ws} tokens (the window attention kernel holds at most {MAX_TOKENS})")
        table = self.bias_table(sd.rpb, ws, heads)
        qkv_spec, out_spec = self.plain_linear(wa[0]), self.plain_linear(wa[2])
        _expect(qkv_spec.N == 3 * C and qkv_spec.b is not None and out_spec.N == C, "unexpected projections")
        part, merge, nw = self._tables(B, g, ws, shift)
        _expect(nw >= 2, f"a stage of {nw} x {nw} windows (at least 2 per side are needed)")
        N, nW = ws * ws, B * nw * nw
        h = self.layernorm(tok, r1[0])
        hw = self.pool.get(nW * N, C)
        native.gather_rows(h, part, hw)
        self.pool.put(h)
        qkv = self.linear(hw, qkv_spec)
        self.pool.put(hw)
        att = self.pool.get(nW * N, C)
        q3 = qkv.view(nW, N, 3 * C)
        native.window_attention(q3[:, :, :C], q3[:, :, C : 2 * C], q3[:, :, 2 * C :], table, att.view(nW, N, C), heads, ws, nw=nw, shift=shift, scale=HEAD_DIM ** -0.5)
        self.pool.put(qkv)
        am = self.pool.get(M, C)
        native.gather_rows(att, merge, am)
        self.pool.put(att)
        stats = self.row_stats(M, C)
        self.linear(am, out_spec, res=tok, out=tok, stats_out=stats)
        self.pool.put(am)
        _expect(len(r2) == 4 and isa(r2[0], "LayerNorm") and isa(r2[1], "Linear", "LoraAdapter") and isa(r2[2], "GeLU") and r2[2].approximation.value == "none"
                and isa(r2[3], "Linear", "LoraAdapter"), "unexpected MLP residual")
        s1, s2 = self.plain_linear(r2[1]), self.plain_linear(r2[3])
        if self.ln_fusable(stats, s1):
            f = self.linear(tok, s1, gelu=True, ln=(stats, r2[0]))
        else:
            h2 = self.layernorm(tok, r2[0])
            f = self.linear(h2, s1, gelu=True)
            self.pool.put(h2)
        self.linear(f, s2, res=tok, out=tok)
        self.pool.put(f)
        return tok

    def patch_merging(self, pm: Any, tok: Tensor, B: int, g: int) -> tuple[Tensor, int]:
        ch = kids(pm)
        names = ["SquareUnflatten", "Pad", "WindowUnflatten", "WindowUnflatten", "Permute", "Flatten", "Flatten", "LayerNorm", "Linear"]
        _expect([cname(c) for c in ch] == names and ch[1].step == 2 and tuple(ch[4].dims) == (0, 1, 3, 4, 2, 5) and (ch[2].dim, ch[3].dim) == (2, 1), "unexpected PatchMerging layout")
        C = tok.shape[1]
        spec = self.plain_linear(ch[8])
        _expect(spec.K == 4 * C and spec.b is None, "unexpected PatchMerging projection")

        def make() -> tuple:
            tabs, g2 = merging_tables(B, g)
            return tuple(t.to(self.device) for t in tabs) + (g2,)

        *tabs, g2 = self.cache.get(("swin_merging", B, g), make)
        cat = self.pool.get(B * g2 * g2, 4 * C)
        for j, t in enumerate(tabs):
            native.gather_rows(tok, t, cat[:, j * C : (j + 1) * C])
        self.pool.put(tok)
        hn = self.layernorm(cat, ch[7])
        self.pool.put(cat)
        out = self.linear(hn, spec)
        self.pool.put(hn)
        return out, g2


def output_shapes(swin: Any, B: int, S: int) -> list[tuple[int, int, int, int]]:
    """Shapes of the maps the forward returns for a [B, 3, S, S] input (stage_n, ..., stage_1, patch_embedding)."""
    pe = kids(swin)[0]
    conv = kids(pe)[0]
    g, C = S // conv.kernel_size[0], conv.out_channels
    shapes = [(B, C, g, g)]
    n = len(kids(swin)) - 2
    for i in range(n):
        shapes.insert(0, (B, C, g, g))
        g, C = -(-g // 2), 2 * C
    return shapes


class CompiledSwinTransformer:
    """`fast = CompiledSwinTransformer(swin); maps = fast(x)` == `swin(x)`: the tuple (stage_n, ..., stage_1, patch_embedding) of NCHW maps.
    One program per (batch, side), replayed as a HIP graph.  `dtype` (default: the tree's) is the compute dtype.  A tree the lowering does
    not cover runs its stock forward behind a RuntimeWarning."""

    def __init__(self, swin: Any, dtype: Optional[torch.dtype] = None, use_graph: bool = True) -> None:
        native.load()
        self.swin = swin
        self.dtype = dtype
        self.use_graph = use_graph
        self.cache = PackCache()
        self.key: Any = None
        self.bad_key: Any = None
        self.lowerings = 0
        self.stats: dict[str, Any] = {}

    def _tree_dtype(self) -> torch.dtype:
        return next(p.dtype for p in self.swin.parameters())

    def _weights_version(self, dtype: torch.dtype) -> int:
        """Versions of the tensors a program holds COPIES of (K-blocked / padded / converted): an in-place edit of one re-lowers (the PackCache
        re-packs only what changed).  The float32 bias tables are read where they are and need no new program."""
        return sum(p._version for n, p in self.swin.named_parameters() if not (n.endswith("relative_position_bias_table") and p.dtype == torch.float32 == dtype)) + sum(
            b._version for b in self.swin.buffers())

    @torch.no_grad()
    def __call__(self, image: Tensor) -> tuple[Tensor, ...]:
        dtype = self.dtype or self._tree_dtype()
        key = (tree_epoch(), tuple(image.shape), dtype, image.device, self._weights_version(dtype))
        if key == self.bad_key:
            return self._stock(image)
        if key != self.key:
            try:
                _expect(image.dim() == 4 and image.shape[2] == image.shape[3], f"non-square input {tuple(image.shape)}")
                self.x = torch.empty(tuple(image.shape), device=image.device, dtype=dtype)
                self.outs = [torch.empty(s, device=image.device, dtype=dtype) for s in output_shapes(self.swin, image.shape[0], image.shape[2])]
                low = SwinLowering(image.device, dtype, self.cache, "merged")
                low.lower(self.swin, self.x, self.outs)
            except Unsupported as e:
                warnings.warn(f"CompiledSwinTransformer: {e}; running the stock forward", RuntimeWarning, stacklevel=2)
                self.bad_key = key
                return self._stock(image)
            self.cache.sweep()
            self.low, self.key = low, key
            self.lowerings += 1
            self.program = Program(low.step, self.use_graph, low=low)
            self.stats = dict(low.stats, step_ops=launches(low.step), pool_bytes=low.step_pool.bytes(), lowerings=self.lowerings)
        self.x.copy_(image)
        self.program.run()
        return tuple(o.clone() for o in self.outs)

    def _stock(self, image: Tensor) -> tuple[Tensor, ...]:
        return self.swin(image.to(self._tree_dtype()))
