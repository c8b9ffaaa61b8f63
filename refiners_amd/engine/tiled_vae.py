"""MI355X lowering of the autoencoder's tiled inference (reference auto_encoder.py:209-621: FixedGroupNorm, _generate_latent_tiles,
_create_blending_mask, _tiled_encode, _tiled_decode) -- the two ends of a canvas larger than one encoder / decoder call.

    vae = CompiledTiledVAE(lda, tile_size=(512, 512), blending=64)
    vae.calibrate(x)              # x: the (1, 3, tile_h, tile_w) tensor _add_fixed_group_norm feeds to encode; or vae.adopt() inside
                                  # `with lda.tiled_inference(image):` to take the statistics the FixedGroupNorm nodes already hold
    latents = vae.encode(image)   # == lda._tiled_encode(image, tile_size, blending)
    image = vae.decode(latents)   # == lda._tiled_decode(latents, tile_size, blending)

Fixed statistics: every GroupNorm owns a persistent float32 table [C][2] = (group mean, gamma / sqrt(var + eps)).  The calibration programs
fill it (mi355x_groupnorm_table) and apply it (mi355x_groupnorm_fixed); every tile program only applies it: ONE launch per GroupNorm, no statistics
pass, and the convolutions write no column statistics (gn_stats off).  Tiles: the grid has at most four tile sizes; the tiles of one size run in chunks
of `tile_batch` through one program per (size, chunk length), cached by shape.  mi355x_vae_tile_gather cuts a chunk's tiles out of the canvas straight
into the program's input (NCHW latents for the decoder, the zero-padded token-major first activation for the encoder).  Blend: a chunk's output (the
token-major rows of the decoder's last convolution as they are, the encoder's NCHW latents) is kept in one arena (one device-to-device copy of the
3- or 4-channel result per chunk), and mi355x_vae_tile_blend reads every tile there through its strides -- no mask tensor, no per-tile layout change.
One tile: the plain program with the fixed statistics, no blend.  Everything stays on the device; a repeat call of the same shape replays one HIP graph.

No timing exists yet: `tile_batch = 4` is a guess until tools/probe_tiled_vae.py has run on an MI355X.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import Any, Iterator, Optional

import torch
from torch import Tensor

from .. import native
from .packing import Act, PackCache, Unsupported, _expect, cname, isa, kids, launches
from .unet_lowering import UNetContext
from .vae import VAEDecoderLowering

TILE_BATCH = 4  # tiles per program launch; a guess (see the module docstring)


# ------------------------------------------------------------------------------------------------ geometry (host)
@dataclass
class Grid:
    """The tile list of _generate_latent_tiles as the grid it is, in the units of the blended canvas (`scale` = 8 for the decoder's pixels)."""

    xs: list[tuple[int, int]]  # (start, extent) of the columns
    ys: list[tuple[int, int]]  # (start, extent) of the rows
    stride: tuple[int, int]    # (x, y)
    tile: tuple[int, int]      # nominal (w, h)
    size: tuple[int, int]      # canvas (W, H)
    blending: int

    @property
    def tiles(self) -> list[tuple[int, int, int, int]]:
        """(top, left, bottom, right) in list order: x outer, y inner."""
        return [(y, x, y + h, x + w) for x, w in self.xs for y, h in self.ys]

    def ramp(self, ix: int, iy: int) -> int:
        """The ramp length _create_blending_mask uses for tile (ix, iy)."""
        return 0 if self.blending == 0 else min(self.blending, min(self.ys[iy][1], self.xs[ix][1]) // 2)

    def scaled(self, s: int, blending: int) -> "Grid":
        """The same grid in units s times finer (latents -> pixels), with the ramp length of those units."""
        up = lambda ax: [(a * s, e * s) for a, e in ax]  # noqa: E731
        return Grid(up(self.xs), up(self.ys), (self.stride[0] * s, self.stride[1] * s), (self.tile[0] * s, self.tile[1] * s), (self.size[0] * s, self.size[1] * s), blending)


def latent_grid(latent_wh: tuple[int, int], tile_wh: tuple[int, int], blending: int) -> Grid:
    """_generate_latent_tiles(size, tile_size // 8, overlap = blending // 8) per axis; `blending` of the result is in latents (blending // 8)."""
    overlap = blending // 8
    tile = (tile_wh[0] // 8, tile_wh[1] // 8)
    if tile[0] - overlap < 1 or tile[1] - overlap < 1:
        raise ValueError(f"blending {blending} leaves no stride for a tile of {tile_wh}")
    axes = []
    for size, t in zip(latent_wh, tile):
        axes.append([(s, min(size, s + t) - s) for s in range(0, max(size - overlap, 1), t - overlap)])
    return Grid(axes[0], axes[1], (tile[0] - overlap, tile[1] - overlap), tile, latent_wh, overlap)


def ramp_tables(grid: Grid) -> tuple[Tensor, dict[int, int]]:
    """One torch.linspace(0, 1, steps=b) per distinct ramp length of the grid, concatenated (float32, CPU), and {b: offset}."""
    lengths = sorted({grid.ramp(ix, iy) for ix in range(len(grid.xs)) for iy in range(len(grid.ys))} - {0})
    offs, parts, o = {0: 0}, [], 0
    for b in lengths:
        offs[b] = o
        parts.append(torch.linspace(0, 1, steps=b, dtype=torch.float32))
        o += b
    return (torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32)), offs


def tile_groups(grid: Grid, tile_batch: int) -> list[tuple[tuple[int, int], list[int]]]:
    """[((h, w), list indices)]: the tiles grouped by size (first appearance), each group cut into chunks of at most `tile_batch`."""
    by_size: dict[tuple[int, int], list[int]] = {}
    ny = len(grid.ys)
    for ix, (_x, w) in enumerate(grid.xs):
        for iy, (_y, h) in enumerate(grid.ys):
            by_size.setdefault((h, w), []).append(ix * ny + iy)
    return [(size, idx[i : i + tile_batch]) for size, idx in by_size.items() for i in range(0, len(idx), tile_batch)]


def blend_rows(grid: Grid, placement: dict[int, tuple[int, int, int, int]], ramp_offs: dict[int, int]) -> list[tuple[int, int, int, int, int, int]]:
    """The tile rows of mi355x_vae_tile_blend in list order; placement[list index] = (offset, s_c, s_y, s_x) of the tile in the source arena."""
    ny = len(grid.ys)
    rows = []
    for ix in range(len(grid.xs)):
        for iy in range(ny):
            b = grid.ramp(ix, iy)
            rows.append((*placement[ix * ny + iy], ramp_offs[b], b))
    return rows


# ------------------------------------------------------------------------------------------------ lowering
@dataclass
class NodeStats:
    """The frozen statistics of one GroupNorm: tab [C, 2] float32 = (group mean, gamma / sqrt(var + eps)), raw [G, 2] = (mean, biased variance)."""

    node: Any
    tab: Tensor
    raw: Tensor
    ready: bool = False


class TiledVAELowering(VAEDecoderLowering):
    """VAEDecoderLowering whose GroupNorms read per-node tables: mode "table" computes them from the activation first (calibration, batch 1),
    mode "fixed" only applies them.  No column statistics are produced: nobody reads them."""

    def __init__(self, device: torch.device, dtype: torch.dtype, cache: PackCache, tables: dict[int, NodeStats], mode: str) -> None:
        super().__init__(device, dtype, cache)
        assert mode in ("table", "fixed")
        self.gn_stats = False
        self.tables, self.mode = tables, mode
        self._table_ws: Optional[Tensor] = None
        self.keepalive: list[Any] = []

    def groupnorm(self, a: Any, gn: Any, silu: bool) -> Act:
        _expect(isa(gn, "GroupNorm") and gn.num_channels == a.C and isinstance(a, Act), "GroupNorm channel mismatch")
        st = self.tables.get(id(gn))
        if st is None or st.node is not gn:
            raise Unsupported(f"{cname(gn)} has no frozen statistics: it is not a node of the autoencoder this engine was built for")
        out = self.pool.get(a.M, a.C)
        oa = Act(out, a.B, a.H, a.W)
        if self.mode == "table":
            _expect(a.B == 1, "the calibration pass takes one image")
            need = native.load().mi355x_groupnorm_ws_floats(1, a.HW, a.C)
            if self._table_ws is None or self._table_ws.numel() < need:  # (an earlier, smaller scratch stays alive in its launches' keep-alive tuples)
                self._table_ws = torch.empty(need, dtype=torch.float32, device=self.device)
            native.groupnorm_table(a.tokens(), self._w(gn.weight), gn.num_groups, gn.eps, st.tab, st.raw, ws=self._table_ws)
        native.groupnorm_fixed(a.tokens(), st.tab, self._w(gn.bias), silu, oa.tokens())
        self.stats["gn_fixed"] = self.stats.get("gn_fixed", 0) + 1
        return oa

    def sdpa(self, q: Tensor, B: int, heads: int, streams: list, v_plain: Optional[list[Tensor]] = None) -> Tensor:
        """The mid-block's single wide head over a tile whose token count is no multiple of the GEMM's K block (edge tiles: 8 x 7 latents): the
        base lowering's GEMM / row softmax / GEMM with the key axis zero-padded to the block -- softmax_rows writes zero probabilities into the pad
        columns, V^T gets zero pad columns from a strided mi355x_vae_tile_gather of V (one launch for the batch)."""
        M, C = q.shape
        d, Lq = C // heads, M // B
        kblk = 128 // self.es
        plain = self.head_kernel(d) is not None or v_plain is None or len(streams) != 1 or streams[0][3] != 1.0 or d % kblk or self.device.type == "meta"
        if plain or (streams[0][2] % kblk == 0) or streams[0][0].shape[0] != B * streams[0][2]:
            return super().sdpa(q, B, heads, streams, v_plain)
        (k, _vt, Lk, _osc), v = streams[0], v_plain[0]
        Lp = (Lk + kblk - 1) // kblk * kblk
        out = self.pool.get(M, C)
        vt = torch.zeros(B, C, Lp, device=self.device, dtype=self.dtype)  # pad columns stay zero: the gather below never writes them
        pos_host = native.vae_pos_rows([(b * Lk, 0) for b in range(B)])
        pos = pos_host.to(self.device)
        sc = torch.empty(Lq, Lp, device=self.device, dtype=torch.float32)
        pr = torch.empty(Lq, Lp, device=self.device, dtype=self.dtype)
        self.keepalive += [vt, pos, pos_host, sc, pr]
        # V [B * Lk, C] read as a one-channel image: tile b = rows b Lk .. (b + 1) Lk, written transposed (y -> stride 1, x -> stride Lp)
        native.vae_tile_gather(v.view(1, 1, B * Lk, C), pos, pos_host, vt, B, (Lk, C), (C * Lp, 0, 1, Lp))
        for b in range(B):
            for hh in range(heads):
                qb = q[b * Lq : (b + 1) * Lq, hh * d : (hh + 1) * d]
                kb = k[b * Lk : (b + 1) * Lk, hh * d : (hh + 1) * d]
                native.gemm([(qb, kb)], sc[:, :Lk], out_f32=self.dtype != torch.float32)
                native.softmax_rows(sc, pr, Lk, d ** -0.5)
                native.gemm([(pr, vt[b, hh * d : (hh + 1) * d])], out[b * Lq : (b + 1) * Lq, hh * d : (hh + 1) * d])
        return out

    def _stages(self, stages: Any, cur: Act, ctx: UNetContext, H: int, W: int, resample: str) -> Act:
        for stage in kids(stages):
            for m in kids(stage):
                if isa(m, "Resnet"):
                    nxt = self.resnet(m, cur)
                elif isa(m, "Residual") and len(kids(m)) == 2 and isa(kids(m)[1], "SelfAttention2d"):
                    nxt = self.attention_2d(m, cur)
                elif isa(m, resample):
                    nxt = self.piece(m, cur, ctx, H, W)
                    cur = None  # piece() released the input already
                else:
                    nxt = self.torch_node(m, cur)
                if cur is not None:
                    self.pool.put(cur.t)
                cur = nxt
        return cur

    def _head(self, block: Any, cur: Act) -> Act:
        gn, act, conv = kids(block)
        _expect(isa(gn, "GroupNorm") and isa(act, "SiLU") and isa(conv, "Conv2d"), "unexpected output block")
        g = self.groupnorm(cur, gn, silu=True)
        self.pool.put(cur.t)
        y = self.conv(g, self.conv_spec(conv))
        self.pool.put(g.t)
        return y

    def lower_tile_decoder(self, dec: Any, latents: Tensor, encoder_scale: float, nchw_out: Optional[Tensor] = None) -> Act:
        """lower_decoder that leaves the last convolution's token-major rows where they are (returned; never given back to the pool) for the blend to
        read in place; `nchw_out` (the one-tile case) adds the layout change of the plain decoder."""
        ch = kids(dec)
        _expect(len(ch) == 4 and isa(ch[0], "Conv2d") and isa(ch[1], "Conv2d") and isa(ch[2], "Chain") and isa(ch[3], "Chain"), "unexpected Decoder layout")
        B, C, H, W = latents.shape
        ctx = UNetContext(self, B)
        with self.in_step():
            c0 = ch[0]
            _expect(c0.kernel_size == (1, 1) and c0.in_channels == C and c0.in_channels <= 8 and c0.out_channels <= 8, "unexpected post-quantisation conv")
            w0 = self.cache.get(("vae_pq", encoder_scale) + PackCache.ident(c0.weight),
                                lambda: (c0.weight.detach().to(self.device, torch.float32).reshape(c0.out_channels, c0.in_channels) / encoder_scale).to(self.dtype).contiguous())
            y0 = torch.empty(B, c0.out_channels, H, W, device=self.device, dtype=self.dtype)
            self.keepalive.append(y0)
            native.pointwise_nchw(latents, w0, self._w(c0.bias), y0)
            y = self._head(ch[3], self._stages(ch[2], self._stem_from(ch[1], y0), ctx, H, W, "Upsample"))
            if nchw_out is not None:
                native.nhwc_to_nchw(y.tokens(), nchw_out, y.C)
        return y

    def lower_tile_encoder(self, enc: Any, x0: Tensor, B: int, H: int, W: int, out: Tensor, encoder_scale: float) -> None:
        """lower_encoder from the token-major first activation x0 [B * H * W, cpad] (mi355x_vae_tile_gather wrote it, pad channels zero) to the NCHW
        latents `out` [B, 4, H / 8, W / 8]."""
        ch = kids(enc)
        _expect(len(ch) == 4 and isa(ch[0], "Conv2d") and all(isa(c, "Chain") for c in ch[1:]), "unexpected Encoder layout")
        ctx = UNetContext(self, B)
        with self.in_step():
            cur = self.conv(Act(x0, B, H, W), self._padded_conv_spec(ch[0], x0.shape[1], ch[0].out_channels))
            y = self._head(ch[2], self._stages(ch[1], cur, ctx, H, W, "Downsample"))
            quant, cut = kids(ch[3])
            _expect(isa(quant, "Conv2d") and quant.kernel_size == (1, 1) and isa(cut, "Slicing") and cut.dim == 1 and cut.start == 0 and cut.step == 1, "unexpected quantisation tail")
            keep = cut.end or quant.out_channels
            _expect(out.shape[1] == keep and quant.in_channels <= 8, "unexpected latent width")
            moments = torch.empty(B, y.C, y.H, y.W, device=self.device, dtype=self.dtype)
            self.keepalive.append(moments)
            native.nhwc_to_nchw(y.tokens(), moments, y.C)
            self.pool.put(y.t)
            wq = self.cache.get(("vae_q_w", encoder_scale, keep) + PackCache.ident(quant.weight),
                                lambda: (quant.weight.detach().to(self.device, torch.float32).reshape(quant.out_channels, quant.in_channels)[:keep] * encoder_scale).to(self.dtype).contiguous())
            bq = self.cache.get(("vae_q_b", encoder_scale, keep) + PackCache.ident(quant.bias),
                                lambda: (quant.bias.detach().to(self.device, torch.float32)[:keep] * encoder_scale).to(self.dtype).contiguous())
            native.pointwise_nchw(moments, wq, bq, out)


# ------------------------------------------------------------------------------------------------ engine
@dataclass
class _TileProgram:
    """One lowered encoder / decoder for `n` tiles of one size: its static input, its output and where a tile sits in the output (element strides)."""

    low: TiledVAELowering
    x: Tensor                  # what mi355x_vae_tile_gather writes
    gather: tuple              # (hw, (s_tile, s_c, s_y, s_x), cpad) of that call
    y: Tensor                  # the output the blend reads (flat view)
    y_strides: tuple           # (s_tile, s_c, s_y, s_x) inside y
    nchw: Optional[Tensor] = None  # one-tile decode: the image itself


@dataclass
class _Plan:
    """Static state of one canvas shape."""

    grid: Grid                                   # in the units of the output canvas
    canvas_in: Tensor
    canvas_out: Tensor
    chunks: list = field(default_factory=list)   # (program, pos, pos_host, n, arena offset)
    arena: Optional[Tensor] = None
    blend: tuple = ()
    graph: Any = None


class CompiledTiledVAE:
    """`CompiledTiledVAE(vae, tile_size=(width, height), blending, tile_batch)`: see the module docstring.  `stats` after a call: fallback_nodes, tile_groups
    [((h, w), list indices)], program_launches {(kind, h, w, n): launches}, gn_launches_per_program, graph_replayed."""

    def __init__(self, vae: Any, tile_size: tuple[int, int] = (512, 512), blending: int = 64, tile_batch: int = TILE_BATCH, use_graph: bool = True) -> None:
        native.load()
        assert tile_batch >= 1 and tile_size[0] % 8 == 0 and tile_size[1] % 8 == 0
        self.vae, self.tile_size, self.blending, self.tile_batch, self.use_graph = vae, tuple(tile_size), blending, tile_batch, use_graph
        self.cache = PackCache()
        self.tables: dict[int, NodeStats] = {}
        self.nodes: list[NodeStats] = []  # in walk order: the order of the reference's FixedGroupNorm nodes
        self.calibrated = False
        self.programs: dict[tuple, _TileProgram] = {}
        self.plans: dict[tuple, _Plan] = {}
        self.stats: dict[str, Any] = {}

    # -- statistics --------------------------------------------------------------------------------------------------------------------------
    def _groupnorms(self) -> list[tuple[Any, Any]]:
        """[(GroupNorm, its FixedGroupNorm or None)] in walk order (an injected FixedGroupNorm holds its target outside the module tree)."""
        out = []
        for m in self.vae.modules():
            if cname(m) == "FixedGroupNorm":
                out.append((m.target, m))
            elif isa(m, "GroupNorm"):
                out.append((m, None))
        return out

    def _alloc_tables(self, dev: torch.device) -> list[tuple[Any, Any]]:
        found = self._groupnorms()
        if [id(g) for g, _ in found] != [id(s.node) for s in self.nodes] or (self.nodes and self.nodes[0].tab.device != dev):
            self.nodes = [NodeStats(g, torch.zeros(g.num_channels, 2, dtype=torch.float32, device=dev), torch.zeros(g.num_groups, 2, dtype=torch.float32, device=dev)) for g, _ in found]
            self.tables = {id(s.node): s for s in self.nodes}
            self.programs, self.plans, self.calibrated = {}, {}, False
        return found

    @contextlib.contextmanager
    def _plain_tree(self) -> Iterator[None]:
        """The tree with its FixedGroupNorm adapters ejected for the time of a lowering (the matchers know the plain GroupNorm layout)."""
        fixed = [(f, f.parent) for _g, f in self._groupnorms() if f is not None]
        for f, _p in fixed:
            f.eject()
        try:
            yield
        finally:
            for f, p in fixed:
                f.inject(p)

    def _device_dtype(self) -> tuple[torch.device, torch.dtype]:
        p = next(self.vae.parameters())
        return p.device, p.dtype

    @torch.no_grad()
    def calibrate(self, x: Tensor) -> None:
        """x: (1, 3, tile_h, tile_w) in [-1, 1], what _add_fixed_group_norm feeds to encode.  Runs the lowered encoder, then the lowered decoder on the
        latents it produced; every GroupNorm's statistics are computed there and frozen."""
        dev, dtype = self._device_dtype()
        assert x.dim() == 4 and x.shape[0] == 1 and x.shape[2] % 8 == 0 and x.shape[3] % 8 == 0, "one image whose sides are multiples of 8"
        self._alloc_tables(dev)
        es = float(self.vae.encoder_scale)
        _, _, H, W = x.shape
        canvas = x.to(device=dev, dtype=dtype).contiguous()
        with self._plain_tree():
            low = TiledVAELowering(dev, dtype, self.cache, self.tables, "table")
            cpad = low.kblk
            x0 = torch.empty(H * W, cpad, device=dev, dtype=dtype)
            z = torch.empty(1, 4, H // 8, W // 8, device=dev, dtype=dtype)
            img = torch.empty(1, 3, H, W, device=dev, dtype=dtype)
            low.lower_tile_encoder(kids(self.vae)[0], x0, 1, H, W, z, es)
            low.lower_tile_decoder(kids(self.vae)[1], z, es, nchw_out=img)
        pos_host = native.vae_pos_rows([(0, 0)])
        native.vae_tile_gather(canvas, pos_host.to(dev), pos_host, x0, 1, (H, W), (H * W * cpad, 1, W * cpad, cpad), cpad=cpad)
        native.replay(low.step)
        torch.cuda.synchronize()
        low.handover_raise()
        self.cache.sweep()
        for s in self.nodes:
            s.ready = True
        self.calibrated = True
        self.plans = {}  # (captured graphs read the tables in place and would stay valid; the plans are cheap to rebuild and this keeps the rule simple)
        self.stats = dict(low.stats, calibration_launches=launches(low.step))

    @torch.no_grad()
    def adopt(self) -> None:
        """Take the statistics of the FixedGroupNorm nodes in the tree (mean and var set; weight and eps from their targets)."""
        dev, _ = self._device_dtype()
        found = self._alloc_tables(dev)
        if not found or any(f is None or f.mean is None or f.var is None for _g, f in found):
            raise ValueError("adopt() needs a FixedGroupNorm with statistics on every GroupNorm: call it inside `with vae.tiled_inference(image):`")
        for s, (g, f) in zip(self.nodes, found):
            mean, var = f.mean.detach().to(dev, torch.float32).reshape(-1), f.var.detach().to(dev, torch.float32).reshape(-1)
            _expect(mean.numel() == g.num_groups, "FixedGroupNorm statistics of a batch: the tiled paths take one image")
            cg = g.num_channels // g.num_groups
            s.raw.copy_(torch.stack((mean, var), dim=1))
            s.tab[:, 0] = mean.repeat_interleave(cg)
            s.tab[:, 1] = g.weight.detach().to(dev, torch.float32) / torch.sqrt(var + g.eps).repeat_interleave(cg)
            s.ready = True
        self.calibrated = True

    def statistics(self) -> tuple[Tensor, Tensor]:
        """(mean, var) [nodes, groups] in walk order, as the reference's FixedGroupNorm.mean / .var."""
        raw = torch.stack([s.raw for s in self.nodes])
        return raw[..., 0], raw[..., 1]

    # -- programs and plans ------------------------------------------------------------------------------------------------------------------
    def _program(self, kind: str, h: int, w: int, n: int, dev: torch.device, dtype: torch.dtype, whole: bool = False) -> _TileProgram:
        """kind "dec": n latent tiles of h x w; "enc": n pixel tiles of h x w.  `whole`: the one-tile case (the decoder then also writes NCHW)."""
        key = (kind, h, w, n, dev, dtype, whole, float(self.vae.encoder_scale))
        hit = self.programs.get(key)
        if hit is not None:
            return hit
        es = float(self.vae.encoder_scale)
        with self._plain_tree():
            low = TiledVAELowering(dev, dtype, self.cache, self.tables, "fixed")
            if kind == "dec":
                x = torch.empty(n, 4, h, w, device=dev, dtype=dtype)
                nchw = torch.empty(n, 3, 8 * h, 8 * w, device=dev, dtype=dtype) if whole else None
                y = low.lower_tile_decoder(kids(self.vae)[1], x, es, nchw_out=nchw)
                ld = y.t.stride(0)
                prog = _TileProgram(low, x, ((h, w), (4 * h * w, h * w, w, 1), 4), y.t.reshape(-1), (y.HW * ld, 1, y.W * ld, ld), nchw)
            else:
                cpad = low.kblk
                x = torch.empty(n * h * w, cpad, device=dev, dtype=dtype)
                out = torch.empty(n, 4, h // 8, w // 8, device=dev, dtype=dtype)
                low.lower_tile_encoder(kids(self.vae)[0], x, n, h, w, out, es)
                hl, wl = h // 8, w // 8
                prog = _TileProgram(low, x, ((h, w), (h * w * cpad, 1, w * cpad, cpad), cpad), out.reshape(-1), (4 * hl * wl, hl * wl, wl, 1), None)
        self.cache.sweep()
        self.programs[key] = prog
        return prog

    def _plan(self, kind: str, shape: tuple, dev: torch.device, dtype: torch.dtype) -> _Plan:
        key = (kind, shape, dev, dtype, self.tile_size, self.blending, self.tile_batch)
        hit = self.plans.get(key)
        if hit is not None:
            return hit
        H, W = shape[2], shape[3]
        lat = latent_grid((W // 8, H // 8) if kind == "enc" else (W, H), self.tile_size, self.blending)
        pix = lat.scaled(8, self.blending)  # _tiled_encode blends latents under ramps of blending // 8, _tiled_decode pixels under ramps of blending
        grid_in, grid_out = (pix, lat) if kind == "enc" else (lat, pix)
        cout = 4 if kind == "enc" else 3
        plan = _Plan(grid_out, torch.empty(shape, device=dev, dtype=dtype), torch.empty(1, cout, grid_out.size[1], grid_out.size[0], device=dev, dtype=dtype))
        tiles_in = grid_in.tiles
        groups = tile_groups(grid_in, self.tile_batch)
        whole = len(tiles_in) == 1
        placement: dict[int, tuple[int, int, int, int]] = {}
        off = 0
        for (h, w), idx in groups:
            prog = self._program(kind, h, w, len(idx), dev, dtype, whole)
            pos_host = native.vae_pos_rows([(tiles_in[i][0], tiles_in[i][1]) for i in idx])
            plan.chunks.append((prog, pos_host.to(dev), pos_host, len(idx), off))
            s_tile, s_c, s_y, s_x = prog.y_strides
            for r, i in enumerate(idx):
                placement[i] = (off + r * s_tile, s_c, s_y, s_x)
            off += prog.y.numel()
        if not whole:
            ramps, offs = ramp_tables(grid_out)
            axis_host = native.vae_axis_rows(grid_out.xs, grid_out.ys)
            tiles_host = native.vae_blend_rows(blend_rows(grid_out, placement, offs))
            plan.arena = torch.empty(off, device=dev, dtype=dtype)
            plan.blend = (ramps.to(dev), axis_host.to(dev), axis_host, tiles_host.to(dev), tiles_host)
        self.plans[key] = plan
        return plan

    def _launch(self, plan: _Plan) -> None:
        for prog, pos, pos_host, n, off in plan.chunks:
            hw, strides, cpad = prog.gather
            native.vae_tile_gather(plan.canvas_in, pos, pos_host, prog.x, n, hw, strides, cpad=cpad)
            native.replay(prog.low.step)
            if plan.arena is not None:
                plan.arena[off : off + prog.y.numel()].copy_(prog.y)
        if plan.arena is not None:
            g = plan.grid
            ramps, axis, axis_host, tiles, tiles_host = plan.blend
            native.vae_tile_blend(plan.canvas_out, plan.arena, ramps, axis, axis_host, tiles, tiles_host, (len(g.xs), len(g.ys)), g.stride, g.tile)

    def _run(self, kind: str, x: Tensor) -> Tensor:
        if not self.calibrated:
            raise ValueError("Tiled inference statistics are not set: call calibrate(x) or adopt() first.")
        dev, dtype = self._device_dtype()
        assert x.dim() == 4 and x.shape[0] == 1, "the tiled paths take one image (auto_encoder.py:480, 543)"
        for s, (g, _f) in zip(self.nodes, self._groupnorms()):
            assert s.node is g, "the autoencoder's GroupNorms changed since the statistics were taken"
        plan = self._plan(kind, tuple(x.shape), dev, dtype)
        plan.canvas_in.copy_(x)
        lows = [c[0].low for c in plan.chunks]
        fallbacks = [n for low in lows for n in low.stats["fallback_nodes"]]
        replayed = False
        if plan.graph is not None:
            plan.graph.replay()
            replayed = True
        else:
            self._launch(plan)  # also the warm-up: first-launch work must not be captured
            if self.use_graph and not fallbacks:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch(plan)
                plan.graph = g
        whole = plan.arena is None
        out = (plan.chunks[0][0].nchw if kind == "dec" else plan.chunks[0][0].y.view(plan.canvas_out.shape)) if whole else plan.canvas_out
        out = out.clone()  # (the clone waits for nothing; the hand-over check below synchronises)
        for low in {id(low): low for low in lows}.values():
            bad = low.handover_pending()
            if bad and bool(torch.stack(bad).any().item()):
                low.handover_raise()
        self.stats = {
            "fallback_nodes": fallbacks,
            "tile_groups": [(c[0].gather[0], c[3]) for c in plan.chunks],  # ((h, w) of the program's input tiles, tiles in the chunk)
            "tiles": len(plan.grid.xs) * len(plan.grid.ys),
            "program_launches": {(kind, *c[0].gather[0], c[3]): launches(c[0].low.step) for c in plan.chunks},
            "gn_launches_per_program": lows[0].stats.get("gn_fixed", 0),
            "graph_replayed": replayed,
        }
        return out

    @torch.no_grad()
    def encode(self, image: Tensor) -> Tensor:
        """(1, 3, 8h, 8w) in [-1, 1] -> latents (1, 4, h, w): lda._tiled_encode(image, tile_size, blending)."""
        assert image.shape[2] % 8 == 0 and image.shape[3] % 8 == 0, "the autoencoder downsamples by 8"
        return self._run("enc", image)

    @torch.no_grad()
    def decode(self, latents: Tensor) -> Tensor:
        """latents (1, 4, h, w) -> image (1, 3, 8h, 8w): lda._tiled_decode(latents, tile_size, blending)."""
        return self._run("dec", latents)
