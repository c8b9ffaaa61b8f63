"""MI355X lowering of MVANet (refiners_amd.mvanet, or refiners' own foundationals.swin.mvanet classes: `solutions.BoxSegmenter`).

Same engine as the Swin backbone it contains: the Chain tree is walked once and turned into a launch program; every activation is
channels-last token rows [views * S * S, E], the four local views first, the global view last.  PatchMerge / PatchSplit / Interpolate / Rescale
are index arithmetic inside the streaming kernels of csrc/mvanet.hip, never a copy.

  MultiheadAttention (one head, E = 128; torch's packed in_proj_weight)
      Q = x Wq^T + bq            GEMM; a sine position embedding of the queries enters as the row-bias table pos Wq^T + bq, made at lowering time
      K = keys Wk^T + bk         GEMM over the key rows padded to 64 (position embedding likewise)
      V^T = Wv keys^T            swapped-operand GEMM over the PADDED rows: the padding columns are written (zeros), never pool garbage.
                                 V's bias is not added here: softmax rows sum to one, so it is Wo bv in the out-projection's bias (float64 fold)
      mi355x_attention_general   H = 1, Dqk = Dv = E; the four patchwise attentions of a block share ONE launch (B = 4)
      out-projection + residual  GEMM
  MCRM   gate | pool (PatchSplit quadrants of the UNCHANGED global view, ratios 1, 2, 4) | 4 x (Q, K, V^T) | attention | 4 x out-proj |
         LayerNorm | FeedForward (ReLU epilogue) | LayerNorm | global + nearest_down(PatchMerge(local))
  MCLM   pool (PatchMerge of the local views, ratios 2, 8, 16) | Q, K, V^T with position tables | attention | out-proj | LayerNorm | FeedForward |
         LayerNorm | quadrants of the new global view (pool at ratio 1) | 4 x (Q, K, V^T) | attention | 4 x out-proj | the same LayerNorms and a second FeedForward
  CBR / CBG   BatchNorm's running statistics and affine folded into the convolution's weight and bias in float64 at pack time; GELU is the
         convolution's epilogue, Rescale(2) its loader; PReLU rides in the resize-add that consumes the map, or is an in-place pass where
         the consumer is a convolution or the map has several readers.  PReLU slopes are read from the tree's own storage: live.
  MVANet split_views | Swin (SwinLowering, token outputs) | pyramid | RearrangeMultiView | ShallowUpscaler | Conv2d(E -> n_logits) on padded
         output channels.  The shallow map conv3x3(image) is materialised once ([1024^2, E]) and sampled by the two bilinear resize-adds.

Refused (Unsupported: the stock forward runs instead, behind a RuntimeWarning): an input that is not 1 x 3 x 1024 x 1024, BatchNorm in
training mode, num_heads != 1, an embedding width that is not 128, LoRA on any layer, whatever SwinLowering refuses.
"""
from __future__ import annotations

import math
import warnings
from types import SimpleNamespace
from typing import Any, Optional

import torch
from torch import Tensor

from .. import native
from ..fluxion.tree import tree_epoch
from .compiled import Program
from .packing import Act, ConvSpec, PackCache, Unsupported, _expect, cname, isa, kids, launches
from .swin import SwinLowering, output_shapes

EMB = 128  # the head width the decoder's attention runs at (mi355x_attention_general instance (4, 8))
SIDE = 1024  # the one input side the reference's hard-wired sizes admit


# -------------------------------------------------------------------------------------------------------- host tables and folds
def position_embedding(h: int, w: int, E: int) -> Tensor:
    """[h w, E] float32: DETR's sine embedding as PositionEmbeddingSine(E // 2)(h, w) gives it, columns (y features | x features)."""
    n = E // 2
    i = torch.arange(n, dtype=torch.float32)
    dim_t = 10000 ** (2 * (i // 2) / n)
    y = (torch.arange(1, h + 1, dtype=torch.float32) - 0.5) / (h + 1e-6) * (2 * math.pi)
    x = (torch.arange(1, w + 1, dtype=torch.float32) - 0.5) / (w + 1e-6) * (2 * math.pi)

    def feats(p: Tensor) -> Tensor:
        a = p[:, None] / dim_t
        return torch.stack((a[:, 0::2].sin(), a[:, 1::2].cos()), dim=2).flatten(1)

    fy, fx = feats(y), feats(x)
    return torch.cat((fy[:, None, :].expand(h, w, n), fx[None, :, :].expand(h, w, n)), dim=2).reshape(h * w, E)


def pool_positions(G: int, ratios: list[int], E: int) -> Tensor:
    """Position embedding of MultiPool's rows of a G x G map: the embedding of each pooled grid, one ratio after the other."""
    return torch.cat([position_embedding(G // r, G // r, E) for r in ratios])


def merged_rows(S: int) -> Tensor:
    """[2S, 2S] int64: the row of pixel (Y, X) of PatchMerge(four views of side S) in the stacked views -- the kernels' `merged_row`."""
    Y, X = torch.meshgrid(torch.arange(2 * S), torch.arange(2 * S), indexing="ij")
    return ((2 * (Y // S) + X // S) * S + Y % S) * S + X % S


def quadrant_rows(S: int, q: int) -> Tensor:
    """[S / 2, S / 2] int64: the rows of quadrant q = 2 qy + qx (PatchSplit) of one view of side S."""
    G = S // 2
    y, x = torch.meshgrid(torch.arange(G), torch.arange(G), indexing="ij")
    return ((q >> 1) * G + y) * S + (q & 1) * G + x


def pool_model(tokens: Tensor, rows: Tensor, ratios: list[int]) -> Tensor:
    """Host restatement of mi355x_mvanet_pool: tokens [n, E], rows [G, G] (merged_rows or quadrant_rows) -> [sum (G / r)^2, E]."""
    G = rows.shape[0]
    m = tokens[rows.reshape(-1)].reshape(G, G, -1)
    return torch.cat([m.reshape(G // r, r, G // r, r, -1).mean(dim=(1, 3)).reshape((G // r) ** 2, -1) for r in ratios])


def fold_batchnorm(w: Tensor, b: Optional[Tensor], bn: Any) -> tuple[Tensor, Tensor]:
    """conv -> BatchNorm2d.eval() as one convolution, in float64: w' = w g / sqrt(var + eps) per output channel, b' = (b - mean) g / sqrt(var + eps) + beta."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    b0 = b.detach().double() if b is not None else torch.zeros_like(s)
    return w.detach().double() * s.view(-1, 1, 1, 1), (b0 - bn.running_mean.detach().double()) * s + bn.bias.detach().double()


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


class MVANetLowering(SwinLowering):
    def __init__(self, *args: Any, **kwargs: Any) -> None:
        super().__init__(*args, **kwargs)
        self.gn_stats = False  # no GroupNorm reads these convolutions' outputs: no column statistics from their epilogues
        self.taps: Optional[dict] = None  # a dict: lower_net leaves copies of the Pyramid and RearrangeMultiView outputs in it (tests locate a failure with them)

    def tap(self, name: str, a: Act, slope: Optional[Tensor] = None) -> None:
        if self.taps is not None:
            t = self.hold(torch.empty_like(a.t))
            native.axpby(a.t, 1.0, a.t, 0.0, t)
            if slope is not None:
                native.mvanet_prelu(t, slope)
            self.taps[name] = Act(t, a.B, a.H, a.W)

    # ---------------------------------------------------------------------------------------------------------------- pieces
    def hold(self, t: Tensor) -> Tensor:
        self.__dict__.setdefault("_keep_alive", []).append(t)
        return t

    def slope(self, act: Any) -> Tensor:
        """The PReLU's one slope where the kernels read it: the tree's own storage when it already is of the compute dtype on the device (live)."""
        _expect(isa(act, "PReLU") and act.weight.numel() == 1, f"expected a single-slope PReLU, got {cname(act)}")
        return self._w(act.weight)

    def mha_pack(self, mha: Any, pos_q: Optional[Tensor], pos_k: Optional[Tensor], lkp: int) -> dict:
        _expect(isa(mha, "MultiheadAttention"), f"expected a MultiheadAttention, got {cname(mha)}")
        _expect(mha.num_heads == 1, f"{mha.num_heads} attention heads (the decoder's attention is lowered for one)")
        E = mha.embed_dim
        _expect(E == EMB, f"embedding width {E} (the decoder's kernels take {EMB})")
        _expect(mha.in_proj_weight is not None and mha.in_proj_bias is not None and mha.bias_k is None and not mha.add_zero_attn and not mha.batch_first,
                "unexpected MultiheadAttention configuration")
        wi, bi, wo, bo = mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias

        def make() -> dict:
            w64, b64 = wi.detach().to(self.device).double(), bi.detach().to(self.device).double()
            p = {n: w64[j * E : (j + 1) * E].to(self.dtype).contiguous() for j, n in enumerate(("wq", "wk", "wv"))}
            p["bq"], p["bk"] = b64[:E].to(self.dtype).contiguous(), b64[E : 2 * E].to(self.dtype).contiguous()
            wo64 = wo.detach().to(self.device).double()
            p["wo"] = wo64.to(self.dtype).contiguous()
            p["bo"] = (bo.detach().to(self.device).double() + wo64 @ b64[2 * E :]).to(self.dtype).contiguous()  # softmax rows sum to 1: P (V + 1 bv^T) Wo^T = P V Wo^T + Wo bv
            if pos_q is not None:
                p["tq"] = (pos_q.to(self.device).double() @ w64[:E].T + b64[:E]).to(self.dtype).contiguous()
            if pos_k is not None:
                tk = torch.zeros(lkp, E, device=self.device, dtype=torch.float64)
                tk[: pos_k.shape[0]] = pos_k.to(self.device).double() @ w64[E : 2 * E].T + b64[E : 2 * E]
                p["tk"] = tk.to(self.dtype).contiguous()
            return p

        return self.cache.get(("mvanet_mha", pos_q is not None, pos_k is not None, lkp) + PackCache.ident(wi, bi, wo, bo), make)

    def project(self, mha: Any, xq: Tensor, keys: Tensor, q: Tensor, k: Tensor, vt: Tensor, pos_q: Optional[Tensor] = None, pos_k: Optional[Tensor] = None) -> dict:
        """Q, K and V^T of one MultiheadAttention into the given slices: xq [Lq, E] -> q [Lq, E]; keys [Lkp, E] (padding rows zero) -> k [Lkp, E], vt [E, Lkp]."""
        p = self.mha_pack(mha, pos_q, pos_k, keys.shape[0])
        if pos_q is None:
            native.gemm([(xq, self.kblocked(p["wq"]))], q, bias=p["bq"])
        else:
            native.gemm([(xq, self.kblocked(p["wq"]))], q, rowbias=p["tq"], rows_per_group=1)
        if pos_k is None:
            native.gemm([(keys, self.kblocked(p["wk"]))], k, bias=p["bk"])
        else:
            native.gemm([(keys, self.kblocked(p["wk"]))], k, rowbias=p["tk"], rows_per_group=1)
        native.gemm([(self.kblocked(p["wv"]), keys)], vt, weight_operand="x")
        return p

    def attend(self, q: Tensor, k: Tensor, vt: Tensor, B: int, Lk: int) -> Tensor:
        """q [B Lq, E], k [B Lkp, E], vt [E, B Lkp] -> [B Lq, E], one launch."""
        E = q.shape[1]
        Lq, lkp = q.shape[0] // B, k.shape[0] // B
        o = self.pool.get(B * Lq, E)
        native.attention_general(q.view(B, Lq, E), k.view(B, lkp, E), vt.view(E, B, lkp), o.view(B, Lq, E), 1, Lk)
        return o

    def patchwise(self, pca: Any, xq: Tensor, keys: Tensor, Lk: int, out: Tensor) -> None:
        """PatchwiseCrossAttention + its residual: out[v] = xq[v] + MHA_v(xq[v], keys[v], keys[v]) for the four local views; xq, out [4 Lq, E]
        (out may be xq), keys [4 Lkp, E] with zero padding rows."""
        ch = kids(pca)
        _expect(isa(pca, "PatchwiseCrossAttention") and len(ch) == 2 and isa(ch[0], "Concatenate") and len(kids(ch[0])) == 4, "unexpected PatchwiseCrossAttention layout")
        mhas = []
        for n, br in enumerate(kids(ch[0])):
            bc = kids(br)
            _expect(len(bc) == 2 and isa(bc[0], "_GetArgs") and isa(bc[1], "MultiheadAttention"), "unexpected PatchwiseCrossAttention branch")
            sl = [kids(c)[1] for c in kids(bc[0])]
            _expect(all((s.start, s.end) == (n, n + 1) for s in sl), "PatchwiseCrossAttention branch reads another view")
            mhas.append(bc[1])
        E = xq.shape[1]
        Lq, lkp = xq.shape[0] // 4, keys.shape[0] // 4
        q, k, vt = self.pool.get(4 * Lq, E), self.pool.get(4 * lkp, E), self.pool.get(E, 4 * lkp)
        packs = [self.project(m, xq[v * Lq : (v + 1) * Lq], keys[v * lkp : (v + 1) * lkp], q[v * Lq : (v + 1) * Lq], k[v * lkp : (v + 1) * lkp], vt[:, v * lkp : (v + 1) * lkp])
                 for v, m in enumerate(mhas)]
        o = self.attend(q, k, vt, 4, Lk)
        for v, p in enumerate(packs):
            rows = slice(v * Lq, (v + 1) * Lq)
            native.gemm([(o[rows], self.kblocked(p["wo"]))], out[rows], bias=p["bo"], res=xq[rows])
        for t in (q, k, vt, o):
            self.pool.put(t)

    def feed_forward_relu(self, ff: Any, x: Tensor, out: Tensor) -> None:
        """FeedForward: out = x + W2 relu(W1 x + b1) + b2 (out may be x)."""
        ch = kids(ff)
        _expect(isa(ff, "Residual") and len(ch) == 3 and isa(ch[1], "ReLU"), "unexpected FeedForward layout")
        s1, s2 = self.plain_linear(ch[0]), self.plain_linear(ch[2])
        h = self.pool.get(x.shape[0], s1.N)
        native.gemm([(x, self.kblocked(s1.w))], h, bias=s1.b, relu=True)
        native.gemm([(h, self.kblocked(s2.w))], out, bias=s2.b, res=x)
        self.pool.put(h)

    def ln(self, node: Any, x: Tensor, out: Tensor) -> Tensor:
        _expect(isa(node, "LayerNorm") and tuple(node.normalized_shape) == (x.shape[1],), "LayerNorm shape mismatch")
        return native.layernorm(x, self._w(node.weight), self._w(node.bias), node.eps, out)

    @staticmethod
    def ratios_of(multipool: Any) -> list[int]:
        _expect(isa(multipool, "MultiPool") and 1 <= len(kids(multipool)) <= native.MVANET_MAX_RATIOS, "unexpected MultiPool layout")
        return [kids(c)[0].ratio for c in kids(multipool)]

    # ---------------------------------------------------------------------------------------------------------------- blocks
    def mcrm(self, blk: Any, x: Tensor, S: int, out: Tensor) -> None:
        """x, out: [5 S S, E] (distinct buffers)."""
        ch = kids(blk)
        _expect(isa(blk, "MCRM") and len(ch) == 4 and all(isa(c, "Parallel") for c in ch[:3]) and isa(ch[3], "Concatenate"), "unexpected MCRM layout")
        mul, tca = kids(ch[1])[0], kids(ch[2])[0]
        _expect(isa(mul, "Multiply") and isa(tca, "TiledCrossAttention"), "unexpected MCRM layout")
        gc = kids(kids(mul)[1])
        _expect([cname(c) for c in gc] == ["GetArg", "Conv2d", "Sigmoid", "Interpolate", "PatchSplit"] and gc[3].mode == "nearest" and tuple(gc[3].size) == (2 * S, 2 * S),
                f"unexpected MCRM gate (the block is built for views of {tuple(gc[3].size)[0] // 2}, got {S})")
        conv = gc[1]
        _expect(conv.kernel_size == (1, 1) and conv.out_channels == 1 and conv.in_channels == x.shape[1] and conv.bias is not None, "unexpected gate convolution")
        tc = kids(tca)
        _expect(len(tc) == 7 and isa(tc[0], "Distribute") and isa(tc[1], "Sum") and isa(tc[2], "LayerNorm") and isa(tc[4], "LayerNorm"), "unexpected TiledCrossAttention layout")
        ratios = self.ratios_of(kids(kids(tc[0])[1])[2])
        pca = kids(kids(tc[1])[1])[0]
        down = kids(kids(kids(ch[3])[1])[0])[1]
        _expect(isa(kids(down)[2], "Interpolate") and kids(down)[2].mode == "nearest" and tuple(kids(down)[2].size) == (S, S), "unexpected MCRM global update")
        n, E = S * S, x.shape[1]
        _expect(S % 2 == 0 and all((S // 2) % r == 0 for r in ratios), f"views of side {S} cannot be pooled at {ratios}")
        local, glb = x[: 4 * n], x[4 * n :]
        lg = self.pool.get(4 * n, E)
        native.mvanet_gate(local, glb, self._w(conv.weight).view(-1), self._w(conv.bias), lg, S)
        Lk = native.mvanet_pool_rows(S // 2, ratios)
        keys = self.pool.get(4 * pad64(Lk), E)
        native.mvanet_pool(glb, S, ratios, keys.view(4, pad64(Lk), E), split=True)
        self.patchwise(pca, lg, keys, Lk, lg)
        self.pool.put(keys)
        h = self.pool.get(4 * n, E)
        self.ln(tc[2], lg, h)
        self.feed_forward_relu(tc[3], h, h)
        self.ln(tc[4], h, out[: 4 * n])
        self.pool.put(h)
        self.pool.put(lg)
        native.mvanet_resize_add(out[: 4 * n], (2 * S, 2 * S), glb, out[4 * n :], (S, S), mode="nearest", x_merge=True)

    def mclm(self, blk: Any, x: Tensor, S: int, out: Tensor) -> None:
        """x, out: [5 S S, E] (distinct buffers); the reference's Unflatten(0, (2, 8, 2, 8)) fixes S = 16."""
        ch = kids(blk)
        names = ["Parallel", "Lambda", "Converter", "GlobalAttention", "LayerNorm", "FeedForward", "LayerNorm", "SetContext", "UseContext", "Flatten", "Permute", "Residual",
                 "Lambda", "FeedForward", "Lambda", "Concatenate", "Unflatten", "Permute"]
        _expect(isa(blk, "MCLM") and [cname(c) for c in ch] == names, "unexpected MCLM layout")
        _expect(S == 16 and tuple(ch[16].sizes) == (16, 16), f"MCLM runs on five 16 x 16 views, got {S}")
        ln1, ln2 = ch[4], ch[6]
        for lam, ln in ((ch[12], ln1), (ch[14], ln2)):
            _expect(any(c.cell_contents is ln for c in (lam.func.__closure__ or ())), "the second use of an MCLM LayerNorm is not a proxy of the first")
        ratios = self.ratios_of(kids(kids(kids(kids(ch[0])[1])[3])[0])[0])
        mha = kids(kids(kids(ch[3])[0])[1])[1]
        pca = kids(ch[11])[1]
        n, E = S * S, x.shape[1]
        G = 2 * S
        _expect(all(G % r == 0 for r in ratios), f"a {G} x {G} map cannot be pooled at {ratios}")
        local, glb = x[: 4 * n], x[4 * n :]
        Lk = native.mvanet_pool_rows(G, ratios)
        keys = self.pool.get(pad64(Lk), E)
        native.mvanet_pool(local, S, ratios, keys, split=False)
        q, k, vt = self.pool.get(n, E), self.pool.get(pad64(Lk), E), self.pool.get(E, pad64(Lk))
        p = self.project(mha, glb, keys, q, k, vt, pos_q=position_embedding(S, S, E), pos_k=pool_positions(G, ratios, E))
        o = self.attend(q, k, vt, 1, Lk)
        g1 = self.pool.get(n, E)
        native.gemm([(o, self.kblocked(p["wo"]))], g1, bias=p["bo"], res=glb)
        for t in (keys, q, k, vt, o):
            self.pool.put(t)
        g2 = self.pool.get(n, E)
        self.ln(ln1, g1, g2)
        self.feed_forward_relu(ch[5], g2, g2)
        gout = out[4 * n :]
        self.ln(ln2, g2, gout)
        self.pool.put(g1)
        self.pool.put(g2)
        # each local view attends to its quadrant of the new global view: PatchSplit rows = a pool at ratio 1
        quad = self.pool.get(4 * pad64(n // 4), E)
        native.mvanet_pool(gout, S, [1], quad.view(4, pad64(n // 4), E), split=True)
        l1 = self.pool.get(4 * n, E)
        self.patchwise(pca, local, quad, n // 4, l1)
        self.pool.put(quad)
        l2 = self.pool.get(4 * n, E)
        self.ln(ln1, l1, l2)
        self.feed_forward_relu(ch[13], l2, l2)
        self.ln(ln2, l2, out[: 4 * n])
        self.pool.put(l1)
        self.pool.put(l2)

    def lower_block(self, blk: Any, x: Tensor, out: Tensor) -> None:
        """One MCLM or MCRM: x [5 S S, E] -> out [5 S S, E], both static."""
        _expect(x.dim() == 2 and x.shape[1] == EMB and x.shape[0] % 5 == 0 and math.isqrt(x.shape[0] // 5) ** 2 == x.shape[0] // 5, f"expected [5 S S, {EMB}] token rows, got {tuple(x.shape)}")
        self.check_tree(blk)
        S = math.isqrt(x.shape[0] // 5)
        with self.in_step():
            (self.mclm if isa(blk, "MCLM") else self.mcrm)(blk, x, S, out)

    # ---------------------------------------------------------------------------------------------------------------- the network
    def check_tree(self, tree: Any) -> None:
        for m in tree.modules():
            _expect(not isa(m, "LoraAdapter", "Lora"), "LoRA on an MVANet layer is not lowered")
            _expect(not (isa(m, "BatchNorm2d") and m.training), "BatchNorm in training mode (the fold needs the running statistics: call .eval())")
            _expect(not isa(m, "BatchNorm2d") or (m.track_running_stats and m.affine and m.running_mean is not None), "BatchNorm without running statistics or affine")

    def folded_conv(self, conv: Any, bn: Any, cin_pad: int = 0, cout_pad: int = 0) -> tuple[ConvSpec, Optional[Tensor]]:
        """Conv2d 3x3 (+ BatchNorm2d in eval mode) as a ConvSpec; cin_pad / cout_pad: zero-padded channel counts for widths below the kernel's granularity.
        Second result: under bfloat16 the folded bias is a NEW number whose rounding would shift a whole channel (the per-channel means of the
        logits see it), so it is kept as two bfloat16 terms: the ConvSpec's bias and this [1, cout] remainder, which the launch adds as a row bias."""
        _expect(isa(conv, "Conv2d") and conv.kernel_size == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1) and conv.groups == 1 and tuple(conv.dilation) == (1, 1),
                "unexpected decoder convolution")
        o, i = conv.out_channels, conv.in_channels
        ci, co = cin_pad or i, cout_pad or o
        _expect((ci * self.es) % 128 == 0, f"conv in_channels {ci} not 128-byte aligned")
        _expect(bn is None or (isa(bn, "BatchNorm2d") and bn.num_features == o), "unexpected BatchNorm")
        srcs = (conv.weight, conv.bias) + ((bn.weight, bn.bias, bn.running_mean, bn.running_var) if bn is not None else ())

        def pack() -> tuple[Tensor, Tensor]:
            w64 = conv.weight.detach().to(self.device).double()
            b64 = conv.bias.detach().to(self.device).double() if conv.bias is not None else torch.zeros(o, device=self.device, dtype=torch.float64)
            if bn is not None:
                w64, b64 = fold_batchnorm(w64, b64, _on(bn, self.device))
            w = torch.zeros(co, ci, 3, 3, device=self.device, dtype=self.dtype)
            w[:o, :i] = w64.to(self.dtype)
            b = torch.zeros(co, device=self.device, dtype=self.dtype)
            b[:o] = b64.to(self.dtype)
            lo = torch.zeros(1, co, device=self.device, dtype=self.dtype)
            lo[0, :o] = (b64 - b[:o].double()).to(self.dtype)
            return native.pack_conv_weight(w), b, lo

        wp, bp, lo = self.cache.get(("mvanet_conv", ci, co, float(bn.eps) if bn is not None else None) + PackCache.ident(*srcs), pack)
        return ConvSpec(wp, bp, ci, co, 3, 1), (lo if bn is not None and self.dtype != torch.float32 else None)

    def fconv(self, a: Act, conv: Any, bn: Any = None, cin_pad: int = 0, cout_pad: int = 0, ups: int = 1, gelu: bool = False) -> Act:
        spec, lo = self.folded_conv(conv, bn, cin_pad, cout_pad)
        rb = None if lo is None else self.cache.get(("mvanet_bias_lo", a.B) + PackCache.ident(lo), lambda: lo.expand(a.B, -1).contiguous())
        return self.conv(a, spec, rowbias=rb, ups=ups, gelu=gelu)

    def cbx(self, node: Any, kind: str) -> tuple[Any, Any, Any]:
        ch = kids(node)
        _expect(isa(node, kind) and len(ch) == 3 and isa(ch[0], "Conv2d") and isa(ch[1], "BatchNorm2d") and isa(ch[2], "PReLU" if kind == "CBR" else "GeLU"), f"unexpected {kind} layout")
        if kind == "CBG":
            _expect(ch[2].approximation.value == "none", "only the erf GeLU is an epilogue")
        return ch[0], ch[1], ch[2]

    def cbr(self, node: Any, a: Act, apply: bool = False) -> tuple[Act, Tensor]:
        """CBR -> (the convolution's output BEFORE the PReLU, the slope); apply: run the in-place PReLU pass now."""
        conv, bn, act = self.cbx(node, "CBR")
        y = self.fconv(a, conv, bn)
        s = self.slope(act)
        if apply:
            native.mvanet_prelu(y.t, s)
        return y, s

    def lateral(self, node: Any, index: int, feats: list[Act]) -> tuple[Act, Tensor]:
        ch = kids(node)
        _expect(len(ch) == 4 and isa(ch[0], "GetArg") and ch[0].index == index and isa(ch[1], "Flatten") and isa(ch[2], "CBR") and isa(ch[3], "Unflatten"), "unexpected lateral branch")
        return self.cbr(ch[2], feats[index])

    def pyramid(self, node: Any, feats: list[Act], level: int) -> tuple[Act, Optional[Tensor], int]:
        """Pyramid / PyramidL2..L5 -> (the level's last convolution output or MCLM output, its pending PReLU slope or None, the side its Interpolate asks for)."""
        ch = kids(node)
        if isa(node, "PyramidL5"):
            _expect([cname(c) for c in ch] == ["GetArg", "Flatten", "CBR", "Unflatten", "MCLM", "Flatten", "Interpolate"] and ch[0].index == 0 and ch[6].mode == "bilinear", "unexpected PyramidL5 layout")
            y, _s = self.cbr(ch[2], feats[0], apply=True)  # MCLM reads its input several times
            out = self.pool.get(y.M, y.C)
            self.mclm(ch[4], y.t, y.H, out)
            self.pool.put(y.t)
            return Act(out, 5, y.H, y.W), None, ch[6].size[0]
        _expect(len(ch) == 5 and isa(ch[0], "Sum") and isa(ch[1], "MCRM") and isa(ch[2], "Flatten") and isa(ch[3], "CBR"), f"unexpected {cname(node)} layout")
        deeper, lat = kids(ch[0])
        a, sa, side = self.pyramid(deeper, feats, level - 1)
        b, sb = self.lateral(lat, level, feats)
        _expect(side == b.H, f"{cname(deeper)} resizes to {side}, the lateral map has {b.H}")
        native.mvanet_resize_add(a.t, (a.H, a.W), b.t, b.t, (b.H, b.W), B=5, mode="bilinear", slope_x=sa, slope_y=sb)
        self.pool.put(a.t)
        m = self.pool.get(b.M, b.C)
        self.mcrm(ch[1], b.t, b.H, m)
        self.pool.put(b.t)
        y, s = self.cbr(ch[3], Act(m, 5, b.H, b.W))
        self.pool.put(m)
        if isa(ch[4], "Interpolate"):
            _expect(ch[4].mode == "bilinear", "unexpected pyramid Interpolate")
            return y, s, ch[4].size[0]
        return y, s, y.H

    def lower_net(self, net: Any, image: Tensor, logits: Tensor) -> None:
        """image [1, 3, 1024, 1024] (static) -> logits [1, n_logits, 1024, 1024] (static)."""
        ch = kids(net)
        names = ["ComputeShallow", "SplitMultiView", "Flatten", "SwinTransformer", "Distribute", "Pyramid", "RearrangeMultiView", "ShallowUpscaler", "Conv2d"]
        _expect(isa(net, "MVANet") and [cname(c) for c in ch] == names, "unexpected MVANet layout")
        _expect(tuple(image.shape) == (1, 3, SIDE, SIDE), f"input {tuple(image.shape)} (MVANet's hard-wired sizes admit 1 x 3 x {SIDE} x {SIDE} only)")
        self.check_tree(net)
        H = SIDE
        views = self.hold(torch.empty(5, 3, H // 2, H // 2, device=self.device, dtype=self.dtype))
        shapes = output_shapes(ch[3], 5, H // 2)
        toks = [self.hold(torch.empty(b * g * g2, c, device=self.device, dtype=self.dtype)) for (b, c, g, g2) in shapes]
        with self.in_step():
            native.mvanet_split_views(image, views)
        self.lower(ch[3], views, toks, as_tokens=True)
        feats = [Act(t, 5, s[2], s[3]) for t, s in zip(toks, shapes)]
        with self.in_step():
            # shallow = conv3x3(image), channels zero-padded to one K block
            sc = kids(ch[0])
            _expect(len(sc) == 2 and isa(sc[0], "Conv2d") and isa(sc[1], "SetContext"), "unexpected ComputeShallow layout")
            cpad = self.kblk
            x0 = self.hold(torch.zeros(H * H, cpad, device=self.device, dtype=self.dtype))
            a0 = Act(x0, 1, H, H)
            native.nchw_to_nhwc(image, a0.tokens())
            shallow = self.fconv(a0, sc[0], cin_pad=cpad)
            self.pool.pin(shallow.t)
            E = shallow.C
            _expect(E == EMB, f"embedding width {E} (the decoder's kernels take {EMB})")
            y, s, _side = self.pyramid(ch[5], feats, 4)
            self.tap("pyramid", y, s)
            # RearrangeMultiView: PatchMerge(local) + bilinear(global), the pending PReLU of the pyramid's last CBR on both
            rc = kids(ch[6])
            _expect(len(rc) == 2 and isa(rc[0], "Sum") and isa(rc[1], "Chain") and [cname(c) for c in kids(rc[1])] == ["CBR", "CBR", "Conv2d"], "unexpected RearrangeMultiView layout")
            S = y.H
            n = S * S
            m = self.pool.get(4 * n, E)
            native.mvanet_resize_add(y.t[4 * n :], (S, S), y.t[: 4 * n], m, (2 * S, 2 * S), mode="bilinear", slope_x=s, slope_y=s, y_merge=True)
            self.pool.put(y.t)
            cur = Act(m, 1, 2 * S, 2 * S)
            for node in kids(rc[1])[:2]:
                nxt, _s = self.cbr(node, cur, apply=True)  # the consumer is a convolution
                self.pool.put(cur.t)
                cur = nxt
            nxt = self.fconv(cur, kids(rc[1])[2])
            self.pool.put(cur.t)
            cur = nxt
            self.tap("rearrange", cur)
            # ShallowUpscaler
            uc = kids(ch[7])
            _expect(len(uc) == 4 and isa(uc[0], "Sum") and isa(uc[1], "Sum") and isa(uc[2], "Rescale") and isa(uc[3], "CBG"), "unexpected ShallowUpscaler layout")
            up1 = kids(kids(uc[1])[0])
            _expect(isa(up1[0], "Rescale") and up1[0].scale_factor == 2 and up1[0].mode == "nearest" and uc[2].scale_factor == 2 and uc[2].mode == "nearest", "unexpected Rescale")
            native.mvanet_resize_add(shallow.t, (H, H), cur.t, cur.t, (cur.H, cur.W), mode="bilinear")
            conv, bn, _g = self.cbx(up1[1], "CBG")
            nxt = self.fconv(cur, conv, bn, ups=2, gelu=True)
            self.pool.put(cur.t)
            cur = nxt
            native.mvanet_resize_add(shallow.t, (H, H), cur.t, cur.t, (cur.H, cur.W), mode="bilinear")
            conv, bn, _g = self.cbx(uc[3], "CBG")
            nxt = self.fconv(cur, conv, bn, ups=2, gelu=True)
            self.pool.put(cur.t)
            cur = nxt
            n_logits = ch[8].out_channels
            _expect(tuple(logits.shape) == (1, n_logits, H, H) and cur.H == H, "logits of another shape")
            last = self.fconv(cur, ch[8], cout_pad=pad64(n_logits))
            self.pool.put(cur.t)
            native.nhwc_to_nchw(last.tokens(), logits, n_logits)
            self.pool.put(last.t)


def _on(bn: Any, device: torch.device) -> Any:
    """The BatchNorm's tensors on `device` under the attribute names fold_batchnorm reads."""
    return SimpleNamespace(eps=bn.eps, **{k: getattr(bn, k).detach().to(device) for k in ("weight", "bias", "running_mean", "running_var")})


class _Compiled:
    """Shared by the block and whole-net entry points: one program per (tree state, input shape, dtype, weight versions), replayed as a HIP graph."""

    what = ""

    def __init__(self, tree: Any, dtype: Optional[torch.dtype] = None, use_graph: bool = True) -> None:
        native.load()
        self.tree = tree
        self.dtype = dtype
        self.use_graph = use_graph
        self.cache = PackCache()
        self.key: Any = None
        self.bad_key: Any = None
        self.lowerings = 0
        self.stats: dict[str, Any] = {}
        self.keep_intermediates = False  # CompiledMVANet: also return the Pyramid and RearrangeMultiView outputs, in `intermediates`
        self.intermediates: dict[str, Tensor] = {}

    def _tree_dtype(self) -> torch.dtype:
        return next(p.dtype for p in self.tree.parameters())

    def _weights_version(self, dtype: torch.dtype) -> int:
        """Versions of the tensors a program holds COPIES of: an in-place edit of one re-lowers.  PReLU slopes (and Swin's float32 bias tables)
        of the compute dtype are read where they are."""
        live = lambda n, p: (n.endswith("relative_position_bias_table") and p.dtype == torch.float32 == dtype) or (n.rsplit(".", 2)[-2].startswith("PReLU") and p.dtype == dtype)  # noqa: E731
        return sum(p._version for n, p in self.tree.named_parameters() if not live(n, p)) + sum(b._version for b in self.tree.buffers())

    def _modes(self) -> tuple:
        return tuple(m.training for m in self.tree.modules() if isa(m, "BatchNorm2d"))

    def _lower(self, low: MVANetLowering, x: Tensor) -> Tensor:
        raise NotImplementedError

    def _stock(self, x: Tensor) -> Tensor:
        raise NotImplementedError

    @torch.no_grad()
    def __call__(self, x: Tensor) -> Tensor:
        dtype = self.dtype or self._tree_dtype()
        key = (tree_epoch(), tuple(x.shape), dtype, x.device, self._weights_version(dtype), self._modes(), self.keep_intermediates)
        if key == self.bad_key:
            return self._stock(x)
        if key != self.key:
            try:
                self.x = torch.empty(tuple(x.shape), device=x.device, dtype=dtype)
                low = MVANetLowering(x.device, dtype, self.cache, "merged")
                low.taps = {} if self.keep_intermediates else None
                self.out = self._lower(low, self.x)
            except Unsupported as e:
                warnings.warn(f"{self.what}: {e}; running the stock forward", RuntimeWarning, stacklevel=2)
                self.bad_key = key
                return self._stock(x)
            self.cache.sweep()
            self.low, self.key = low, key
            self.lowerings += 1
            self.program = Program(low.step, self.use_graph, low=low)
            self.stats = dict(low.stats, step_ops=launches(low.step), pool_bytes=low.step_pool.bytes(), lowerings=self.lowerings)
        self.x.copy_(x)
        self.program.run()
        self.intermediates = {k: a.image().permute(0, 3, 1, 2).clone() for k, a in (self.low.taps or {}).items()}
        return self.out.clone()


class CompiledMVANet(_Compiled):
    """`fast = CompiledMVANet(mvanet); logits = fast(image)` == `mvanet(image)` for the one input the model admits, 1 x 3 x 1024 x 1024:
    [1, n_logits, 1024, 1024].  `dtype` (default: the tree's) is the compute dtype.  A tree or input the lowering does not cover runs its
    stock forward behind a RuntimeWarning."""

    what = "CompiledMVANet"

    def _lower(self, low: MVANetLowering, x: Tensor) -> Tensor:
        _expect(x.dim() == 4, f"input {tuple(x.shape)}")
        n_logits = kids(self.tree)[-1].out_channels if isa(kids(self.tree)[-1], "Conv2d") else 1
        out = torch.empty(1, n_logits, SIDE, SIDE, device=x.device, dtype=x.dtype)
        low.lower_net(self.tree, x, out)
        return out

    def _stock(self, x: Tensor) -> Tensor:
        return self.tree(x.to(self._tree_dtype()))


class CompiledMVANetBlock(_Compiled):
    """One MCLM or MCRM on token rows: `fast(tokens [5 S S, E]) -> tokens [5 S S, E]`, views stacked (four local, then the global one), i.e.
    `block(x)` for x [1, 5, E, S, S] with tokens = x[0].permute(0, 2, 3, 1).reshape(5 S S, E)."""

    what = "CompiledMVANetBlock"

    def _lower(self, low: MVANetLowering, x: Tensor) -> Tensor:
        _expect(isa(self.tree, "MCLM", "MCRM"), f"expected an MCLM or MCRM, got {cname(self.tree)}")
        out = torch.empty_like(x)
        low.lower_block(self.tree, x, out)
        return out

    def _stock(self, x: Tensor) -> Tensor:
        S = math.isqrt(x.shape[0] // 5)
        y = self.tree(x.to(self._tree_dtype()).view(1, 5, S, S, -1).permute(0, 1, 4, 2, 3))
        return y[0].permute(0, 2, 3, 1).reshape(x.shape[0], -1)


CompiledMCLM = CompiledMCRM = CompiledMVANetBlock
