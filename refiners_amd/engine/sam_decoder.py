"""MI355X lowering of the SegmentAnything mask decoder (segment_anything/mask_decoder.py, transformer.py, prompt_encoder.py, model.py).

P prompt sets of T = 5 + points tokens against ONE image embedding, token-major throughout: tokens [P*T, 256], the dense embedding
[P*4096, 256] (or [4096, 256] shared by every prompt until the first image -> token attention writes it, when no mask prompt is given).

  image embedding (NCHW)  -> nchw_to_nhwc; + no_mask_embedding (axpby with a constant table)     | MaskEncoder: patchify 4x4 + three
                                                                                                  GEMMs + two convt2x2_ln_gelu (below)
  TwoWayTransformerLayer  -> QKV GEMM (the sparse embedding as a second K segment) | sam_attention (8 x 32, Lk = T) | out GEMM (+ residual)
                             | LayerNorm | Q GEMM, K|V GEMM of the dense embedding (+ the positional embedding folded into a constant
                             residual table: (d + pe) W^T + b = d W^T + [pe W^T + b]) | sam_attention (8 x 16, Lk = 4096, key split)
                             | out GEMM + residual | LayerNorm | FF GEMM (ReLU epilogue) | GEMM + residual | LayerNorm
                             | Q GEMM of the dense side, K|V GEMM of the tokens | sam_attention (8 x 16, Lq = 4096, Lk = T) | out GEMM
                             + dense residual | LayerNorm -> the new dense embedding
  final token -> image attention + LayerNorm
  Hypernetworks / IOU MLPs -> 3 GEMMs each (ReLU epilogues) on the rows of their token
  DenseEmbeddingUpscaling -> GEMM [P*4096, 256] x [256, 4*64] (ConvTranspose2d 256 -> 64, 2x2/2) | convt2x2_ln_gelu (LayerNorm2d + GELU +
                             2x scatter to NHWC [P, 128, 128, 64]) | sam_mask_head (ConvTranspose2d 64 -> 32 + GELU + hypernetwork
                             contraction) -> low_res_masks [P, k, 256, 256]
  postprocess_masks       -> sam_postprocess_masks, outside the recorded program (the original size is per call)

MaskEncoder (a low_res_mask prompt): both 2x2/2 convolutions come from ONE 4x4 space-to-depth of the mask: patchify(P = 4) gives each
64 x 64 output pixel its 16 input pixels, the first convolution is a [16 -> 4 quadrants x 4 channels] GEMM, LayerNorm2d + GELU per
4-channel group (convt2x2_ln_gelu without scatter), the second a [16 -> 16] GEMM over those groups, then LayerNorm2d + GELU and the 1x1
convolution (GEMM, the image embedding as its residual).
"""
from __future__ import annotations

import warnings
from typing import Any, Optional, Sequence

import torch
from torch import Tensor

from .. import native
from ..fluxion.tree import tree_epoch
from .compiled import Program
from .lowering import Lowering
from .packing import PackCache, Unsupported, _expect, cname, isa, kids, launches
from .sam import CompiledSAMViT

#: class names of HQ-SAM's decoder adapters (segment_anything/hq_sam.py:16-412): refused here; engine/sam_hq.py lowers a tree that has them
HQ_NODES = ("HQSAMAdapter", "MaskDecoderTokensExtender", "MaskPredictionAdapter", "PredictionsPostProc", "HQSAMMaskPrediction")
NOT_A_POINT = 5  # PointType.NOT_A_POINT.value


def _attention_linears(att: Any) -> tuple[Any, Any, Any, Any, Any]:
    """fl.Attention (or SelfAttention) -> (wq, wk, wv, wo, sdpa)."""
    ch = kids(att)
    if isa(att, "SelfAttention"):
        _expect(isa(ch[0], "Parallel") and all(isa(c, "Identity") for c in kids(ch[0])), "unexpected SelfAttention layout")
        ch = ch[1:]
    _expect(len(ch) == 3 and isa(ch[0], "Distribute") and isa(ch[1], "ScaledDotProductAttention") and isa(ch[2], "Linear"), "unexpected Attention layout")
    q, k, v = kids(ch[0])
    _expect(not ch[1].is_causal and ch[1].num_heads == att.num_heads, "causal or mismatching attention")
    return q, k, v, ch[2], ch[1]


def _multilinear(ml: Any) -> list[Any]:
    ch = kids(ml)
    _expect(isa(ml, "MultiLinear") and len(ch) == 5 and isa(ch[1], "ReLU") and isa(ch[3], "ReLU"), "unexpected MultiLinear")
    return [ch[0], ch[2], ch[4]]


class SAMDecoderLowering(Lowering):
    """lower(sam, P, T, ...) records one program over static buffers: inputs `emb` [1, 256, 64, 64], `sparse` [P*T, 256], `mask_in`
    [P, 1, 256, 256] (has_mask); outputs `low` [P, k, 256, 256] and `iou` [P, 16] (columns iou_cols)."""

    def __init__(self, device: torch.device, dtype: torch.dtype, cache: Optional[PackCache] = None) -> None:
        super().__init__(device, dtype, cache, "merged")
        self.keep: list[Tensor] = []

    # -- helpers -----------------------------------------------------------------------------------------------
    def _zeros(self, rows: int, cols: int) -> Tensor:
        """A buffer whose columns beyond what its producer writes must stay zero (K padding of a GEMM operand): never pooled."""
        t = torch.zeros(rows, cols, device=self.device, dtype=self.dtype)
        self.keep.append(t)
        return t

    def _f32(self, t: Tensor) -> Tensor:
        return self.cache.get(("f32",) + PackCache.ident(t), lambda: t.detach().to(device=self.device, dtype=torch.float32).contiguous())

    def _cat_rows(self, tag: str, parts: Sequence[Optional[Tensor]], shapes: Sequence[tuple[int, ...]]) -> Tensor:
        """Rows of several weights (None = zeros of that shape) stacked in the compute dtype."""
        srcs = [p for p in parts if p is not None]

        def make() -> Tensor:
            out = [self.cvt(p) if p is not None else torch.zeros(*s, device=self.device, dtype=self.dtype) for p, s in zip(parts, shapes)]
            return torch.cat(out, dim=0).contiguous()

        return self.cache.get((tag, tuple(p is None for p in parts)) + PackCache.ident(*srcs), make)

    def _lin(self, x: Tensor, node: Any, out: Optional[Tensor] = None, res: Optional[Tensor] = None, relu: bool = False) -> Tensor:
        _expect(isa(node, "Linear") and node.in_features % self.kblk == 0, "unexpected Linear")
        if out is None:
            out = self.pool.get(x.shape[0], node.out_features)
        native.gemm([(x, self.kblocked(self._w(node.weight)))], out, bias=self._w(node.bias), res=res, relu=relu)
        return out

    def _rows(self, x: Tensor, P: int, T: int, t: int) -> Tensor:
        """The [P, C] rows of token t of every prompt (a strided view)."""
        return x.as_strided((P, x.shape[1]), (T * x.stride(0), 1), x.storage_offset() + t * x.stride(0))

    def _pe_table(self, tag: str, pe: Tensor, lins: Sequence[tuple[Any, bool]], reps: int) -> Tensor:
        """[reps * 4096, sum N] constant residual: per Linear (node, with_pe) the columns pe W^T + b, or just b."""
        srcs = [t for (n, _w) in lins for t in (n.weight, n.bias) if t is not None]

        def make() -> Tensor:
            cols = []
            for node, with_pe in lins:
                b = node.bias.detach().to(self.device, torch.float32) if node.bias is not None else torch.zeros(node.out_features, device=self.device)
                if with_pe:
                    cols.append(self._mm(pe, node.weight.detach().to(self.device, torch.float32)) + b)
                else:
                    cols.append(b.expand(pe.shape[0], -1))
            return torch.cat(cols, dim=1).to(self.dtype).repeat(reps, 1).contiguous()

        return self.cache.get((tag, reps) + PackCache.ident(pe, *srcs), make)

    def _attn(self, q: Tensor, k: Tensor, v: Tensor, P: int, Lq: int, Lk: int, heads: int, q_shared: bool = False, kv_shared: bool = False) -> Tensor:
        """q [Pq*Lq, >=], k / v column views [Pk*Lk, >=] -> out [P*Lq, inner]."""
        inner = q.shape[1]
        out = self.pool.get(P * Lq, inner)
        v3 = lambda t, L, shared: t.as_strided((1 if shared else P, L, t.shape[1]), (0 if shared else L * t.stride(0), t.stride(0), 1))  # noqa: E731
        need = native.sam_attention_ws_floats(P, heads, inner // heads, Lq, Lk)
        ws = None
        if need:
            store = self.__dict__.setdefault("_attn_ws", {})
            ws = store.get(need)
            if ws is None:
                ws = store[need] = torch.empty(need, device=self.device, dtype=torch.float32)
        native.sam_attention(v3(q, Lq, q_shared), v3(k, Lk, kv_shared), v3(v, Lk, kv_shared), out.view(P, Lq, inner), heads, ws=ws)
        self.stats.setdefault("attention_kinds", []).append(f"h{heads}xd{inner // heads} Lq={Lq} Lk={Lk}")
        return out

    # -- the tree ----------------------------------------------------------------------------------------------
    def check(self, sam: Any) -> tuple[Any, Any, Any, Any]:
        for m in sam.modules():
            _expect(cname(m) not in HQ_NODES, f"{cname(m)}: HQ-SAM's mask decoder branch is not lowered")
        ch = kids(sam)
        _expect(isa(sam, "SegmentAnything") and len(ch) == 4, "unexpected SegmentAnything layout")
        _expect(isa(ch[1], "PointEncoder") and isa(ch[2], "MaskEncoder") and isa(ch[3], "MaskDecoder"), "unexpected SegmentAnything children")
        dec = kids(ch[3])
        _expect(len(dec) == 4 and [cname(c) for c in dec] == ["MaskDecoderTokens", "EmbeddingsAggregator", "Transformer", "Predictions"], "unexpected MaskDecoder layout")
        _expect(tuple(getattr(ch[0], "image_embedding_size", ())) == (64, 64) and getattr(ch[3], "embedding_dim", None) == 256,
                "only the 64 x 64 x 256 SAM image embedding is lowered")
        return ch[0], ch[1], ch[2], ch[3]

    def lower(self, sam: Any, P: int, T: int, has_mask: bool, pe: Tensor) -> dict[str, Tensor]:
        """pe: the dense positional embedding as float32 tokens [4096, 256]."""
        _enc, _pt, menc, dec = self.check(sam)
        C = dec.embedding_dim
        _expect(C == 256 and pe.shape == (4096, C), "only the 64 x 64 x 256 SAM embedding is lowered")
        _expect(T <= 64, f"{T} prompt tokens: mi355x_sam_attention takes at most 64 keys per token self-attention")
        transformer, mp, ip = self.decoder_parts(dec)
        multimask = bool(mp.multimask_output)
        k_out = 3 if multimask else 1
        first = 1 if multimask else 0
        io = self.make_io(P, T, has_mask, k_out, C)
        self.iou_cols = (1, 4) if multimask else (0, 1)
        L = 4096
        with self.in_step():
            img = self.img = self.pool.get(L, C)  # (never returned to the pool: a subclass reads the token-major image embedding again)
            native.nchw_to_nhwc(io["emb"], img)
            if has_mask:
                dense = self.mask_encoder(menc, io["mask_in"], img, P)
                shared = False
            else:
                nm = menc.no_mask_embedding
                table = self.cache.get(("no_mask", L) + PackCache.ident(nm), lambda: self.cvt(nm.detach().reshape(1, C)).expand(L, C).contiguous())
                dense = self.pool.get(L, C)
                native.axpby(img, 1.0, table, 1.0, dense)
                shared = True
            x = io["sparse"]
            layers = kids(transformer)
            _expect(len(layers) >= 3 and isa(layers[-2], "SparseCrossDenseAttention") and isa(layers[-1], "LayerNorm"), "unexpected Transformer layout")
            for li, layer in enumerate(layers[:-2]):
                _expect(isa(layer, "TwoWayTransformerLayer"), f"unexpected {cname(layer)} in the Transformer")
                x, dense, shared = self.two_way_layer(layer, x, io["sparse"], dense, shared, pe, P, T)
            x = self.token_to_image(layers[-2], x, io["sparse"], dense, shared, pe, P, T)
            x = self._ln(x, layers[-1])
            if shared:  # (no transformer layer: not a SAM configuration, kept exact anyway)
                dense = self._expand(dense, P)
            self.predictions(mp, ip, x, dense, P, T, first, k_out, io)
        return io

    def decoder_parts(self, dec: Any) -> tuple[Any, Any, Any]:
        """(Transformer, MaskPrediction, IOUPrediction) of a MaskDecoder that check() accepted."""
        _tokens, _agg, transformer, predictions = kids(dec)
        mp, ip = kids(predictions)
        return transformer, mp, ip

    def make_io(self, P: int, T: int, has_mask: bool, k_out: int, C: int) -> dict[str, Any]:
        """The static input and output buffers of one program."""
        return dict(
            emb=torch.empty(1, C, 64, 64, device=self.device, dtype=self.dtype),
            sparse=torch.empty(P * T, C, device=self.device, dtype=self.dtype),
            mask_in=torch.empty(P, 1, 256, 256, device=self.device, dtype=self.dtype) if has_mask else None,
            low=torch.empty(P, k_out, 256, 256, device=self.device, dtype=self.dtype),
            iou=torch.empty(P, 16, device=self.device, dtype=self.dtype),
        )

    def mask_head(self, up1: Tensor, P: int, wct2: Tensor, bias: Tensor, hyper: Tensor, io: dict[str, Any]) -> None:
        """ConvTranspose2d(64 -> 32) + GELU + hypernetwork contraction of the upscaled embedding [P, 128, 128, 64] -> io["low"]."""
        native.sam_mask_head(up1, P, 128, 128, wct2, bias, hyper, io["low"])

    def _ln(self, x: Tensor, node: Any) -> Tensor:
        return self.layernorm(x, node)

    def _expand(self, dense: Tensor, P: int) -> Tensor:
        """The shared [4096, C] dense embedding copied per prompt (the first launch that writes per-prompt values reads it)."""
        idx = self.cache.get(("rows_mod", P, dense.shape[0]), lambda: (torch.arange(P * dense.shape[0], device=self.device) % dense.shape[0]).to(torch.int32))
        out = self.pool.get(P * dense.shape[0], dense.shape[1])
        native.gather_rows(dense, idx, out)
        return out

    def two_way_layer(self, layer: Any, x: Tensor, sparse: Tensor, dense: Tensor, shared: bool, pe: Tensor, P: int, T: int) -> tuple[Tensor, Tensor, bool]:
        ch = kids(layer)
        _expect(len(ch) == 7 and isa(ch[1], "LayerNorm") and isa(ch[2], "SparseCrossDenseAttention") and isa(ch[3], "LayerNorm")
                and isa(ch[4], "FeedForward") and isa(ch[5], "LayerNorm") and isa(ch[6], "Passthrough"), "unexpected TwoWayTransformerLayer layout")
        # self-attention of the tokens: SelfAttention (first layer, no residual, no positional term) or SparseSelfAttention
        sa = ch[0]
        if isa(sa, "SparseSelfAttention"):
            par, att = kids(sa)
            _expect(isa(par, "Parallel") and len(kids(par)) == 3 and isa(kids(par)[2], "Identity"), "unexpected SparseSelfAttention layout")
            residual, with_pe = True, True
        else:
            _expect(isa(sa, "SelfAttention"), f"unexpected {cname(sa)} as the self-attention")
            att, residual, with_pe = sa, False, False
        wq, wk, wv, wo, _ = _attention_linears(att)
        heads = att.num_heads
        inner = wq.out_features
        wqkv = self._cat_rows("sam_qkv", [wq.weight, wk.weight, wv.weight], [(inner, 256)] * 3)
        bqkv = self._cat_rows("sam_qkv_b", [wq.bias, wk.bias, wv.bias], [(inner,)] * 3)
        segs = [(x, self.kblocked(wqkv))]
        if with_pe:
            segs.append((sparse, self.kblocked(self._cat_rows("sam_qk0", [wq.weight, wk.weight, None], [(inner, 256)] * 3))))
        qkv = self.pool.get(P * T, 3 * inner)
        native.gemm(segs, qkv, bias=bqkv)
        a = self._attn(qkv[:, :inner], qkv[:, inner : 2 * inner], qkv[:, 2 * inner :], P, T, T, heads)
        self.pool.put(qkv)
        if residual:
            _expect(x is not sparse, "a residual self-attention on the raw prompt tokens")
            self._lin(a, wo, out=x, res=x)
        else:
            x = self._lin(a, wo)
        self.pool.put(a)
        x0, x = x, self._ln(x, ch[1])
        self.pool.put(x0)
        x = self.token_to_image(ch[2], x, sparse, dense, shared, pe, P, T)
        x = self._ln(x, ch[3])
        ff = kids(ch[4])
        _expect(len(ff) == 3 and isa(ff[1], "ReLU"), "unexpected FeedForward layout")
        h = self._lin(x, ff[0], relu=True)
        self._lin(h, ff[2], out=x, res=x)
        self.pool.put(h)
        x = self._ln(x, ch[5])
        # image -> token attention; the dense embedding becomes per prompt here
        pas = kids(ch[6])
        _expect(len(pas) == 3 and isa(pas[0], "Sum") and isa(pas[1], "LayerNorm") and isa(pas[2], "SetContext"), "unexpected Passthrough layout")
        s0, dcs = kids(pas[0])
        _expect(isa(s0, "UseContext") and isa(dcs, "DenseCrossSparseAttention"), "unexpected dense update")
        par, att = kids(dcs)
        wq, wk, wv, wo, _ = _attention_linears(att)
        inner = wq.out_features
        L = pe.shape[0]
        qd = self.pool.get(dense.shape[0], inner)
        native.gemm([(dense, self.kblocked(self._w(wq.weight)))], qd, res=self._pe_table("sam_pe_q", pe, [(wq, True)], 1 if shared else P))
        kv = self.pool.get(P * T, 2 * inner)
        wkv = self._cat_rows("sam_kv", [wk.weight, wv.weight], [(inner, 256)] * 2)
        wk0 = self._cat_rows("sam_k0", [wk.weight, None], [(inner, 256)] * 2)
        native.gemm([(x, self.kblocked(wkv)), (sparse, self.kblocked(wk0))], kv, bias=self._cat_rows("sam_kv_b", [wk.bias, wv.bias], [(inner,)] * 2))
        a = self._attn(qd, kv[:, :inner], kv[:, inner:], P, L, T, att.num_heads, q_shared=shared)
        self.pool.put(qd)
        self.pool.put(kv)
        if shared:
            dense = self._expand(dense, P)
            shared = False
        self._lin(a, wo, out=dense, res=dense)
        self.pool.put(a)
        dense_new = self._ln(dense, pas[1])
        self.pool.put(dense)
        return x, dense_new, shared

    def token_to_image(self, node: Any, x: Tensor, sparse: Tensor, dense: Tensor, shared: bool, pe: Tensor, P: int, T: int) -> Tensor:
        """SparseCrossDenseAttention: x + Attention(x + sparse, dense + pe, dense)."""
        par, att = kids(node)
        _expect(isa(par, "Parallel") and len(kids(par)) == 3 and isa(kids(par)[1], "Sum"), "unexpected SparseCrossDenseAttention layout")
        wq, wk, wv, wo, _ = _attention_linears(att)
        inner = wq.out_features
        L = pe.shape[0]
        q = self.pool.get(P * T, inner)
        w = self.kblocked(self._w(wq.weight))
        native.gemm([(x, w), (sparse, w)], q, bias=self._w(wq.bias))
        kv = self.pool.get(dense.shape[0], 2 * inner)
        wkv = self._cat_rows("sam_kv", [wk.weight, wv.weight], [(inner, 256)] * 2)
        native.gemm([(dense, self.kblocked(wkv))], kv, res=self._pe_table("sam_pe_kv", pe, [(wk, True), (wv, False)], 1 if shared else P))
        a = self._attn(q, kv[:, :inner], kv[:, inner:], P, T, L, att.num_heads, kv_shared=shared)
        self.pool.put(q)
        self.pool.put(kv)
        out = x if x is not sparse else self.pool.get(P * T, x.shape[1])
        self._lin(a, wo, out=out, res=x)
        self.pool.put(a)
        return out

    # -- prompt-side mask encoder --------------------------------------------------------------------------------
    def mask_encoder(self, menc: Any, mask_in: Tensor, img: Tensor, P: int) -> Tensor:
        ch = kids(menc)
        _expect([cname(c) for c in ch] == ["Conv2d", "LayerNorm2d", "GeLU", "Conv2d", "LayerNorm2d", "GeLU", "Conv2d"], "unexpected MaskEncoder layout")
        c1, n1, _g1, c2, n2, _g2, c3 = ch
        _expect(c1.in_channels == 1 and c1.kernel_size == (2, 2) and tuple(c1.stride) == (2, 2) and c2.kernel_size == (2, 2) and tuple(c2.stride) == (2, 2)
                and c3.kernel_size == (1, 1) and tuple(mask_in.shape[2:]) == (256, 256), "unexpected MaskEncoder convolutions")
        ci, cm = c1.out_channels, c2.out_channels
        _expect(4 * ci <= 64 and cm <= 64 and 64 % ci == 0 and 64 % cm == 0, "unexpected MaskEncoder widths")
        M = P * 4096
        kp = self.kblk

        def w1() -> Tensor:  # [4 quadrants x ci, 16 -> kp]: row (q, c), column ky * 4 + kx of the 4x4 patch
            w = torch.zeros(4, ci, 4, 4, device=self.device, dtype=torch.float32)
            src = c1.weight.detach().to(self.device, torch.float32)[:, 0]  # [ci, 2, 2]
            for q in range(4):
                dy, dx = divmod(q, 2)
                w[q, :, 2 * dy : 2 * dy + 2, 2 * dx : 2 * dx + 2] = src
            out = torch.zeros(4 * ci, kp, device=self.device, dtype=torch.float32)
            out[:, :16] = w.reshape(4 * ci, 16)
            return out.to(self.dtype).contiguous()

        def w2() -> Tensor:  # [cm, (q, c) -> kp]
            src = c2.weight.detach().to(self.device, torch.float32)  # [cm, ci, 2, 2]
            out = torch.zeros(cm, kp, device=self.device, dtype=torch.float32)
            out[:, : 4 * ci] = src.permute(0, 2, 3, 1).reshape(cm, 4 * ci)
            return out.to(self.dtype).contiguous()

        def w3() -> Tensor:
            out = torch.zeros(c3.out_channels, kp, device=self.device, dtype=torch.float32)
            out[:, :cm] = c3.weight.detach().to(self.device, torch.float32).reshape(c3.out_channels, cm)
            return out.to(self.dtype).contiguous()

        ident = PackCache.ident(c1.weight, c2.weight, c3.weight)
        W1, W2, W3 = (self.cache.get((tag, kp) + ident, f) for tag, f in (("sam_me_w1", w1), ("sam_me_w2", w2), ("sam_me_w3", w3)))
        b1 = self.cache.get(("sam_me_b1",) + PackCache.ident(c1.bias), lambda: self.cvt(c1.bias.detach()).repeat(4).contiguous())
        cols = self._zeros(M, kp)
        native.patchify_nchw(mask_in, 4, cols)
        y1 = self.pool.get(M, 4 * ci)
        native.gemm([(cols, W1)], y1, bias=b1)
        z1 = self._zeros(M, kp)
        native.convt2x2_ln_gelu(y1, ci, 4, self._f32(n1.weight), self._f32(n1.bias), float(n1.eps), z1)
        y2 = self.pool.get(M, cm)
        native.gemm([(z1, W2)], y2, bias=self._w(c2.bias))
        z2 = self._zeros(M, kp)
        native.convt2x2_ln_gelu(y2, cm, 1, self._f32(n2.weight), self._f32(n2.bias), float(n2.eps), z2)
        dense = self._expand(img, P)
        native.gemm([(z2, W3)], dense, bias=self._w(c3.bias), res=dense)
        return dense

    # -- predictions ----------------------------------------------------------------------------------------------
    def predictions(self, mp: Any, ip: Any, x: Tensor, dense: Tensor, P: int, T: int, first: int, k_out: int, io: dict[str, Tensor]) -> None:
        mch = kids(mp)
        _expect(len(mch) == 4 and isa(mch[1], "Matmul"), "unexpected MaskPrediction layout")
        hyper_node, up = kids(mch[1])
        _expect(isa(hyper_node, "Hypernetworks") and isa(up, "DenseEmbeddingUpscaling"), "unexpected MaskPrediction operands")
        hyper = self.pool.get(P, 4 * 32)
        for j in range(k_out):
            t = first + j  # mask token t (token 1 + t of the sequence)
            chain = kids(hyper_node)[t]
            mls = _multilinear(kids(chain)[1])
            _expect(mls[2].out_features == 32, "unexpected hypernetwork width")
            h = self._lin(self._rows(x, P, T, 1 + t), mls[0], relu=True)
            h2 = self._lin(h, mls[1], relu=True)
            self._lin(h2, mls[2], out=hyper[:, 32 * j : 32 * j + 32])
            self.pool.put(h)
            self.pool.put(h2)
        uch = kids(up)
        _expect([cname(c) for c in uch][3:] == ["ConvTranspose2d", "LayerNorm2d", "GeLU", "ConvTranspose2d", "GeLU", "Flatten", "SetContext"], "unexpected DenseEmbeddingUpscaling layout")
        ct1, ln, _g, ct2 = uch[3], uch[4], uch[5], uch[6]
        _expect(ct1.kernel_size == (2, 2) and tuple(ct1.stride) == (2, 2) and ct1.out_channels == 64 and ct2.in_channels == 64 and ct2.out_channels == 32
                and ct2.kernel_size == (2, 2) and tuple(ct2.stride) == (2, 2) and ct1.bias is not None and ct2.bias is not None, "unexpected transposed convolutions")
        # ConvTranspose2d(256 -> 64, 2, 2) as ONE GEMM: column q * 64 + c = output channel c of quadrant q = (dy, dx)
        wct1 = self.cache.get(("sam_ct1",) + PackCache.ident(ct1.weight), lambda: self.cvt(ct1.weight.detach().permute(2, 3, 1, 0).reshape(4 * 64, ct1.in_channels)))
        bct1 = self.cache.get(("sam_ct1_b",) + PackCache.ident(ct1.bias), lambda: self.cvt(ct1.bias.detach()).repeat(4).contiguous())
        y = self.pool.get(dense.shape[0], 256)
        native.gemm([(dense, self.kblocked(wct1))], y, bias=bct1)
        up1 = self.pool.get(4 * dense.shape[0], 64)
        native.convt2x2_ln_gelu(y, 64, 4, self._f32(ln.weight), self._f32(ln.bias), float(ln.eps), up1, scatter_hw=(64, 64))
        self.pool.put(y)
        wct2 = self.cache.get(("sam_ct2",) + PackCache.ident(ct2.weight), lambda: ct2.weight.detach().to(self.device, torch.float32).permute(0, 2, 3, 1).reshape(64, 128).contiguous())
        self.mask_head(up1, P, wct2, self._f32(ct2.bias), hyper.view(P, 4, 32)[:, :k_out], io)
        # IoU head on token 0 (output padded to 16 columns)
        ich = kids(ip)
        _expect(len(ich) == 4 and isa(ich[2], "MultiLinear"), "unexpected IOUPrediction layout")
        l1, l2, l3 = _multilinear(ich[2])
        _expect(l3.out_features <= 16, "unexpected IoU head width")
        w3 = self.cache.get(("sam_iou_w",) + PackCache.ident(l3.weight), lambda: torch.cat([self.cvt(l3.weight), torch.zeros(16 - l3.out_features, l3.in_features, device=self.device, dtype=self.dtype)]).contiguous())
        b3 = self.cache.get(("sam_iou_b",) + PackCache.ident(l3.bias), lambda: torch.cat([self.cvt(l3.bias), torch.zeros(16 - l3.out_features, device=self.device, dtype=self.dtype)]).contiguous())
        h = self._lin(self._rows(x, P, T, 0), l1, relu=True)
        h2 = self._lin(h, l2, relu=True)
        native.gemm([(h2, w3)], io["iou"], bias=b3)


class CompiledSegmentAnything:
    """`fast = CompiledSegmentAnything(sam)`: `fast.predict(...)` == `sam.predict(...)` (same signature, shapes and dtypes) on the MI355X
    kernels, and `fast.predict_batch(...)` for many prompt sets against one image embedding.  An unrecognised tree (HQ-SAM's decoder
    adapters, ...) runs the stock forward with a RuntimeWarning and stats["whole_fallback"] set."""

    lowering_cls = SAMDecoderLowering

    def __init__(self, sam: Any, use_graph: bool = True) -> None:
        native.load()
        self.sam = sam
        self.use_graph = use_graph
        self.cache = PackCache()
        self.programs: dict[tuple, tuple[SAMDecoderLowering, dict[str, Tensor], Program]] = {}
        self.bad_keys: dict[tuple, str] = {}  # program keys whose lowering raised Unsupported (per tree epoch: any tree change retries)
        self.stats: dict[str, Any] = {}
        self._vit: Optional[CompiledSAMViT] = None
        self._pe: Optional[tuple] = None

    # -- plumbing ----------------------------------------------------------------------------------------------
    @property
    def dtype(self) -> torch.dtype:
        return self.sam.mask_decoder.dtype

    @property
    def device(self) -> torch.device:
        return self.sam.mask_decoder.device

    def _fallback_reason(self) -> Optional[str]:
        try:
            self.lowering_cls(torch.device("meta"), self.dtype).check(self.sam)
        except Unsupported as exc:
            return str(exc)
        return None

    def _dense_pe(self) -> Tensor:
        key = (tree_epoch(), self.dtype, self.device)
        if self._pe is None or self._pe[0] != key:
            with torch.no_grad():
                pe = self.sam.point_encoder.get_dense_positional_embedding(image_embedding_size=(64, 64))
            self._pe = (key, pe.reshape(pe.shape[1], -1).t().to(torch.float32).contiguous())
        return self._pe[1]

    def _program(self, P: int, T: int, has_mask: bool) -> tuple[SAMDecoderLowering, dict[str, Tensor], Program]:
        """The program of one geometry, lowered on first use; raises Unsupported (remembered per key) for a tree it does not know."""
        multimask = bool(self.sam.mask_decoder.multimask_output)
        key = (tree_epoch(), P, T, multimask, has_mask, self.dtype, self.device)
        got = self.programs.get(key)
        if got is None:
            if key in self.bad_keys:
                raise Unsupported(self.bad_keys[key])
            new_epoch = any(k[0] != key[0] for k in list(self.programs) + list(self.bad_keys))
            if new_epoch:  # the tree changed: earlier programs and their packed weights go
                self.programs.clear()
                self.bad_keys.clear()
                self.cache.sweep()
            try:
                low = self.lowering_cls(self.device, self.dtype, self.cache)
                io = low.lower(self.sam, P, T, has_mask, self._dense_pe())
            except Unsupported as exc:
                self.bad_keys[key] = str(exc)
                raise
            if new_epoch:
                self.cache.sweep()  # keep only what the new tree's first program packed
            got = (low, io, Program(low.step, self.use_graph, low=low))
            self.programs[key] = got
        low = got[0]  # the stats of the program that runs now, also after a whole fallback of another geometry
        self.stats = dict(low.stats, step_ops=launches(low.step), pool_bytes=low.step_pool.bytes(), whole_fallback=None)
        return got

    def compute_image_embedding(self, image: Any) -> Any:
        """The image encoder on CompiledSAMViT (the reference's compute_image_embedding)."""
        if self._vit is None:
            self._vit = CompiledSAMViT(self.sam.image_encoder, use_graph=self.use_graph)
        features = self._vit(self.sam.preprocess_image(image))
        return _embedding(self.sam)(features=features, original_image_size=(image.height, image.width))

    def _tokens(self) -> Tensor:
        """The decoder's own tokens [n, 256], the head of every prompt's token sequence."""
        return kids(kids(self.sam.mask_decoder)[0])[1].weight

    def _sparse(self, coords: Tensor, types: Tensor, original_size: tuple[int, int]) -> Tensor:
        """[tokens | point embedding] of ONE prompt set (see _sparse_batch)."""
        return self._sparse_batch([(coords.reshape(-1, 2), types.reshape(-1))], original_size)[0]

    def _sparse_batch(self, sets: Sequence[tuple[Tensor, Tensor]], original_size: tuple[int, int]) -> list[Tensor]:
        """[tokens | point embedding] of each prompt set: the PointEncoder's arithmetic (prompt_encoder.py:13-160) in float32 torch on its
        weights, a few rows per prompt, batched over the prompt sets of the same point count and box / no-box padding; float32 whatever the
        model's dtype (the tree's own PointTypeEmbedding writes float32 rows, which a bfloat16 model cannot index_put)."""
        pt = self.sam.point_encoder
        ce = next(m for m in pt.modules() if isa(m, "CoordinateEncoder"))
        m1, lin, m2, cat = kids(ce)
        _expect(isa(m1, "Multiply") and isa(lin, "Linear") and isa(m2, "Multiply") and isa(cat, "Concatenate"), "unexpected CoordinateEncoder layout")
        te = next(m for m in pt.modules() if isa(m, "PointTypeEmbedding"))
        f = dict(device=self.device, dtype=torch.float32)
        tok = self._tokens().to(self.dtype)
        groups: dict[tuple[int, bool], list[int]] = {}
        for i, (_c, t) in enumerate(sets):
            groups.setdefault((int(t.numel()), bool(((t == 3) | (t == 4)).any())), []).append(i)
        out: list[Optional[Tensor]] = [None] * len(sets)
        for (n, has_box), idx in groups.items():
            G = len(idx)
            x = self.sam.normalize(torch.stack([sets[i][0].reshape(n, 2) for i in idx]).to(**f), original_size=original_size)
            t = torch.stack([sets[i][1].reshape(n) for i in idx]).to(device=self.device, dtype=torch.int64)
            x = m1.scale * x + m1.bias
            x = torch.nn.functional.linear(x, lin.weight.to(**f))
            x = m2.scale * x + m2.bias
            x = torch.cat([torch.sin(x), torch.cos(x)], dim=-1)
            if not has_box:  # one NOT_A_POINT token per prompt set (PointEncoder.pad)
                x = torch.cat([x, torch.zeros(G, 1, x.shape[-1], **f)], dim=1)
                t = torch.cat([t, torch.full((G, 1), NOT_A_POINT, device=self.device, dtype=torch.int64)], dim=1)
            x = (x + te.weight.to(**f)[t - 1]).to(self.dtype)
            rows = torch.cat([tok.unsqueeze(0).expand(G, -1, -1), x], dim=1)
            for j, i in enumerate(idx):
                out[i] = rows[j]
        return out  # type: ignore[return-value]

    def _run(self, emb: Tensor, sparse: list[Tensor], masks: Optional[Tensor]) -> tuple[Tensor, Tensor]:
        P, T = len(sparse), sparse[0].shape[0]
        low, io, prog = self._program(P, T, masks is not None)
        _expect(emb.numel() == io["emb"].numel(), f"image embedding of shape {tuple(emb.shape)}: the program takes one [1, 256, 64, 64] embedding")
        io["emb"].copy_(emb.reshape(io["emb"].shape))
        io["sparse"].copy_(torch.cat(sparse, dim=0))
        if masks is not None:
            io["mask_in"].copy_(masks.reshape(io["mask_in"].shape))
        self._fill_inputs(io)
        prog.run()
        a, b = low.iou_cols
        return self._low_res(io), io["iou"][:, a:b].clone()

    def _fill_inputs(self, io: dict[str, Any]) -> None:
        """Further program inputs of a subclass, read at call time."""

    def _low_res(self, io: dict[str, Any]) -> Tensor:
        """The program's low-resolution masks as a tensor of the caller's."""
        return io["low"].clone()

    def _postprocess(self, low: Tensor, original_size: tuple[int, int], binarize: bool) -> Tensor:
        R = self.sam.image_encoder_resolution
        scaled = _scaled_size(original_size, R)
        out = torch.empty(*low.shape[:2], *original_size, device=low.device, dtype=torch.bool if binarize else low.dtype)
        native.sam_postprocess_masks(low, R, scaled, out, threshold=float(self.sam.mask_threshold) if binarize else None)
        return out

    # -- public ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, input: Any, foreground_points: Optional[Sequence[tuple[float, float]]] = None, background_points: Optional[Sequence[tuple[float, float]]] = None,
                box_points: Optional[Sequence[Sequence[tuple[float, float]]]] = None, low_res_mask: Optional[Tensor] = None, binarize: bool = True) -> tuple[Tensor, Tensor, Tensor]:
        """SegmentAnything.predict (segment_anything/model.py:105-168): ONE prompt set -> (masks, iou_predictions, low_res_masks)."""
        stock = dict(foreground_points=foreground_points, background_points=background_points, box_points=box_points, low_res_mask=low_res_mask, binarize=binarize)
        reason = self._fallback_reason()
        if reason is not None:
            self._whole_fallback(reason)
            return self.sam.predict(input, **stock)
        if not hasattr(input, "features"):
            input = self.compute_image_embedding(input)
        try:
            coords, types = self.sam.point_encoder.points_to_tensor(foreground_points=foreground_points, background_points=background_points, box_points=box_points)
            sparse = self._sparse(coords, types, input.original_image_size)
            low, iou = self._run(input.features, [sparse], low_res_mask)
        except Unsupported as exc:  # a node deeper in the tree than check() looks: the same convention
            self._whole_fallback(str(exc))
            return self.sam.predict(input, **stock)
        return self._postprocess(low, input.original_image_size, binarize), iou, low

    @torch.no_grad()
    def predict_batch(self, embedding: Any, points: Any, point_types: Any, low_res_masks: Optional[Tensor] = None,
                      original_size: Optional[tuple[int, int]] = None, binarize: bool = True) -> tuple[Tensor, Tensor, Tensor]:
        """P prompt sets against one image embedding ([1, 256, 64, 64] tensor or ImageEmbedding): points [P, N, 2] (pixel coordinates of the
        original image) and point_types [P, N] (PointType values; entries <= 0 are padding, not points) -- or lists of per-prompt [N_p, 2] /
        [N_p] tensors; low_res_masks [P, 1, 256, 256] or None.  Returns ([P, k, H, W], [P, k], [P, k, 256, 256]); prompt p's rows equal
        predict() on that prompt alone.  Prompts are grouped by token count, one program (one graph replay) per group."""
        if hasattr(embedding, "features"):
            original_size = original_size or embedding.original_image_size
            embedding = embedding.features
        assert original_size is not None, "original_size is needed with a bare embedding tensor"
        P = len(points)
        sets = []
        for p in range(P):
            c, t = torch.as_tensor(points[p], dtype=torch.float32), torch.as_tensor(point_types[p]).to(torch.int32)
            keep = t > 0
            sets.append((c[keep].reshape(-1, 2), t[keep]))
        reason = self._fallback_reason()
        if reason is not None:
            self._whole_fallback(reason)
            return self._stock_batch(embedding, sets, low_res_masks, original_size, binarize)
        try:
            sparse = self._sparse_batch(sets, original_size)
            groups: dict[int, list[int]] = {}
            for p, s in enumerate(sparse):
                groups.setdefault(s.shape[0], []).append(p)
            for T, idx in groups.items():  # every group's program before any of them runs: a refusal falls back for the whole batch
                self._program(len(idx), T, low_res_masks is not None)
            k = 3 if self.sam.mask_decoder.multimask_output else 1
            low = torch.empty(P, k, 256, 256, device=self.device, dtype=self.dtype)
            iou = torch.empty(P, k, device=self.device, dtype=self.dtype)
            for _T, idx in groups.items():
                m = low_res_masks[idx] if low_res_masks is not None else None
                lg, ig = self._run(embedding, [sparse[p] for p in idx], m)
                ii = torch.tensor(idx, device=self.device)
                low[ii], iou[ii] = lg, ig
        except Unsupported as exc:
            self._whole_fallback(str(exc))
            return self._stock_batch(embedding, sets, low_res_masks, original_size, binarize)
        return self._postprocess(low, original_size, binarize), iou, low

    def _whole_fallback(self, reason: str) -> None:
        warnings.warn(f"CompiledSegmentAnything: {reason}; running the unfused SegmentAnything forward", RuntimeWarning, stacklevel=3)
        self.stats = {"whole_fallback": reason, "fallback_nodes": ["<whole mask decoder>"], "step_ops": 0}

    def _stock_batch(self, embedding: Tensor, sets: list, low_res_masks: Optional[Tensor], original_size: tuple[int, int], binarize: bool) -> tuple[Tensor, Tensor, Tensor]:
        outs = []
        names = {1: "background_points", 2: "foreground_points"}
        for p, (c, t) in enumerate(sets):
            kw: dict[str, Any] = {v: [tuple(xy) for xy, tt in zip(c.tolist(), t.tolist()) if tt == k] or None for k, v in names.items()}
            tl = [tuple(xy) for xy, tt in zip(c.tolist(), t.tolist()) if tt == 3]
            br = [tuple(xy) for xy, tt in zip(c.tolist(), t.tolist()) if tt == 4]
            kw["box_points"] = [[a, b] for a, b in zip(tl, br)] or None
            m = low_res_masks[p : p + 1] if low_res_masks is not None else None
            outs.append(self.sam.predict(_embedding(self.sam)(features=embedding, original_image_size=original_size), low_res_mask=m, binarize=binarize, **kw))
        return tuple(torch.cat([o[i] for o in outs]) for i in range(3))  # type: ignore[return-value]


def _scaled_size(size: tuple[int, int], R: int) -> tuple[int, int]:
    """segment_anything/utils.py:7-24 (compute_scaled_size)."""
    scale = R * 1.0 / max(size)
    return (int(size[0] * scale + 0.5), int(size[1] * scale + 0.5))


def _embedding(sam: Any) -> Any:
    """The ImageEmbedding dataclass of the model's own package (the mirror's or refiners')."""
    import sys

    mod = sys.modules[type(sam).__module__]
    emb = getattr(mod, "ImageEmbedding", None)
    if emb is None:
        from ..segment_anything import ImageEmbedding as emb  # noqa: N813
    return emb
