"""MI355X lowering of HQ-SAM mask prediction (segment_anything/hq_sam.py): SAMDecoderLowering plus the HQ branch, for a SegmentAnything
with HQSAMAdapter injected.  On a tree without the adapter both classes here are their base classes.

The adapted decoder has [5 regular tokens ; hq_token] (T = 6 + points), and next to the base mask one HQ mask per prompt,
h . (EmbeddingMaskfeature(u) + F):

  shared per image   F = EmbeddingEncoder(image embedding) + CompressViTFeat(early ViT embedding):
                     GEMM [4096, 256] x [256, 4*64] | convt2x2_ln_gelu (scatter) -> A [16384, 64]
                     GEMM [4096, 1280] x [1280, 4*256] | ln2d_gelu_wide (scatter) -> B [16384, 256]
                     ONE two-segment GEMM [(A, Wa), (B, Wb)] -> Fq [16384, 4*32]: both second transposed convolutions are linear and land on
                     the same grid; Fq stays in quadrant layout (pixel (y, x) = row (y >> 1) * 128 + (x >> 1), columns ((y & 1) * 2 + (x & 1))
                     * 32 + c), the head kernel indexes it
  per prompt         h = HQTokenMLP(token 5): three GEMMs (ReLU epilogues) -> [P, 32]
                     sam_mask_head_up: the base mask AND u = the upscaled dense embedding as NHWC rows [P*65536, 32] (bf16: 64-wide rows whose
                     columns 32.. stay zero, the implicit-GEMM convolution's K block)
                     conv_gemm 3x3 32 -> 64 (+ bias) -> y [P*65536, 64]
                     sam_hq_mask_head: LayerNorm2d + GELU on the way into LDS, the second 3x3 convolution folded with h into a 64 -> 1
                     convolution, + h . (F + b2) -> io["hq"] [P, 1, 256, 256]

PredictionsPostProc.hq_mask_only is a live attribute: the program always writes both planes, and `hq` or `hq + base` is chosen per call
outside the recorded program.  The early ViT embedding is a program input like the image embedding, read from context "hq_sam" at call time.
"""
from __future__ import annotations

from typing import Any, Optional

import torch
from torch import Tensor

from .. import native
from .packing import PackCache, _expect, cname, isa, kids
from .sam_decoder import HQ_NODES, CompiledSegmentAnything, SAMDecoderLowering, _multilinear


def _is_hq(sam: Any) -> bool:
    return any(cname(m) in HQ_NODES for m in sam.modules())


def _convt_ok(ct: Any, cin: int, cout: int) -> bool:
    return (isa(ct, "ConvTranspose2d") and ct.in_channels == cin and ct.out_channels == cout and tuple(ct.kernel_size) == (2, 2) and tuple(ct.stride) == (2, 2)
            and ct.bias is not None)


class HQSAMDecoderLowering(SAMDecoderLowering):
    """SAMDecoderLowering for a tree with HQSAMAdapter injected: further input `early` [1, 64, 64, vit_dim], further output `hq`
    [P, 1, 256, 256] (`low` stays the base SAM mask)."""

    hq: Any = None  # the HQSAMMaskPrediction node of the tree being lowered (None: a plain tree)

    def check(self, sam: Any) -> tuple[Any, Any, Any, Any]:
        if not _is_hq(sam):
            return super().check(sam)
        ch = kids(sam)
        _expect(isa(sam, "SegmentAnything") and len(ch) == 4, "unexpected SegmentAnything layout")
        enc = kids(ch[0])[0] if isa(ch[0], "SAMViTAdapter") and len(kids(ch[0])) == 1 else ch[0]
        _expect(isa(ch[1], "PointEncoder") and isa(ch[2], "MaskEncoder") and isa(ch[3], "MaskDecoder"), "unexpected SegmentAnything children")
        _expect([cname(c) for c in kids(ch[3])] == ["MaskDecoderTokensExtender", "EmbeddingsAggregator", "Transformer", "Predictions", "PredictionsPostProc"],
                "unexpected MaskDecoder layout under HQSAMAdapter")
        _expect(tuple(getattr(enc, "image_embedding_size", ())) == (64, 64) and getattr(ch[3], "embedding_dim", None) == 256,
                "only the 64 x 64 x 256 SAM image embedding is lowered")
        _expect(not ch[3].multimask_output, "HQ-SAM predicts one mask")
        return enc, ch[1], ch[2], ch[3]

    def decoder_parts(self, dec: Any) -> tuple[Any, Any, Any]:
        parts = kids(dec)
        if len(parts) == 4:
            self.hq = None
            return super().decoder_parts(dec)
        ext, _agg, transformer, predictions, _post = parts
        ek = kids(ext)
        _expect(len(ek) == 2 and isa(ek[0], "MaskDecoderTokens") and isa(ek[1], "Chain") and len(kids(ek[1])) == 2 and isa(kids(ek[1])[1], "Parameter")
                and tuple(kids(ek[1])[1].weight.shape) == (1, 256) and tuple(kids(ek[0])[1].weight.shape) == (5, 256), "unexpected MaskDecoderTokensExtender layout")
        mpa, ip = kids(predictions)
        _expect(isa(mpa, "MaskPredictionAdapter") and len(kids(mpa)) == 2 and isa(kids(mpa)[0], "MaskPrediction") and isa(kids(mpa)[1], "Chain"),
                "unexpected MaskPredictionAdapter layout")
        tail = kids(kids(mpa)[1])
        _expect(len(tail) == 2 and isa(tail[0], "HQSAMMaskPrediction") and isa(tail[1], "Reshape"), "unexpected HQ mask prediction layout")
        self.hq = tail[0]
        return transformer, kids(mpa)[0], ip

    def make_io(self, P: int, T: int, has_mask: bool, k_out: int, C: int) -> dict[str, Any]:
        io = super().make_io(P, T, has_mask, k_out, C)
        if self.hq is not None:
            _expect(k_out == 1, "HQ-SAM predicts one mask")
            vit_dim = self.hq_parts()["compress"][0].in_channels
            io["early"] = torch.empty(1, 64, 64, vit_dim, device=self.device, dtype=self.dtype)
            io["hq"] = torch.empty(P, 1, 256, 256, device=self.device, dtype=self.dtype)
        return io

    def hq_parts(self) -> dict[str, Any]:
        """The leaves of HQSAMMaskPrediction, with their layout checked."""
        mlp, chain = kids(self.hq)
        _expect(isa(mlp, "HQTokenMLP") and isa(chain, "Chain") and len(kids(chain)) == 2 and isa(kids(chain)[0], "DenseEmbeddingUpscalingHQ") and isa(kids(chain)[1], "Flatten"),
                "unexpected HQSAMMaskPrediction layout")
        sl, ml = kids(mlp)
        _expect(isa(sl, "Slicing") and (sl.dim, sl.start, sl.end) == (1, 5, 6), "the HQ token is not token 5")
        feat, hqf = kids(kids(chain)[0])
        _expect(isa(feat, "EmbeddingMaskfeature") and isa(hqf, "HQFeatures"), "unexpected DenseEmbeddingUpscalingHQ layout")
        fk = kids(feat)
        _expect([cname(c) for c in fk] == ["UseContext", "Reshape", "Conv2d", "LayerNorm2d", "GeLU", "Conv2d"] and fk[0].key == "upscaled_dense_embedding",
                "unexpected EmbeddingMaskfeature layout")
        c1, ln, c2 = fk[2], fk[3], fk[5]
        for c, cin, cout in ((c1, 32, 64), (c2, 64, 32)):
            _expect((c.in_channels, c.out_channels) == (cin, cout) and tuple(c.kernel_size) == (3, 3) and tuple(c.stride) == (1, 1) and tuple(c.padding) == (1, 1)
                    and c.bias is not None, "unexpected EmbeddingMaskfeature convolution")
        ee, cv = kids(hqf)
        _expect(isa(ee, "EmbeddingEncoder") and isa(cv, "CompressViTFeat"), "unexpected HQFeatures layout")
        ek, ck = kids(ee), kids(cv)
        _expect([cname(c) for c in ek] == ["UseContext", "ConvTranspose2d", "LayerNorm2d", "GeLU", "ConvTranspose2d"] and ek[0].key == "image_embedding"
                and _convt_ok(ek[1], 256, 64) and _convt_ok(ek[4], 64, 32), "unexpected EmbeddingEncoder layout")
        _expect([cname(c) for c in ck] == ["UseContext", "Permute", "ConvTranspose2d", "LayerNorm2d", "GeLU", "ConvTranspose2d"] and ck[0].key == "early_vit_embedding"
                and tuple(ck[1].dims) == (0, 3, 1, 2) and _convt_ok(ck[2], ck[2].in_channels, 256) and _convt_ok(ck[5], 256, 32)
                and ck[2].in_channels % self.kblk == 0, "unexpected CompressViTFeat layout")
        return dict(mlp=_multilinear(ml), conv1=c1, ln=ln, conv2=c2, encoder=(ek[1], ek[2], ek[4]), compress=(ck[2], ck[3], ck[5]))

    # -- emitters -------------------------------------------------------------------------------------------------
    def _convt_gemm(self, x: Tensor, ct: Any, tag: str) -> Tensor:
        """ConvTranspose2d(Ci -> Co, 2, 2) of token-major x as ONE GEMM: column q * Co + c = output channel c of quadrant q = (dy, dx)."""
        co = ct.out_channels
        w = self.cache.get((tag,) + PackCache.ident(ct.weight), lambda: self.cvt(ct.weight.detach().permute(2, 3, 1, 0).reshape(4 * co, ct.in_channels)))
        b = self.cache.get((tag + "_b",) + PackCache.ident(ct.bias), lambda: self.cvt(ct.bias.detach()).repeat(4).contiguous())
        y = self.pool.get(x.shape[0], 4 * co)
        native.gemm([(x, self.kblocked(w))], y, bias=b)
        return y

    def hq_features(self, parts: dict[str, Any], early: Tensor) -> Tensor:
        """Fq [16384, 128] (quadrant layout) of the image embedding self.img [4096, 256] and the early ViT embedding [1, 64, 64, vit_dim]."""
        ct1, ln, ct2 = parts["encoder"]
        y = self._convt_gemm(self.img, ct1, "hq_enc_ct1")
        a = self.pool.get(4 * 4096, 64)
        native.convt2x2_ln_gelu(y, 64, 4, self._f32(ln.weight), self._f32(ln.bias), float(ln.eps), a, scatter_hw=(64, 64))
        self.pool.put(y)
        cv1, cln, cv2 = parts["compress"]
        y = self._convt_gemm(early.view(4096, early.shape[-1]), cv1, "hq_vit_ct1")
        b = self.pool.get(4 * 4096, 256)
        native.ln2d_gelu_wide(y, 256, self._f32(cln.weight), self._f32(cln.bias), float(cln.eps), b, scatter_hw=(64, 64))
        self.pool.put(y)
        pack = lambda ct: self.cvt(ct.weight.detach().permute(2, 3, 1, 0).reshape(4 * 32, ct.in_channels))  # noqa: E731
        wa = self.cache.get(("hq_enc_ct2",) + PackCache.ident(ct2.weight), lambda: pack(ct2))
        wb = self.cache.get(("hq_vit_ct2",) + PackCache.ident(cv2.weight), lambda: pack(cv2))
        bias = self.cache.get(("hq_ct2_b",) + PackCache.ident(ct2.bias, cv2.bias),
                              lambda: (ct2.bias.detach().to(self.device, torch.float32) + cv2.bias.detach().to(self.device, torch.float32)).to(self.dtype).repeat(4).contiguous())
        fq = self.pool.get(4 * 4096, 128)
        native.gemm([(a, self.kblocked(wa)), (b, self.kblocked(wb))], fq, bias=bias)
        self.pool.put(a)
        self.pool.put(b)
        return fq

    def mask_head(self, up1: Tensor, P: int, wct2: Tensor, bias: Tensor, hyper: Tensor, io: dict[str, Any]) -> None:
        if self.hq is None:
            return super().mask_head(up1, P, wct2, bias, hyper, io)
        # conv_gemm takes channel counts that are a multiple of one 128-byte K block: 32 float32, 64 bfloat16 (columns 32.. stay zero)
        self.u = self.pool.get(P * 65536, 32) if self.kblk == 32 else self._zeros(P * 65536, self.kblk)
        native.sam_mask_head_up(up1, P, 128, 128, wct2, bias, hyper, io["low"], self.u)

    def predictions(self, mp: Any, ip: Any, x: Tensor, dense: Tensor, P: int, T: int, first: int, k_out: int, io: dict[str, Any]) -> None:
        super().predictions(mp, ip, x, dense, P, T, first, k_out, io)
        if self.hq is None:
            return
        parts = self.hq_parts()
        fq = self.hq_features(parts, io["early"])
        l1, l2, l3 = parts["mlp"]
        _expect(l3.out_features == 32, "unexpected HQ token MLP width")
        h1 = self._lin(self._rows(x, P, T, 5), l1, relu=True)
        h2 = self._lin(h1, l2, relu=True)
        h = self._lin(h2, l3)
        self.pool.put(h1)
        self.pool.put(h2)
        c1, ln, c2 = parts["conv1"], parts["ln"], parts["conv2"]
        cu = self.u.shape[1]

        def w1() -> Tensor:  # [64, (ky, kx, channel of u)] with the channels padded to u's row
            w = torch.zeros(64, cu, 3, 3, device=self.device, dtype=torch.float32)
            w[:, :32] = c1.weight.detach().to(self.device, torch.float32)
            return native.pack_conv_weight(w).to(self.dtype).contiguous()

        W1 = self.cache.get(("hq_conv1", cu) + PackCache.ident(c1.weight), w1)
        y = self.pool.get(P * 65536, 64)
        native.conv_gemm([(self.u.view(P, 256, 256, cu), self.kblocked(W1), 3, 1, 1)], y, P, 256, 256, bias=self._w(c1.bias))
        W2 = self.cache.get(("hq_conv2",) + PackCache.ident(c2.weight), lambda: c2.weight.detach().to(self.device, torch.float32).permute(0, 2, 3, 1).reshape(32, 9, 64).contiguous())
        native.sam_hq_mask_head(y, P, 256, 256, self._f32(ln.weight), self._f32(ln.bias), float(ln.eps), W2, self._f32(c2.bias), h, fq, io["hq"])
        self.pool.put(y)
        self.pool.put(fq)
        self.pool.put(h)


class CompiledHQSegmentAnything(CompiledSegmentAnything):
    """CompiledSegmentAnything for a SegmentAnything with HQSAMAdapter injected: `predict`, `predict_batch` and `compute_image_embedding`
    with the same signatures, the HQ branch on the MI355X kernels.  The early ViT embedding is read from context "hq_sam" at call time
    (compute_image_embedding writes it), or passed to predict_batch as early_vit_embedding=.  Without the adapter (or after eject())
    this is CompiledSegmentAnything."""

    lowering_cls = HQSAMDecoderLowering

    def _post_proc(self) -> Optional[Any]:
        return next((m for m in self.sam.mask_decoder.modules() if isa(m, "PredictionsPostProc")), None)

    def _hq_context(self) -> dict:
        node = next(m for m in self.sam.mask_decoder.modules() if isa(m, "UseContext") and m.context == "hq_sam")
        return node.use_context("hq_sam")

    def _tokens(self) -> Tensor:
        node = kids(self.sam.mask_decoder)[0]
        if not isa(node, "MaskDecoderTokensExtender"):
            return super()._tokens()
        regular, extra = kids(node)
        return torch.cat([kids(regular)[1].weight, kids(extra)[1].weight.to(kids(regular)[1].weight.dtype)], dim=0)

    def _fill_inputs(self, io: dict[str, Any]) -> None:
        if "early" not in io:
            return
        early = self._hq_context().get("early_vit_embedding")
        _expect(early is not None, 'context "hq_sam" holds no early_vit_embedding: run compute_image_embedding, or pass early_vit_embedding=')
        _expect(early.numel() == io["early"].numel(), f"early ViT embedding of shape {tuple(early.shape)}: the program takes {tuple(io['early'].shape)}")
        io["early"].copy_(early.reshape(io["early"].shape))

    def _low_res(self, io: dict[str, Any]) -> Tensor:
        if "hq" not in io:
            return super()._low_res(io)
        return io["hq"].clone() if self._post_proc().hq_mask_only else io["hq"] + io["low"]

    @torch.no_grad()
    def predict_batch(self, embedding: Any, points: Any, point_types: Any, low_res_masks: Optional[Tensor] = None, original_size: Optional[tuple[int, int]] = None,
                      binarize: bool = True, early_vit_embedding: Optional[Tensor] = None) -> tuple[Tensor, Tensor, Tensor]:
        """CompiledSegmentAnything.predict_batch; early_vit_embedding [1, 64, 64, vit_dim] goes with a bare embedding tensor (it is put into
        context "hq_sam", where the native program and the stock forward both read it)."""
        if early_vit_embedding is not None and self._post_proc() is not None:
            self._hq_context()["early_vit_embedding"] = early_vit_embedding
        return super().predict_batch(embedding, points, point_types, low_res_masks=low_res_masks, original_size=original_size, binarize=binarize)
