"""SAM mask prediction without a GPU: the mirror's SegmentAnythingH against the real reference (tests/golden/sam_h_decoder*, written by
tools/make_golden_sam_decoder.py), dry lowerings of the mask decoder on the meta device, and numpy models of the index arithmetic of the
new kernels (csrc/sam_decoder.hip) against torch."""
import json
import os
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from refiners_amd import synth
from refiners_amd.engine.packing import Unsupported
from refiners_amd.engine.sam_decoder import SAMDecoderLowering
from refiners_amd.segment_anything import ImageEmbedding, MaskDecoder, SegmentAnythingH
from tests import support as S
from tests.sam_decoder_cases import SAM_DECODER_CASE, SAM_DECODER_CASES, decoder_sample, embedding, low_res_mask

TOL = 2e-4
REF = Path(os.environ.get("REFINERS_SRC") or Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "src")


def _shapes():
    return {k: tuple(v) for k, v in json.loads((S.GOLD / "sam_h_decoder_keys.json").read_text()).items()}


def test_mirror_keys_equal_the_reference():
    sam = SegmentAnythingH(device="meta")
    shapes = _shapes()
    assert list(sam.state_dict()) == list(shapes)
    assert {k: tuple(v.shape) for k, v in sam.state_dict().items()} == shapes


@pytest.mark.parametrize("name", list(SAM_DECODER_CASES))
def test_mirror_predict_matches_reference(name):
    case = SAM_DECODER_CASES[name]
    shapes = _shapes()
    sd = synth.synth_state_dict({k: v for k, v in shapes.items() if not k.startswith("SAMViTH.")}, SAM_DECODER_CASE["weight_seed"])
    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=case["multimask"], device="meta"), device="meta")
    sam.load_state_dict(sd, strict=False, assign=True)
    kw = {k: case[k] for k in ("foreground_points", "background_points", "box_points") if k in case}
    if case.get("low_res_mask"):
        kw["low_res_mask"] = low_res_mask()
    masks, iou, low = sam.predict(ImageEmbedding(embedding(), case["original_size"]), binarize=False, **kw)
    gold = S.golden("sam_h_decoder")
    for k, v in decoder_sample(masks, iou, low).items():
        l2, mx = S.rel_err(v, gold[f"{name}.{k}"])
        assert l2 <= TOL and mx <= TOL, (name, k, l2, mx)
    binary, _, _ = sam.predict(ImageEmbedding(embedding(), case["original_size"]), binarize=True, **kw)
    assert binary.dtype == torch.bool and binary.shape == masks.shape


# ------------------------------------------------------------------------------------------------ dry lowering
def _dry(sam, P, T, has_mask, dtype):
    low = SAMDecoderLowering(torch.device("meta"), dtype)
    low.lower(sam, P, T, has_mask, torch.empty(4096, 256, device="meta"))
    return low


EXPECTED = {  # launches of one program: (multimask, has_mask) -> kinds
    (True, False): {"mi355x_gemm": 36, "mi355x_layernorm": 9, "mi355x_sam_attention": 7, "mi355x_nchw_to_nhwc": 1, "mi355x_axpby": 1,
                    "mi355x_gather_rows": 1, "mi355x_convt2x2_ln_gelu": 1, "mi355x_sam_mask_head": 1},
    (True, True): {"mi355x_gemm": 39, "mi355x_layernorm": 9, "mi355x_sam_attention": 7, "mi355x_nchw_to_nhwc": 1, "mi355x_patchify_nchw": 1,
                   "mi355x_gather_rows": 1, "mi355x_convt2x2_ln_gelu": 3, "mi355x_sam_mask_head": 1},
    (False, True): {"mi355x_gemm": 33, "mi355x_layernorm": 9, "mi355x_sam_attention": 7, "mi355x_nchw_to_nhwc": 1, "mi355x_patchify_nchw": 1,
                    "mi355x_gather_rows": 1, "mi355x_convt2x2_ln_gelu": 3, "mi355x_sam_mask_head": 1},
}


def _check_program(low, multimask, has_mask):
    assert dict(Counter(e[2] for e in low.step)) == EXPECTED[(multimask, has_mask)]
    assert low.stats["fallback_nodes"] == []
    assert not [e[2] for e in low.step if e[0] is None or str(e[2]).startswith("torch:")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("multimask,has_mask,P,T", [(True, False, 1, 7), (False, True, 16, 8), (True, True, 4, 6)])
def test_decoder_lowers_without_fallback(dtype, multimask, has_mask, P, T):
    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=multimask, device="meta", dtype=dtype), device="meta", dtype=dtype)
    low = _dry(sam, P, T, has_mask, dtype)
    _check_program(low, multimask, has_mask)
    kinds = low.stats["attention_kinds"]
    assert kinds.count(f"h8xd32 Lq={T} Lk={T}") == 2 and kinds.count(f"h8xd16 Lq={T} Lk=4096") == 3 and kinds.count(f"h8xd16 Lq=4096 Lk={T}") == 2


def _ref_classes():
    if not (REF / "refiners").exists():
        pytest.skip("no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "oracle" / "shim"), str(REF)]
    from refiners.foundationals.segment_anything import image_encoder, mask_decoder, model, prompt_encoder

    return image_encoder, mask_decoder, model, prompt_encoder


def _ref_sam(multimask, dtype=torch.float32):
    """refiners' own SegmentAnything on the meta device (its SegmentAnythingH moves the parts to "cpu" first: built from the base class)."""
    ie, md, mo, pe = _ref_classes()
    kw = dict(device="meta", dtype=dtype)
    return mo.SegmentAnything(ie.SAMViTH(**kw), pe.PointEncoder(**kw), pe.MaskEncoder(**kw), md.MaskDecoder(multimask_output=multimask, **kw), **kw)


@pytest.mark.parametrize("multimask,has_mask,P,T", [(True, False, 1, 7), (False, True, 16, 8)])
def test_decoder_lowering_accepts_the_real_refiners_tree(multimask, has_mask, P, T):
    low = _dry(_ref_sam(multimask, torch.bfloat16), P, T, has_mask, torch.bfloat16)
    _check_program(low, multimask, has_mask)
    mirror = _dry(SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=multimask, device="meta", dtype=torch.bfloat16), device="meta", dtype=torch.bfloat16),
                  P, T, has_mask, torch.bfloat16)
    assert [e[2] for e in low.step] == [e[2] for e in mirror.step]


def test_hq_sam_adapter_is_refused():
    _ref_classes()
    from refiners.foundationals.segment_anything.hq_sam import HQSAMAdapter

    sam = _ref_sam(False)  # (HQ-SAM supports single-mask output only)
    HQSAMAdapter(sam, weights=None).inject()
    with pytest.raises(Unsupported):
        _dry(sam, 1, 7, False, torch.float32)


# ------------------------------------------------------------------------------------------------ numpy models of the kernels' indexing
def test_convt_2x2_scatter_model():
    """mi355x_convt2x2_ln_gelu's scatter after the GEMM [pixels, Ci] x [Ci, 4 Co] (column q * Co + c, q = (dy, dx)) == conv_transpose2d."""
    g = torch.Generator().manual_seed(0)
    P, H, W, Ci, Co = 2, 3, 5, 6, 4
    x = torch.randn(P, Ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Ci, Co, 2, 2, generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x, w, stride=2).numpy()
    rows = x.permute(0, 2, 3, 1).reshape(-1, Ci).numpy()
    wg = w.permute(2, 3, 1, 0).reshape(4 * Co, Ci).numpy()  # what the lowering packs
    y = rows @ wg.T
    out = np.zeros((P, 2 * H, 2 * W, Co))
    for m in range(P * H * W):
        p, yy, xx = m // (H * W), (m // W) % H, m % W
        for q in range(4):
            row = (p * 2 * H + 2 * yy + (q >> 1)) * (2 * W) + 2 * xx + (q & 1)
            out.reshape(-1, Co)[row] = y[m, q * Co : (q + 1) * Co]
    np.testing.assert_allclose(out.transpose(0, 3, 1, 2), ref, rtol=1e-12, atol=1e-12)


def test_mask_head_quadrant_model():
    """mi355x_sam_mask_head: lane (pixel), wave q; w[ci][q * 32 + co] = weight[ci][co][q / 2][q % 2]; output pixel (2y + q / 2, 2x + q % 2)."""
    g = torch.Generator().manual_seed(1)
    P, H, W, Ci, Co, nk = 2, 3, 4, 8, 5, 3
    x = torch.randn(P, Ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Ci, Co, 2, 2, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    hyper = torch.randn(P, nk, Co, generator=g, dtype=torch.float64)
    ref = (hyper @ F.gelu(F.conv_transpose2d(x, w, b, stride=2)).flatten(2)).reshape(P, nk, 2 * H, 2 * W).numpy()
    wp = w.permute(0, 2, 3, 1).reshape(Ci, 4 * Co).numpy()  # the lowering's packing
    xs = x.permute(0, 2, 3, 1).reshape(P, H * W, Ci).numpy()
    out = np.zeros((P, nk, 2 * H, 2 * W))
    for p in range(P):
        for pix in range(H * W):
            yy, xx = pix // W, pix % W
            for q in range(4):
                acc = F.gelu(torch.from_numpy(xs[p, pix] @ wp[:, q * Co : (q + 1) * Co] + b.numpy())).numpy()
                for kk in range(nk):
                    out[p, kk, 2 * yy + (q >> 1), 2 * xx + (q & 1)] = acc @ hyper[p, kk].numpy()
    np.testing.assert_allclose(out, ref, rtol=1e-10, atol=1e-10)


def _tap(dst, n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    src = max(np.float32(scale * np.float32(dst + 0.5) - np.float32(0.5)), np.float32(0))
    i0 = int(src)
    i1 = i0 + (1 if i0 < n_in - 1 else 0)
    l1 = np.float32(src - i0)
    return i0, i1, np.float32(1) - l1, l1


def _postprocess_model(low, R, scaled, size):
    """mi355x_sam_postprocess_masks: each output pixel = outer bilinear taps of the cropped R x R grid, each tap = inner bilinear of low."""
    Hin, Win = low.shape
    out = np.zeros(size, dtype=np.float64)
    for oy in range(size[0]):
        y0, y1, ly0, ly1 = _tap(oy, scaled[0], size[0])
        for ox in range(size[1]):
            x0, x1, lx0, lx1 = _tap(ox, scaled[1], size[1])
            v = 0.0
            for iy, wy in ((y0, ly0), (y1, ly1)):
                a0, a1, la0, la1 = _tap(iy, Hin, R)
                for ix, wx in ((x0, lx0), (x1, lx1)):
                    b0, b1, lb0, lb1 = _tap(ix, Win, R)
                    inner = la0 * (lb0 * low[a0, b0] + lb1 * low[a0, b1]) + la1 * (lb0 * low[a1, b0] + lb1 * low[a1, b1])
                    v += wy * wx * inner
            out[oy, ox] = v
    return out


@pytest.mark.parametrize("size", [(15, 22), (24, 16), (20, 20)])
def test_postprocess_composed_taps_model(size):
    from refiners_amd.segment_anything import compute_scaled_size, postprocess_masks

    g = torch.Generator().manual_seed(2)
    R, n = 32, 8
    low = torch.randn(1, 1, n, n, generator=g)
    ref = postprocess_masks(low, size, R)[0, 0].double().numpy()
    got = _postprocess_model(low[0, 0].numpy().astype(np.float64), R, compute_scaled_size(size, R), size)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ fallback below the top level
def _decoder_sam(multimask=True):
    shapes = _shapes()
    sd = synth.synth_state_dict({k: v for k, v in shapes.items() if not k.startswith("SAMViTH.")}, SAM_DECODER_CASE["weight_seed"])
    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=multimask, device="meta"), device="meta")
    sam.load_state_dict(sd, strict=False, assign=True)
    return sam


def _wrap_a_decoder_linear(sam):
    """The first FeedForward Linear of the mask decoder wrapped in a Chain: same result, a layout the lowering does not know."""
    import refiners_amd.fluxion.layers as fl

    ff = next(m for m in sam.mask_decoder.modules() if type(m).__name__ == "FeedForward")
    lin = ff[0]
    ff.replace(lin, fl.Chain(lin))


def test_deep_unknown_node_falls_back_to_the_stock_forward():
    """A tree that passes the top-level check but differs further down: RuntimeWarning, stats["whole_fallback"], the stock result (no error)."""
    from refiners_amd.engine.sam_decoder import CompiledSegmentAnything

    sam = _decoder_sam()
    _wrap_a_decoder_linear(sam)
    emb = ImageEmbedding(embedding(), (600, 900))
    ref = sam.predict(emb, foreground_points=[(450.0, 250.0)], binarize=False)
    fast = CompiledSegmentAnything(sam)
    for _ in range(2):  # the second call takes the remembered refusal
        with pytest.warns(RuntimeWarning, match="not lowered|unexpected"):
            got = fast.predict(emb, foreground_points=[(450.0, 250.0)], binarize=False)
        assert fast.stats["whole_fallback"]
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
    assert len(fast.bad_keys) == 1 and not fast.programs
    with pytest.warns(RuntimeWarning):
        masks, iou, low = fast.predict_batch(emb, [torch.tensor([[450.0, 250.0]])], [torch.tensor([2])], binarize=False)
    assert torch.equal(low, ref[2]) and torch.equal(iou, ref[1])


def test_unsupported_embedding_geometry_is_refused():
    sam = SegmentAnythingH(device="meta")
    sam.image_encoder.image_embedding_size = (32, 32)
    with pytest.raises(Unsupported):
        SAMDecoderLowering(torch.device("meta"), torch.float32).check(sam)
    with pytest.raises(Unsupported):
        _dry(SegmentAnythingH(device="meta"), 1, 70, False, torch.float32)  # more than 64 prompt tokens


# ------------------------------------------------------------------------------------------------ wrapper checks
def test_sam_attention_wrapper_refuses_narrow_views_and_head_widths(monkeypatch):
    """native.sam_attention refuses a q / k / v / out view narrower than H*D columns (the kernel would read or write past it) and a head
    width other than 16 or 32, before anything reaches the library (CPU tensors; a launch would fail the test)."""
    from refiners_amd import native

    monkeypatch.setattr(native, "_launch", lambda *a, **k: pytest.fail("the wrapper launched"))
    H, D, Lq, Lk = 8, 16, 5, 300
    q, out = torch.zeros(1, Lq, H * D + 8)[..., : H * D], torch.zeros(1, Lq, H * D)
    kv = torch.zeros(1, Lk, 2 * H * D)
    k, v = kv[..., : H * D], kv[..., H * D :]
    ws = torch.zeros(native.sam_attention_ws_floats(1, H, D, Lq, Lk))
    for args in ((q, kv[..., : H * D - 8], v, out), (q, k, kv[..., H * D : 2 * H * D - 1], out), (q, k, v, out[..., : H * D - 8])):
        with pytest.raises(AssertionError, match="columns"):
            native.sam_attention(*args, H, ws=ws)
    with pytest.raises(AssertionError):  # (a narrower q than out reads as another head width)
        native.sam_attention(q[..., : H * D - 1], k, v, out, H, ws=ws)
    narrow = torch.zeros(1, Lq, 64)
    with pytest.raises(AssertionError, match="head width 8"):
        native.sam_attention(narrow, kv[..., :64], kv[..., 64:128], narrow.clone(), 8, ws=ws)
