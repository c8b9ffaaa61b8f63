"""SAM mask prediction on the MI355X: the kernels of csrc/sam_decoder.hip against float32 torch, CompiledSegmentAnything.predict against
the real reference's outputs (tests/golden/sam_h_decoder.safetensors), predict_batch against single predictions, and the fallback."""
import json
import os
import sys
import warnings
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from refiners_amd import native, synth
from refiners_amd.engine.sam_decoder import CompiledSegmentAnything
from refiners_amd.segment_anything import ImageEmbedding, MaskDecoder, SegmentAnythingH, compute_scaled_size, postprocess_masks
from tests import support as S
from tests.sam_decoder_cases import SAM_DECODER_CASE, SAM_DECODER_CASES, decoder_sample, embedding, low_res_mask

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
REF = Path(os.environ.get("REFINERS_SRC") or Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "src")
DTYPES = [torch.float32, torch.bfloat16]
# relative l2: bf16 outputs are a float32 result rounded to 8 significant bits (<= 2^-9 per element) against a reference computed from the
# same rounded inputs, so twice the worst rounding bounds the l2 figure (tests/test_sam_decoder_kernels_gpu.py holds the per-element bounds)
KTOL = {torch.float32: 1e-5, torch.bfloat16: 2.0**-8}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,Lq,Lk,shared", [(32, 7, 7, ""), (16, 4096, 9, "q"), (16, 9, 4096, "kv"), (16, 6, 1000, "")])
def test_sam_attention(dtype, D, Lq, Lk, shared):
    g = torch.Generator(device=DEV).manual_seed(3)
    B, H = 3, 8
    q = torch.randn(1 if "q" in shared else B, Lq, H * D + 8, device=DEV, generator=g)[..., : H * D]
    k = torch.randn(1 if "kv" in shared else B, Lk, 2 * H * D, device=DEV, generator=g)
    kk, vv = k[..., : H * D], k[..., H * D :]
    out = torch.empty(B, Lq, H * D, device=DEV, dtype=dtype)
    ws = torch.empty(max(native.sam_attention_ws_floats(B, H, D, Lq, Lk), 1), device=DEV)
    native.sam_attention(q.to(dtype), kk.to(dtype), vv.to(dtype), out, H, ws=ws)
    heads = lambda t: t.expand(B, -1, -1).reshape(B, t.shape[1], H, D).transpose(1, 2).to(dtype).float()  # noqa: E731
    ref = F.scaled_dot_product_attention(heads(q), heads(kk), heads(vv)).transpose(1, 2).reshape(B, Lq, H * D)
    assert _rel(out.float(), ref) < KTOL[dtype]
    again = torch.empty_like(out)
    native.sam_attention(q.to(dtype), kk.to(dtype), vv.to(dtype), again, H, ws=ws)
    assert torch.equal(out, again)


@pytest.mark.parametrize("dtype", DTYPES)
def test_convt2x2_ln_gelu(dtype):
    g = torch.Generator(device=DEV).manual_seed(4)
    P, Hs, Ws, Ci, Co = 2, 8, 12, 64, 64
    x = torch.randn(P, Ci, Hs, Ws, device=DEV, generator=g)
    w = torch.randn(Ci, Co, 2, 2, device=DEV, generator=g) / 8
    b, gam, bet = (torch.randn(Co, device=DEV, generator=g) for _ in range(3))
    y = (x.permute(0, 2, 3, 1).reshape(-1, Ci) @ w.permute(2, 3, 1, 0).reshape(4 * Co, Ci).t() + b.repeat(4)).to(dtype)
    out = torch.empty(4 * P * Hs * Ws, Co, device=DEV, dtype=dtype)
    native.convt2x2_ln_gelu(y, Co, 4, gam, bet, 1e-6, out, scatter_hw=(Hs, Ws))
    z = y.float().view(P, Hs, Ws, 2, 2, Co).permute(0, 5, 1, 3, 2, 4).reshape(P, Co, 2 * Hs, 2 * Ws)  # the kernel's input, as an image
    assert _rel(z, F.conv_transpose2d(x, w, b, stride=2)) < (1e-4 if dtype == torch.float32 else 2.0**-8)  # (a layout check)
    mu, var = z.mean(1, keepdim=True), z.var(1, keepdim=True, unbiased=False)
    ref = F.gelu(gam[:, None, None] * (z - mu) / torch.sqrt(var + 1e-6) + bet[:, None, None])
    assert _rel(out.float().view(P, 2 * Hs, 2 * Ws, Co).permute(0, 3, 1, 2), ref) < KTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nk", [1, 3])
def test_sam_mask_head(dtype, nk):
    g = torch.Generator(device=DEV).manual_seed(5)
    P, Hin, Win = 3, 16, 20
    x = torch.randn(P, 64, Hin, Win, device=DEV, generator=g)
    w = torch.randn(64, 32, 2, 2, device=DEV, generator=g) / 8
    b = torch.randn(32, device=DEV, generator=g)
    hyper = torch.randn(P, 4, 32, device=DEV, generator=g)
    rows = x.permute(0, 2, 3, 1).reshape(-1, 64).to(dtype).contiguous()
    out = torch.empty(P, nk, 2 * Hin, 2 * Win, device=DEV, dtype=dtype)
    native.sam_mask_head(rows, P, Hin, Win, w.permute(0, 2, 3, 1).reshape(64, 128).contiguous(), b, hyper.to(dtype)[:, 1 : 1 + nk], out)
    up = F.gelu(F.conv_transpose2d(rows.float().view(P, Hin, Win, 64).permute(0, 3, 1, 2), w, b, stride=2))
    ref = torch.matmul(hyper.to(dtype).float()[:, 1 : 1 + nk], up.flatten(2)).view(P, nk, 2 * Hin, 2 * Win)
    assert _rel(out.float(), ref) < KTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(600, 900), (1024, 1024), (333, 250)])
def test_sam_postprocess_masks(dtype, size):
    g = torch.Generator(device=DEV).manual_seed(6)
    low = torch.randn(2, 3, 256, 256, device=DEV, generator=g).to(dtype)
    out = torch.empty(2, 3, *size, device=DEV, dtype=dtype)
    native.sam_postprocess_masks(low, 1024, compute_scaled_size(size, 1024), out)
    ref = postprocess_masks(low.float(), size, 1024)
    assert _rel(out.float(), ref) < KTOL[dtype]
    binary = torch.empty(2, 3, *size, device=DEV, dtype=torch.bool)
    native.sam_postprocess_masks(low, 1024, compute_scaled_size(size, 1024), binary, threshold=0.0)
    far = ref.abs() > 1e-3
    assert torch.equal(binary[far], (ref > 0)[far])


# ------------------------------------------------------------------------------------------------ end to end
_SD = {}


def _sam(multimask, dtype):
    if not _SD:
        shapes = {k: tuple(v) for k, v in json.loads((S.GOLD / "sam_h_decoder_keys.json").read_text()).items()}
        _SD.update(synth.synth_state_dict({k: v for k, v in shapes.items() if not k.startswith("SAMViTH.")}, SAM_DECODER_CASE["weight_seed"]))
    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=multimask), device=DEV, dtype=dtype)
    sam.load_state_dict({k: v.to(DEV, dtype) for k, v in _SD.items()}, strict=False)
    return sam


def _predict(fast, name, dtype):
    case = SAM_DECODER_CASES[name]
    kw = {k: case[k] for k in ("foreground_points", "background_points", "box_points") if k in case}
    if case.get("low_res_mask"):
        kw["low_res_mask"] = low_res_mask().to(DEV, dtype)
    return fast.predict(ImageEmbedding(embedding().to(DEV, dtype), case["original_size"]), binarize=False, **kw)


_FAST = {}


def _fast(multimask, dtype):
    if (multimask, dtype) not in _FAST:
        _FAST[(multimask, dtype)] = CompiledSegmentAnything(_sam(multimask, dtype))
    return _FAST[(multimask, dtype)]


@pytest.mark.parametrize("name", list(SAM_DECODER_CASES))
def test_predict_float32_matches_reference(name):
    fast = _fast(SAM_DECODER_CASES[name]["multimask"], torch.float32)
    masks, iou, low = _predict(fast, name, torch.float32)
    assert fast.stats["whole_fallback"] is None and fast.stats["fallback_nodes"] == []
    gold = S.golden("sam_h_decoder")
    got = decoder_sample(masks.cpu(), iou.cpu(), low.cpu())
    for k in ("low_res", "iou", "masks"):
        l2, mx = S.rel_err(got[k], gold[f"{name}.{k}"])
        assert l2 < 1e-3 and mx < 1e-3, (k, l2, mx)
    binary, _, _ = fast.predict(ImageEmbedding(embedding().to(DEV), SAM_DECODER_CASES[name]["original_size"]),
                                **{k: v for k, v in SAM_DECODER_CASES[name].items() if k.endswith("points")},
                                low_res_mask=low_res_mask().to(DEV) if SAM_DECODER_CASES[name].get("low_res_mask") else None)
    assert binary.dtype == torch.bool and binary.shape == masks.shape


@pytest.mark.parametrize("name", list(SAM_DECODER_CASES))
def test_predict_bfloat16_matches_reference(name):
    """bf16: low_res_masks within 5 % and iou_predictions within 10 % relative l2 (0.05 absolute) of the float32 reference; binarised masks
    agree on >= 99.5 % of the (sampled) pixels whose reference logit is more than 0.1 away from zero."""
    masks, iou, low = _predict(_fast(SAM_DECODER_CASES[name]["multimask"], torch.bfloat16), name, torch.bfloat16)
    assert masks.dtype == torch.bfloat16 and low.dtype == torch.bfloat16
    gold = S.golden("sam_h_decoder")
    got = decoder_sample(masks.float().cpu(), iou.float().cpu(), low.float().cpu())
    assert S.rel_err(got["low_res"], gold[f"{name}.low_res"])[0] < 5e-2
    gi = gold[f"{name}.iou"]
    assert float((got["iou"] - gi).norm() / gi.norm()) < 0.1 and float((got["iou"] - gi).abs().max()) < 0.05, (got["iou"], gi)
    ref = gold[f"{name}.masks"]
    sure = ref.abs() > 0.1
    agree = ((got["masks"] > 0) == (ref > 0))[sure].float().mean()
    assert agree >= 0.995, float(agree)


def test_predict_batch_equals_single_predictions():
    fast = _fast(True, torch.float32)
    emb = embedding().to(DEV)
    size = (600, 900)
    g = torch.Generator().manual_seed(7)
    pts, types = [], []
    for p in range(16):
        n = 1 + p % 3
        c = torch.rand(n, 2, generator=g) * torch.tensor([900.0, 600.0])
        t = torch.randint(1, 3, (n,), generator=g)
        if p % 5 == 4:  # a box prompt
            c = torch.cat([c, torch.tensor([[100.0, 80.0], [700.0, 500.0]])])
            t = torch.cat([t, torch.tensor([3, 4])])
        pts.append(c)
        types.append(t)
    masks, iou, low = fast.predict_batch(emb, pts, types, original_size=size, binarize=False)
    assert masks.shape == (16, 3, *size) and iou.shape == (16, 3) and low.shape == (16, 3, 256, 256)
    for p in range(16):
        names = {1: "background_points", 2: "foreground_points"}
        kw = {v: [tuple(xy) for xy, tt in zip(pts[p].tolist(), types[p].tolist()) if tt == k] or None for k, v in names.items()}
        tl = [tuple(xy) for xy, tt in zip(pts[p].tolist(), types[p].tolist()) if tt == 3]
        br = [tuple(xy) for xy, tt in zip(pts[p].tolist(), types[p].tolist()) if tt == 4]
        kw["box_points"] = [[a, b] for a, b in zip(tl, br)] or None
        m1, i1, l1 = fast.predict(ImageEmbedding(emb, size), binarize=False, **kw)
        assert _rel(low[p : p + 1], l1) < 1e-5 and _rel(iou[p : p + 1], i1) < 1e-5 and _rel(masks[p : p + 1], m1) < 1e-5, p
    again = fast.predict_batch(emb, pts, types, original_size=size, binarize=False)
    assert all(torch.equal(a, b) for a, b in zip((masks, iou, low), again))


def _points(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    return [tuple(p) for p in (torch.rand(n, 2, generator=g) * torch.tensor([size[1], size[0]])).tolist()]


def _close_to_mirror(got, ref, tol):
    for name, a, b in zip(("masks", "iou", "low_res"), got, ref):
        assert a.shape == b.shape and _rel(a, b) < tol, (name, _rel(a, b))


def test_predict_at_the_largest_prompt_runs_native():
    """T = 64 prompt tokens (5 decoder tokens + 58 points + the pad point), the most the lowering takes: no fallback, 64 keys in the token
    self-attention and 64 queries in the token -> image attention; equal to the mirror's unfused forward."""
    fast = _fast(True, torch.float32)
    emb = ImageEmbedding(embedding().to(DEV), (1024, 1024))
    pts = _points(58, (1024, 1024), 11)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = fast.predict(emb, foreground_points=pts[:40], background_points=pts[40:], binarize=False)
    assert fast.stats["whole_fallback"] is None and fast.stats["fallback_nodes"] == []
    kinds = fast.stats["attention_kinds"]
    assert kinds.count("h8xd32 Lq=64 Lk=64") == 2 and kinds.count("h8xd16 Lq=64 Lk=4096") == 3 and kinds.count("h8xd16 Lq=4096 Lk=64") == 2, kinds
    _close_to_mirror(got, fast.sam.predict(emb, foreground_points=pts[:40], background_points=pts[40:], binarize=False), 1e-4)


def test_one_token_too_many_falls_back_for_that_count_only():
    """T = 65 (59 points): RuntimeWarning and the stock result; the refusal stays with that token count, a 1-point prompt runs native."""
    fast = _fast(True, torch.float32)
    emb = ImageEmbedding(embedding().to(DEV), (1024, 1024))
    one = dict(foreground_points=[(500.0, 400.0)], binarize=False)
    before = fast.predict(emb, **one)
    pts = _points(59, (1024, 1024), 12)
    with pytest.warns(RuntimeWarning, match="64 keys"):
        got = fast.predict(emb, foreground_points=pts, binarize=False)
    assert fast.stats["whole_fallback"]
    ref = fast.sam.predict(emb, foreground_points=pts, binarize=False)
    for a, b in zip(got, ref):  # (the same unfused forward twice)
        assert a.shape == b.shape and torch.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        after = fast.predict(emb, **one)
    assert fast.stats["whole_fallback"] is None
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_predict_batch_of_64_equals_single_predictions():
    """P = 64 prompts of two points each (one program, the benchmark's batch) against 64 predict() calls."""
    fast = _fast(True, torch.float32)
    emb, size = embedding().to(DEV), (480, 640)
    g = torch.Generator().manual_seed(13)
    pts = torch.rand(64, 2, 2, generator=g) * torch.tensor([640.0, 480.0])
    types = torch.randint(1, 3, (64, 2), generator=g)
    masks, iou, low = fast.predict_batch(emb, pts, types, original_size=size, binarize=False)
    assert fast.stats["whole_fallback"] is None and masks.shape == (64, 3, *size)
    for p in range(64):
        kw = {name: [tuple(xy) for xy, t in zip(pts[p].tolist(), types[p].tolist()) if t == k] or None
              for k, name in ((1, "background_points"), (2, "foreground_points"))}
        m1, i1, l1 = fast.predict(ImageEmbedding(emb, size), binarize=False, **kw)
        assert _rel(low[p : p + 1], l1) < 1e-5 and _rel(iou[p : p + 1], i1) < 1e-5 and _rel(masks[p : p + 1], m1) < 1e-5, p


def test_predict_batch_with_mask_prompts_equals_single_predictions():
    """low_res_masks [8, 1, 256, 256] through the batched MaskEncoder against predict(low_res_mask=...) one prompt at a time."""
    fast = _fast(True, torch.float32)
    emb, size = embedding().to(DEV), (600, 900)
    masks_in = torch.cat([low_res_mask(100 + p) for p in range(8)]).to(DEV)
    pts = [torch.tensor([[100.0 + 90 * p, 50.0 + 60 * p]]) for p in range(8)]
    types = [torch.tensor([2 if p % 3 else 1]) for p in range(8)]
    masks, iou, low = fast.predict_batch(emb, pts, types, low_res_masks=masks_in, original_size=size, binarize=False)
    assert fast.stats["whole_fallback"] is None
    for p in range(8):
        name = "foreground_points" if p % 3 else "background_points"
        m1, i1, l1 = fast.predict(ImageEmbedding(emb, size), low_res_mask=masks_in[p : p + 1], binarize=False, **{name: [tuple(pts[p][0].tolist())]})
        assert _rel(low[p : p + 1], l1) < 1e-5 and _rel(iou[p : p + 1], i1) < 1e-5 and _rel(masks[p : p + 1], m1) < 1e-5, p


def test_predict_original_larger_than_the_encoder_matches_the_mirror():
    """original_size (1536, 2048): the outer resize of postprocess_masks upsamples from the (768, 1024) crop."""
    fast = _fast(True, torch.float32)
    emb = ImageEmbedding(embedding().to(DEV), (1536, 2048))
    kw = dict(foreground_points=[(1500.0, 700.0)], background_points=[(300.0, 1200.0)], binarize=False)
    got = fast.predict(emb, **kw)
    assert fast.stats["whole_fallback"] is None and got[0].shape == (1, 3, 1536, 2048)
    _close_to_mirror(got, fast.sam.predict(emb, **kw), 1e-4)


def test_hq_sam_adapter_falls_back_to_the_stock_forward():
    if not (REF / "refiners").exists():
        pytest.skip("no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
    sys.path[:0] = [str(Path(__file__).resolve().parent.parent / "oracle" / "shim"), str(REF)]
    from refiners.foundationals.segment_anything.hq_sam import HQSAMAdapter
    from refiners.foundationals.segment_anything.model import ImageEmbedding as RefEmbedding
    from refiners.foundationals.segment_anything.model import SegmentAnythingH as RefSAM

    torch.manual_seed(0)
    sam = RefSAM(multimask_output=False).to(DEV)
    adapter = HQSAMAdapter(sam, weights=None).inject()
    adapter.set_context("hq_sam", {"early_vit_embedding": torch.randn(1, 64, 64, 1280, device=DEV) * 0.1})
    emb = RefEmbedding(embedding().to(DEV), (1024, 1024))
    ref = sam.predict(emb, foreground_points=[(500.0, 400.0)], binarize=False)
    fast = CompiledSegmentAnything(sam)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = fast.predict(emb, foreground_points=[(500.0, 400.0)], binarize=False)
    assert any(issubclass(w.category, RuntimeWarning) for w in caught) and fast.stats["whole_fallback"]
    for a, b in zip(got, ref):  # (the same unfused forward twice)
        assert a.shape == b.shape and torch.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-6)


def test_deep_unknown_node_falls_back_to_the_stock_forward():
    """A wrapped decoder Linear passes the top-level check and is refused deeper in the lowering: RuntimeWarning and the stock result."""
    import refiners_amd.fluxion.layers as fl

    sam = _sam(True, torch.float32)
    ff = next(m for m in sam.mask_decoder.modules() if type(m).__name__ == "FeedForward")
    lin = ff[0]
    ff.replace(lin, fl.Chain(lin))
    emb = ImageEmbedding(embedding().to(DEV), (1024, 1024))
    ref = sam.predict(emb, foreground_points=[(500.0, 400.0)], binarize=False)
    fast = CompiledSegmentAnything(sam)
    with pytest.warns(RuntimeWarning):
        got = fast.predict(emb, foreground_points=[(500.0, 400.0)], binarize=False)
    assert fast.stats["whole_fallback"]
    for a, b in zip(got, ref):  # (the same unfused forward twice)
        assert a.shape == b.shape and torch.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-6)
