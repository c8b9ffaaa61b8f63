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
KTOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2}


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
    z = F.conv_transpose2d(x, w, b, stride=2)
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
    assert _rel(out.float(), ref) < (1e-5 if dtype == torch.float32 else 1e-2)
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
