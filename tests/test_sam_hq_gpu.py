"""HQ-SAM mask prediction on the MI355X: CompiledHQSegmentAnything.predict against the real reference's outputs
(tests/golden/sam_hq_decoder.safetensors), the live hq_mask_only switch, predict_batch against single predictions, the per-token-count
fallback, eject(), the early ViT embedding from compute_image_embedding, refiners' own tree, and bfloat16 against the unfused bfloat16
forward of the same tree."""
import os
import sys
import warnings
from pathlib import Path

import pytest
import torch

from refiners_amd.engine.sam_hq import CompiledHQSegmentAnything
from refiners_amd.segment_anything import ImageEmbedding, postprocess_masks
from tests import support as S
from tests.sam_hq_cases import SAM_HQ_CASES, decoder_sample, early_embedding, embedding, hq_sam, low_res_mask, prompt_kwargs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


_FAST = {}


def _fast(dtype):
    """One adapted model and its compiled wrapper per dtype, shared by the tests: (fast, sam, adapter)."""
    if dtype not in _FAST:
        sam, adapter = hq_sam(DEV, dtype)
        _FAST[dtype] = (CompiledHQSegmentAnything(sam), sam, adapter)
    fast, sam, adapter = _FAST[dtype]
    adapter.hq_mask_only = False
    adapter.set_context("hq_sam", {"early_vit_embedding": early_embedding().to(DEV, dtype)})
    return fast, sam, adapter


def _case_kwargs(name, dtype):
    case = SAM_HQ_CASES[name]
    kw = prompt_kwargs(case)
    if case.get("low_res_mask"):
        kw["low_res_mask"] = low_res_mask().to(DEV, dtype)
    return ImageEmbedding(embedding().to(DEV, dtype), case["original_size"]), kw


def _check_against_golden(got, name, tol=1e-3):
    gold = S.golden("sam_hq_decoder")
    sample = decoder_sample(*(t.float().cpu() for t in got))
    for k in ("low_res", "iou", "masks"):
        l2, mx = S.rel_err(sample[k], gold[f"{name}.{k}"])
        assert l2 <= tol and mx <= tol, (name, k, l2, mx)


@pytest.mark.parametrize("name", list(SAM_HQ_CASES))
def test_predict_float32_matches_reference(name):
    fast, _sam, adapter = _fast(torch.float32)
    adapter.hq_mask_only = SAM_HQ_CASES[name]["hq_mask_only"]
    emb, kw = _case_kwargs(name, torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = fast.predict(emb, binarize=False, **kw)
    assert fast.stats["whole_fallback"] is None and fast.stats["fallback_nodes"] == []
    assert {"mi355x_sam_hq_mask_head", "mi355x_sam_mask_head_up", "mi355x_ln2d_gelu_wide"} <= {e[2] for e in next(iter(fast.programs.values()))[0].step}
    _check_against_golden(got, name)
    binary, _, _ = fast.predict(emb, **kw)
    assert binary.dtype == torch.bool and binary.shape == got[0].shape


def test_hq_mask_only_is_live_and_neither_relowers_nor_recaptures():
    fast, _sam, adapter = _fast(torch.float32)
    emb, kw = _case_kwargs("point_sum", torch.float32)
    summed = fast.predict(emb, binarize=False, **kw)
    programs = dict(fast.programs)
    graphs = {k: v[2].graph for k, v in programs.items()}
    adapter.hq_mask_only = True
    only = fast.predict(emb, binarize=False, **kw)
    assert fast.programs.keys() == programs.keys()
    for k, v in fast.programs.items():
        assert v[2] is programs[k][2] and v[2].graph is graphs[k] and v[0] is programs[k][0]
    _check_against_golden(summed, "point_sum")
    assert _rel(only[2], summed[2]) > 0.05  # (another mask: the base plane is a large part of the sum)
    adapter.hq_mask_only = False
    emb, kw = _case_kwargs("box_background_hq_only", torch.float32)
    adapter.hq_mask_only = True
    _check_against_golden(fast.predict(emb, binarize=False, **kw), "box_background_hq_only")


def _mixed_prompts(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    pts, types = [], []
    for p in range(n):
        k = 1 + p % 3
        c = torch.rand(k, 2, generator=g) * torch.tensor([float(size[1]), float(size[0])])
        t = torch.randint(1, 3, (k,), generator=g)
        if p % 5 == 4:  # a box prompt
            c = torch.cat([c, torch.tensor([[100.0, 80.0], [700.0, 500.0]])])
            t = torch.cat([t, torch.tensor([3, 4])])
        pts.append(c)
        types.append(t)
    return pts, types


def _single_kwargs(c, t):
    names = {1: "background_points", 2: "foreground_points"}
    kw = {v: [tuple(xy) for xy, tt in zip(c.tolist(), t.tolist()) if tt == k] or None for k, v in names.items()}
    tl = [tuple(xy) for xy, tt in zip(c.tolist(), t.tolist()) if tt == 3]
    br = [tuple(xy) for xy, tt in zip(c.tolist(), t.tolist()) if tt == 4]
    kw["box_points"] = [[a, b] for a, b in zip(tl, br)] or None
    return kw


def test_predict_batch_equals_single_predictions():
    """16 mixed prompts (1-3 points, every fifth a box) in one call against predict() one at a time, relative l2 <= 1e-5: per prompt for
    the two mask tensors; for iou over the batch's [16, 1] vector.  Single-mask mode leaves ONE iou number per prompt, the end of a
    256-term float32 dot product whose terms are O(1) and whose sum may cancel to a few hundredths: its error belongs to the terms, so the
    relative error of one such scalar has no bound, while the vector's norm is the scale of the head's output (the sibling test's per-prompt
    figure is a norm over three values for the same reason)."""
    fast, _sam, _adapter = _fast(torch.float32)
    emb, size = embedding().to(DEV), (600, 900)
    pts, types = _mixed_prompts(16, size, 7)
    masks, iou, low = fast.predict_batch(emb, pts, types, original_size=size, binarize=False)
    assert fast.stats["whole_fallback"] is None and masks.shape == (16, 1, *size) and iou.shape == (16, 1) and low.shape == (16, 1, 256, 256)
    singles = []
    for p in range(16):
        m1, i1, l1 = fast.predict(ImageEmbedding(emb, size), binarize=False, **_single_kwargs(pts[p], types[p]))
        assert _rel(low[p : p + 1], l1) < 1e-5 and _rel(masks[p : p + 1], m1) < 1e-5, p
        singles.append(i1)
    assert _rel(iou, torch.cat(singles)) < 1e-5
    again = fast.predict_batch(emb, pts, types, original_size=size, binarize=False)
    assert all(torch.equal(a, b) for a, b in zip((masks, iou, low), again))


def test_predict_batch_with_mask_prompts_equals_single_predictions():
    fast, _sam, _adapter = _fast(torch.float32)
    emb, size = embedding().to(DEV), (600, 900)
    masks_in = torch.cat([low_res_mask(100 + p) for p in range(8)]).to(DEV)
    pts = [torch.tensor([[100.0 + 90 * p, 50.0 + 60 * p]]) for p in range(8)]
    types = [torch.tensor([2 if p % 3 else 1]) for p in range(8)]
    masks, iou, low = fast.predict_batch(emb, pts, types, low_res_masks=masks_in, original_size=size, binarize=False)
    assert fast.stats["whole_fallback"] is None
    singles = []
    for p in range(8):
        m1, i1, l1 = fast.predict(ImageEmbedding(emb, size), low_res_mask=masks_in[p : p + 1], binarize=False, **_single_kwargs(pts[p], types[p]))
        assert _rel(low[p : p + 1], l1) < 1e-5 and _rel(masks[p : p + 1], m1) < 1e-5, p
        singles.append(i1)
    assert _rel(iou, torch.cat(singles)) < 1e-5
    again = fast.predict_batch(emb, pts, types, low_res_masks=masks_in, original_size=size, binarize=False)
    assert all(torch.equal(a, b) for a, b in zip((masks, iou, low), again))


def test_one_token_too_many_falls_back_for_that_count_only():
    """58 points give T = 6 + 58 + the pad point = 65: RuntimeWarning and the stock result; a 1-point prompt still runs native."""
    fast, sam, _adapter = _fast(torch.float32)
    emb = ImageEmbedding(embedding().to(DEV), (1024, 1024))
    one = dict(foreground_points=[(500.0, 400.0)], binarize=False)
    before = fast.predict(emb, **one)
    g = torch.Generator().manual_seed(12)
    pts = [tuple(p) for p in (torch.rand(58, 2, generator=g) * 1024).tolist()]
    with pytest.warns(RuntimeWarning, match="64 keys"):
        got = fast.predict(emb, foreground_points=pts, binarize=False)
    assert fast.stats["whole_fallback"]
    for a, b in zip(got, sam.predict(emb, foreground_points=pts, binarize=False)):  # (the same unfused forward twice)
        assert a.shape == b.shape and torch.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        after = fast.predict(emb, **one)
    assert fast.stats["whole_fallback"] is None and all(torch.equal(a, b) for a, b in zip(before, after))


def test_after_eject_the_plain_program_runs():
    sam, adapter = hq_sam(DEV)
    adapter.set_context("hq_sam", {"early_vit_embedding": early_embedding().to(DEV)})
    fast = CompiledHQSegmentAnything(sam)
    emb = ImageEmbedding(embedding().to(DEV), (1024, 1024))
    kw = dict(foreground_points=[(500.0, 400.0)], binarize=False)
    fast.predict(emb, **kw)
    assert "mi355x_sam_hq_mask_head" in {e[2] for e in next(iter(fast.programs.values()))[0].step}
    adapter.eject()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = fast.predict(emb, **kw)
    assert fast.stats["whole_fallback"] is None and len(fast.programs) == 1
    kinds = {e[2] for e in next(iter(fast.programs.values()))[0].step}
    assert "mi355x_sam_mask_head" in kinds and not kinds & {"mi355x_sam_hq_mask_head", "mi355x_sam_mask_head_up", "mi355x_ln2d_gelu_wide"}
    for a, b in zip(got, sam.predict(emb, **kw)):
        assert a.shape == b.shape and _rel(a, b) < 1e-4


def test_compute_image_embedding_hands_over_the_early_embedding():
    """The one test that builds the ViT: compute_image_embedding writes context hq_sam.early_vit_embedding, predict reads it at call time;
    the same embedding passed to predict_batch explicitly (the context emptied first) gives the same bits."""
    from PIL import Image

    from refiners_amd.segment_anything import HQSAMAdapter, MaskDecoder, SegmentAnythingH

    torch.manual_seed(0)
    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=False, device=DEV), device=DEV)
    adapter = HQSAMAdapter(sam).inject()
    fast = CompiledHQSegmentAnything(sam)
    g = torch.Generator().manual_seed(1)
    image = Image.fromarray((torch.rand(48, 64, 3, generator=g) * 255).to(torch.uint8).numpy())
    emb = fast.compute_image_embedding(image)
    early = adapter.use_context("hq_sam")["early_vit_embedding"]
    assert early is not None and early.shape == (1, 64, 64, 1280)
    early = early.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        first = fast.predict(emb, foreground_points=[(30.0, 20.0)], binarize=False)
        adapter.set_context("hq_sam", {"early_vit_embedding": None})
        second = fast.predict_batch(emb.features, [torch.tensor([[30.0, 20.0]])], [torch.tensor([2])], original_size=(48, 64), binarize=False, early_vit_embedding=early)
    assert fast.stats["whole_fallback"] is None and all(torch.equal(a, b) for a, b in zip(first, second))


def test_real_refiners_tree_runs_native():
    if not (REF / "refiners").exists():
        pytest.skip("no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
    sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF)]
    from refiners.foundationals.segment_anything.hq_sam import HQSAMAdapter
    from refiners.foundationals.segment_anything.model import ImageEmbedding as RefEmbedding
    from refiners.foundationals.segment_anything.model import SegmentAnythingH as RefSAM

    torch.manual_seed(0)
    sam = RefSAM(multimask_output=False).to(DEV)
    adapter = HQSAMAdapter(sam, weights=None).inject()
    adapter.set_context("hq_sam", {"early_vit_embedding": torch.randn(1, 64, 64, 1280, device=DEV) * 0.1})
    emb = RefEmbedding(embedding().to(DEV), (1024, 1024))
    kw = dict(foreground_points=[(500.0, 400.0)], background_points=[(200.0, 700.0)], binarize=False)
    ref = sam.predict(emb, **kw)
    fast = CompiledHQSegmentAnything(sam)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = fast.predict(emb, **kw)
    assert fast.stats["whole_fallback"] is None and fast.stats["fallback_nodes"] == []
    for name, a, b in zip(("masks", "iou", "low_res"), got, ref):
        assert a.shape == b.shape and _rel(a, b) < 1e-3, (name, _rel(a, b))


# ------------------------------------------------------------------------------------------------ bfloat16
#: what the native bfloat16 path may add to the UNFUSED bfloat16 forward of the same tree (docs/MEASUREMENTS_hq_sam.md holds both measured
#: columns): 1.5 x its relative l2 against the float32 golden, and 0.2 points of sign agreement on |logit| > 0.1 -- the margin for another
#: accumulation order on inputs rounded to 8 bits
BF16_L2_FACTOR, BF16_SIGN_POINTS = 1.5, 0.2  # docs/MEASUREMENTS_hq_sam.md


def _stock_bf16(sam, sam32, emb, case, kw):
    """The unfused bfloat16 forward of the adapted tree (SegmentAnything.predict's steps).  The point embedding comes from the float32
    PointEncoder: the tree's own PointTypeEmbedding writes float32 rows, which a bfloat16 model cannot index_put."""
    bf = torch.bfloat16
    size = case["original_size"]
    coords, types = sam32.point_encoder.points_to_tensor(**{k: v for k, v in kw.items() if k.endswith("points")})
    sam32.point_encoder.set_type_mask(type_mask=types)
    point_embedding = sam32.point_encoder(sam32.normalize(coords, original_size=size)).to(bf)
    pe = sam32.point_encoder.get_dense_positional_embedding(image_embedding_size=(64, 64)).to(bf)
    mask_embedding = sam.mask_encoder(kw["low_res_mask"]) if "low_res_mask" in kw else sam.mask_encoder.get_no_mask_dense_embedding(image_embedding_size=(64, 64))
    dec = sam.mask_decoder
    dec.set_image_embedding(image_embedding=emb.features)
    dec.set_mask_embedding(mask_embedding=mask_embedding)
    dec.set_point_embedding(point_embedding=point_embedding)
    dec.set_dense_positional_embedding(dense_positional_embedding=pe)
    low, iou = dec()
    return postprocess_masks(low, size, 1024), iou, low


def _figures(got, name):
    gold = S.golden("sam_hq_decoder")
    sample = decoder_sample(*(t.float().cpu() for t in got))
    ref = gold[f"{name}.masks"]
    sure = ref.abs() > 0.1
    agree = float(((sample["masks"] > 0) == (ref > 0))[sure].float().mean())
    return S.rel_err(sample["low_res"], gold[f"{name}.low_res"])[0], S.rel_err(sample["iou"], gold[f"{name}.iou"])[0], agree


@pytest.mark.parametrize("name", list(SAM_HQ_CASES))
def test_predict_bfloat16_stays_with_the_unfused_bfloat16_forward(name):
    bf = torch.bfloat16
    fast, sam, adapter = _fast(bf)
    _f32, sam32, _a32 = _fast(torch.float32)
    case = SAM_HQ_CASES[name]
    adapter.hq_mask_only = case["hq_mask_only"]
    emb, kw = _case_kwargs(name, bf)
    with torch.no_grad():
        stock = _figures(_stock_bf16(sam, sam32, emb, case, kw), name)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = fast.predict(emb, binarize=False, **kw)
    assert got[0].dtype == bf and got[2].dtype == bf and fast.stats["whole_fallback"] is None
    native_ = _figures(got, name)
    print(f"hq bf16 {name}: low_res l2 stock {stock[0]:.4e} native {native_[0]:.4e} | iou l2 stock {stock[1]:.4e} native {native_[1]:.4e} | "
          f"sign agreement stock {100 * stock[2]:.3f} % native {100 * native_[2]:.3f} %")
    assert native_[0] <= BF16_L2_FACTOR * stock[0], ("low_res", native_[0], stock[0])
    assert native_[1] <= BF16_L2_FACTOR * stock[1], ("iou", native_[1], stock[1])
    assert 100 * (1 - native_[2]) <= 100 * (1 - stock[2]) + BF16_SIGN_POINTS, ("sign agreement", native_[2], stock[2])
