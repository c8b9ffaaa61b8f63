"""HQ-SAM mask prediction without a GPU: the mirror's HQSAMAdapter against the real reference (tests/golden/sam_hq_*, written by
tools/make_golden_sam_hq.py), a float64 model of the folded mask head's arithmetic and indexing (csrc/sam_hq.hip), and dry lowerings of the
adapted mask decoder on the meta device."""
import json
import os
import sys
from collections import Counter
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from refiners_amd.engine.sam_hq import HQSAMDecoderLowering
from refiners_amd.segment_anything import HQSAMAdapter, ImageEmbedding, MaskDecoder, SegmentAnythingH
from tests import support as S
from tests.sam_hq_cases import SAM_HQ_CASES, decoder_sample, early_embedding, embedding, hq_sam, low_res_mask, prompt_kwargs

TOL = 2e-4  # the bound of tests/test_sam_decoder_cpu.py: the same float32 torch arithmetic on both sides
ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")


def test_mirror_keys_equal_the_reference():
    shapes = {k: tuple(v) for k, v in json.loads((S.GOLD / "sam_hq_keys.json").read_text()).items()}
    adapter = HQSAMAdapter(SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=False, device="meta"), device="meta"))
    assert list(adapter.weights) == list(shapes)
    assert {k: tuple(v.shape) for k, v in adapter.weights.items()} == shapes
    assert all(k.startswith(("Chain.HQSAMMaskPrediction.", "MaskDecoderTokensExtender.hq_token.")) for k in shapes)


@pytest.fixture(scope="module")
def adapted():
    return hq_sam()


@pytest.mark.parametrize("name", list(SAM_HQ_CASES))
def test_mirror_predict_matches_reference(adapted, name):
    sam, adapter = adapted
    case = SAM_HQ_CASES[name]
    adapter.hq_mask_only = case["hq_mask_only"]
    adapter.set_context("hq_sam", {"early_vit_embedding": early_embedding()})
    kw = prompt_kwargs(case)
    if case.get("low_res_mask"):
        kw["low_res_mask"] = low_res_mask()
    masks, iou, low = sam.predict(ImageEmbedding(embedding(), case["original_size"]), binarize=False, **kw)
    assert masks.shape == (1, 1, *case["original_size"]) and low.shape == (1, 1, 256, 256) and iou.shape == (1, 1)
    gold = S.golden("sam_hq_decoder")
    for k, v in decoder_sample(masks, iou, low).items():
        l2, mx = S.rel_err(v, gold[f"{name}.{k}"])
        assert l2 <= TOL and mx <= TOL, (name, k, l2, mx)


def test_inject_eject_round_trip_and_multimask_refusal():
    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=False, device="meta"), device="meta")
    before = [type(m).__name__ for m in sam.modules()]
    keys = list(sam.state_dict())
    adapter = HQSAMAdapter(sam, hq_mask_only=True)
    assert [type(m).__name__ for m in sam.modules()] == before  # nothing changes before inject()
    adapter.inject()
    assert [type(c).__name__ for c in sam.mask_decoder] == ["MaskDecoderTokensExtender", "EmbeddingsAggregator", "Transformer", "Predictions", "PredictionsPostProc"]
    assert type(sam[0]).__name__ == "SAMViTAdapter" and sam.parent is adapter and adapter.hq_mask_only is True
    adapter.hq_mask_only = False
    assert adapter.predictions_post_proc.hq_mask_only is False
    adapter.eject()
    assert [type(m).__name__ for m in sam.modules()] == before and list(sam.state_dict()) == keys and sam.parent is None
    with pytest.raises(NotImplementedError, match="Multi-mask"):
        HQSAMAdapter(SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=True, device="meta"), device="meta"))


def test_two_adapters_keep_their_own_weights():
    a, b = (HQSAMAdapter(SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=False, device="meta"), device="meta")) for _ in range(2))
    key = "MaskDecoderTokensExtender.hq_token"
    assert a._adapter_modules[key] is a.mask_decoder_tokens_extender.hq_token and b._adapter_modules[key] is b.mask_decoder_tokens_extender.hq_token
    assert a._adapter_modules[key] is not b._adapter_modules[key] and list(a.weights) == list(b.weights)


# ------------------------------------------------------------------------------------------------ the ABI extension
def test_sam_hq_header_is_bound_and_exported():
    """Two prototypes of the HQ-SAM header written out by hand (its names, layouts and exports: tests/test_abi_header_cpu.py)."""
    import ctypes as C

    from refiners_amd import native
    from refiners_amd.build_native import build_native

    build_native()
    lib = native.load()
    assert lib.mi355x_sam_hq_mask_head.argtypes == [C.POINTER(native.SamHqMaskHeadArgs), C.c_void_p] and len(lib.mi355x_ln2d_gelu_wide.argtypes) == 13


# ------------------------------------------------------------------------------------------------ the fold
def test_folded_mask_head_model():
    """mi355x_sam_hq_mask_head in float64: weff[p] = sum_c h[p, c] W2[c], a 64 -> 1 convolution of z with zero-padded borders, and
    h . (F + b2) with F read through the quadrant index formula == conv2d(z, padding=1) + F contracted with h."""
    g = torch.Generator().manual_seed(5)
    P, H, W = 3, 6, 10
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    z, w2, b2, h, f = r(P, H, W, 64), r(32, 64, 3, 3), r(32), r(P, 32), r(H, W, 32)
    ref = torch.einsum("pc,pchw->phw", h, F.conv2d(z.permute(0, 3, 1, 2), w2, b2, padding=1) + f.permute(2, 0, 1))
    fq = torch.zeros((H // 2) * (W // 2), 128, dtype=torch.float64)
    for y in range(H):
        for x in range(W):
            fq[(y >> 1) * (W // 2) + (x >> 1), ((y & 1) * 2 + (x & 1)) * 32 : ((y & 1) * 2 + (x & 1)) * 32 + 32] = f[y, x]
    w2p = w2.permute(0, 2, 3, 1).reshape(32, 9, 64)  # what the lowering packs: [c][3 ky + kx][ci]
    weff = torch.einsum("pc,ctk->ptk", h, w2p)
    hb = h @ b2
    out = torch.zeros(P, H, W, dtype=torch.float64)
    for p in range(P):
        for y in range(H):
            for x in range(W):
                acc = 0.0
                for tap in range(9):
                    yy, xx = y + tap // 3 - 1, x + tap % 3 - 1
                    if 0 <= yy < H and 0 <= xx < W:  # outside: z = 0
                        acc += float(weff[p, tap] @ z[p, yy, xx])
                row, col = (y >> 1) * (W // 2) + (x >> 1), ((y & 1) * 2 + (x & 1)) * 32
                out[p, y, x] = acc + float(h[p] @ fq[row, col : col + 32]) + float(hb[p])
    torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ dry lowering
def _dry(sam, P, T, has_mask, dtype):
    low = HQSAMDecoderLowering(torch.device("meta"), dtype)
    low.lower(sam, P, T, has_mask, torch.empty(4096, 256, device="meta"))
    return low


#: launches of one program of the adapted single-mask decoder: has_mask -> kinds.  Against the plain decoder (tests/test_sam_decoder_cpu.py,
#: 30 / 33 GEMMs): + 2 first transposed convolutions + 1 two-segment second one + 3 of the HQ token's MLP, + 1 convt2x2_ln_gelu
HQ_EXPECTED = {
    False: {"mi355x_gemm": 36, "mi355x_layernorm": 9, "mi355x_sam_attention": 7, "mi355x_nchw_to_nhwc": 1, "mi355x_axpby": 1, "mi355x_gather_rows": 1,
            "mi355x_convt2x2_ln_gelu": 2, "mi355x_sam_mask_head_up": 1, "mi355x_ln2d_gelu_wide": 1, "mi355x_gemm(conv)": 1, "mi355x_sam_hq_mask_head": 1},
    True: {"mi355x_gemm": 39, "mi355x_layernorm": 9, "mi355x_sam_attention": 7, "mi355x_nchw_to_nhwc": 1, "mi355x_patchify_nchw": 1, "mi355x_gather_rows": 1,
           "mi355x_convt2x2_ln_gelu": 4, "mi355x_sam_mask_head_up": 1, "mi355x_ln2d_gelu_wide": 1, "mi355x_gemm(conv)": 1, "mi355x_sam_hq_mask_head": 1},
}


def _check_program(low, has_mask):
    kinds = Counter(e[2] for e in low.step)
    assert dict(kinds) == HQ_EXPECTED[has_mask]
    assert kinds["mi355x_sam_hq_mask_head"] == kinds["mi355x_sam_mask_head_up"] == kinds["mi355x_ln2d_gelu_wide"] == 1 and "mi355x_sam_mask_head" not in kinds
    assert low.stats["fallback_nodes"] == []
    assert not [e[2] for e in low.step if e[0] is None or str(e[2]).startswith("torch:")]


def _mirror(dtype):
    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=False, device="meta", dtype=dtype), device="meta", dtype=dtype)
    HQSAMAdapter(sam).inject()
    return sam


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P,T,has_mask", [(1, 8, False), (16, 9, True)])
def test_hq_decoder_lowers_without_fallback(dtype, P, T, has_mask):
    low = _dry(_mirror(dtype), P, T, has_mask, dtype)
    _check_program(low, has_mask)
    kinds = low.stats["attention_kinds"]
    assert kinds.count(f"h8xd32 Lq={T} Lk={T}") == 2 and kinds.count(f"h8xd16 Lq={T} Lk=4096") == 3 and kinds.count(f"h8xd16 Lq=4096 Lk={T}") == 2


def test_plain_tree_lowers_as_the_base_class_does():
    from refiners_amd.engine.sam_decoder import SAMDecoderLowering

    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=True, device="meta"), device="meta")
    base = SAMDecoderLowering(torch.device("meta"), torch.float32)
    io = base.lower(sam, 4, 7, False, torch.empty(4096, 256, device="meta"))
    mine = _dry(sam, 4, 7, False, torch.float32)
    assert [e[2] for e in mine.step] == [e[2] for e in base.step] and "early" not in io


def test_hq_lowering_accepts_the_real_refiners_tree():
    if not (REF / "refiners").exists():
        pytest.skip("no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
    sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF)]
    from refiners.foundationals.segment_anything import hq_sam as rh
    from refiners.foundationals.segment_anything import image_encoder as ie
    from refiners.foundationals.segment_anything import mask_decoder as md
    from refiners.foundationals.segment_anything import model as mo
    from refiners.foundationals.segment_anything import prompt_encoder as pe

    kw = dict(device="meta", dtype=torch.bfloat16)
    sam = mo.SegmentAnything(ie.SAMViTH(**kw), pe.PointEncoder(**kw), pe.MaskEncoder(**kw), md.MaskDecoder(multimask_output=False, **kw), **kw)
    rh.HQSAMAdapter(sam, weights=None).inject()
    for P, T, has_mask in ((1, 8, False), (16, 9, True)):
        low = _dry(sam, P, T, has_mask, torch.bfloat16)
        _check_program(low, has_mask)
        assert [e[2] for e in low.step] == [e[2] for e in _dry(_mirror(torch.bfloat16), P, T, has_mask, torch.bfloat16).step]
