"""Cases of the HQ-SAM fixtures (tests/golden/sam_hq_keys.json, sam_hq_decoder.safetensors, written by tools/make_golden_sam_hq.py): a
single-mask SegmentAnythingH with HQSAMAdapter injected, the seeded inputs of tests/sam_decoder_cases.py plus a seeded early ViT embedding."""
from __future__ import annotations

from tests.sam_decoder_cases import SAM_DECODER_CASE, decoder_sample, embedding, low_res_mask  # noqa: F401

SAM_HQ_CASE = dict(weight_seed=SAM_DECODER_CASE["weight_seed"], hq_weight_seed=3, early_seed=23)

#: name -> predict() keywords (+ the adapter's hq_mask_only and the original image size)
SAM_HQ_CASES = {
    "point_sum": dict(hq_mask_only=False, original_size=(1024, 1024), foreground_points=[(500.0, 400.0)]),
    "box_background_hq_only": dict(hq_mask_only=True, original_size=(1024, 1024), background_points=[(700.0, 200.0)], box_points=[[(250.0, 300.0), (800.0, 780.0)]]),
    "mask_prompt": dict(hq_mask_only=False, original_size=(1024, 1024), foreground_points=[(600.0, 600.0)], low_res_mask=True),
    "non_square": dict(hq_mask_only=False, original_size=(600, 900), foreground_points=[(450.0, 250.0), (120.0, 500.0)]),
}


def early_embedding(seed: int = SAM_HQ_CASE["early_seed"]):
    """Context hq_sam.early_vit_embedding: 0.1 * randn(1, 64, 64, 1280) (the ViT does not run)."""
    import torch

    return 0.1 * torch.randn((1, 64, 64, 1280), generator=torch.Generator().manual_seed(seed))


def prompt_kwargs(case: dict) -> dict:
    return {k: case[k] for k in ("foreground_points", "background_points", "box_points") if k in case}


def hq_weights():
    """(synthetic weights of everything but the image encoder, synthetic weights of the adapter), float32 on the CPU."""
    import json
    from pathlib import Path

    from refiners_amd import synth

    gold = Path(__file__).resolve().parent / "golden"
    base = {k: tuple(v) for k, v in json.loads((gold / "sam_h_decoder_keys.json").read_text()).items() if not k.startswith("SAMViTH.")}
    extra = {k: tuple(v) for k, v in json.loads((gold / "sam_hq_keys.json").read_text()).items()}
    return synth.synth_state_dict(base, SAM_HQ_CASE["weight_seed"]), synth.synth_state_dict(extra, SAM_HQ_CASE["hq_weight_seed"])


def hq_sam(device="cpu", dtype=None):
    """The mirror's single-mask SegmentAnythingH (its ViT on "meta": the fixtures never run it) with HQSAMAdapter injected and the
    fixtures' weights loaded -> (sam, adapter)."""
    import torch

    from refiners_amd.segment_anything import HQSAMAdapter, MaskDecoder, SegmentAnythingH

    dtype = dtype or torch.float32
    base, extra = hq_weights()
    sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=False, device="meta"), device="meta")
    sam.load_state_dict({k: v.to(device, dtype) for k, v in base.items()}, strict=False, assign=True)
    adapter = HQSAMAdapter(sam)
    adapter.load_weights({k: v.to(device, dtype) for k, v in extra.items()}, assign=True)
    return sam, adapter.inject()
