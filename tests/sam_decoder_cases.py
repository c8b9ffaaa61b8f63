"""Cases of the SAM mask-decoder fixtures (tests/golden/sam_h_decoder*.{json,safetensors}, written by tools/make_golden_sam_decoder.py):
the prompts, the seeded inputs and what of each output is stored."""
from __future__ import annotations

SAM_DECODER_CASE = dict(weight_seed=0, embedding_seed=21, mask_seed=22)

#: name -> predict() keywords (+ the decoder's multimask_output and the original image size)
SAM_DECODER_CASES = {
    "point_multimask": dict(multimask=True, original_size=(1024, 1024), foreground_points=[(500.0, 400.0)]),
    "points_box_single": dict(multimask=False, original_size=(1024, 1024), foreground_points=[(320.0, 610.0)], background_points=[(700.0, 200.0)],
                              box_points=[[(250.0, 300.0), (800.0, 780.0)]]),
    "mask_prompt": dict(multimask=True, original_size=(1024, 1024), foreground_points=[(600.0, 600.0)], low_res_mask=True),
    "non_square": dict(multimask=True, original_size=(600, 900), foreground_points=[(450.0, 250.0), (120.0, 500.0)]),
}


def embedding(seed: int = SAM_DECODER_CASE["embedding_seed"]):
    """The decoder input: a seeded [1, 256, 64, 64] image embedding (the ViT does not run)."""
    import torch

    return torch.randn((1, 256, 64, 64), generator=torch.Generator().manual_seed(seed))


def low_res_mask(seed: int = SAM_DECODER_CASE["mask_seed"]):
    """The mask prompt of case "mask_prompt": smooth [1, 1, 256, 256] logits."""
    import torch
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(seed)
    return 4 * F.interpolate(torch.randn((1, 1, 16, 16), generator=g), size=(256, 256), mode="bilinear")


def decoder_sample(masks, iou, low_res):
    """What the fixture stores of one predict(binarize=False): iou in full, strided samples of the two mask tensors, statistics."""
    import torch

    stats = torch.tensor([low_res.mean(), low_res.abs().mean(), low_res.std(), masks.mean(), masks.abs().mean(), (masks > 0).double().mean()], dtype=torch.float64)
    return {"iou": iou.float().clone(), "low_res": low_res[..., ::4, ::4].float().clone(), "masks": masks[..., ::16, ::16].float().clone(), "stats": stats.float()}
