"""Cases of the Swin Transformer fixtures (tests/golden/swin_keys.json, swin.safetensors and its shards, written by
tools/make_golden_swin.py from the reference's own classes): model configurations, the synthetic weight draw, seeded inputs and
what the fixture keeps of every output."""
from __future__ import annotations

import json
from functools import lru_cache
from pathlib import Path

SWIN_SEED = dict(weight_seed=11, input_seed=29)

#: name -> model keywords + input geometry.  Every stage of every case has at least 2 windows per side (the reference raises on a
#: shifted stage of one window).  Grid sides -> windows:  A 48 -> 4x4, 24 -> 2x2 (no padding);  B 50 -> pad 60, 5x5; 25 -> pad 36, 3x3;
#: 13 -> pad 24, 2x2 (padding at every stage, both merges on odd grids);  C 28 -> 4x4, 14 -> 2x2 with ws 7 (49 tokens per window);
#: D Swin-B's widths: 104 -> pad 108, 9x9; 52 -> pad 60, 5x5; 26 -> pad 36, 3x3; 13 -> pad 24, 2x2.
SWIN_CASES = {
    "A": dict(model=dict(embedding_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=12), batch=2, side=192),
    "B": dict(model=dict(embedding_dim=64, depths=[2, 2, 2], num_heads=[2, 4, 8], window_size=12), batch=2, side=200),
    "C": dict(model=dict(embedding_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=7), batch=1, side=112),
    "D": dict(model=dict(embedding_dim=128, depths=[2, 2, 2, 2], num_heads=[4, 8, 16, 32], window_size=12), batch=1, side=416),
}
KEEP_WHOLE = 32 * 1024  # outputs of at most this many elements are stored whole


def output_names(case: str) -> list[str]:
    """Names of the forward's outputs in the order it returns them: stage_n, ..., stage_1, patch_embedding."""
    n = len(SWIN_CASES[case]["model"]["depths"])
    return [f"stage_{i}" for i in range(n, 0, -1)] + ["patch_embedding"]


def image(case: str):
    import torch

    c = SWIN_CASES[case]
    g = torch.Generator().manual_seed(SWIN_SEED["input_seed"] + sum(map(ord, case)))
    return torch.randn((c["batch"], 3, c["side"], c["side"]), generator=g)


@lru_cache(maxsize=None)
def key_shapes(case: str) -> dict[str, tuple[int, ...]]:
    gold = Path(__file__).resolve().parent / "golden"
    return {k: tuple(v) for k, v in json.loads((gold / "swin_keys.json").read_text())[case].items()}


def draw_weights(shapes: dict, case: str) -> dict:
    """synth.synth_state_dict over the key / shape list, with two exceptions: every relative_position_index is the canonical index, and
    the bias tables are drawn with standard deviation 0.5 (the default draw, 1 / sqrt(heads), would leave the bias a small correction)."""
    from refiners_amd import synth
    from refiners_amd.swin import canonical_relative_position_index

    seed = SWIN_SEED["weight_seed"]
    sd = synth.synth_state_dict(shapes, seed)
    for k, s in shapes.items():
        if k.endswith("relative_position_index"):
            sd[k] = canonical_relative_position_index(SWIN_CASES[case]["model"]["window_size"])
            assert tuple(sd[k].shape) == tuple(s)
        elif k.endswith("relative_position_bias_table"):
            sd[k] = synth.synth_tensor(k, s, seed, gain=0.5 * s[1] ** 0.5)
    return sd


def weights(case: str) -> dict:
    return draw_weights(key_shapes(case), case)


def mirror(case: str, device="cpu", dtype=None, **overrides):
    """The mirror's SwinTransformer of a case with the fixture's weights loaded."""
    import torch

    from refiners_amd.swin import SwinTransformer

    dtype = dtype or torch.float32
    model = SwinTransformer(**{**SWIN_CASES[case]["model"], **overrides}, device="meta")
    # (a variant of the case -- other head counts, say -- has no fixture: its weights are drawn over its own key / shape list)
    drawn = draw_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}, case) if overrides else weights(case)
    sd = {k: v.to(device=device, dtype=dtype if v.is_floating_point() else None) for k, v in drawn.items()}
    model.load_state_dict(sd, assign=True)
    return model


def sample_stride(shape) -> int:
    """Spatial stride of the stored sample of a (B, C, H, W) output: 1 (whole) up to KEEP_WHOLE elements, else the smallest that fits."""
    b, c, h, w = shape
    s = 1
    while b * c * -(-h // s) * -(-w // s) > KEEP_WHOLE:
        s += 1
    return s


def output_sample(y) -> dict:
    """What the fixture stores of one (B, C, H, W) output: the tensor itself when small; else a strided sample plus the per-channel
    mean and mean-abs, which see every element."""
    s = sample_stride(y.shape)
    y = y.detach().float().cpu()
    out = {"sample": y[..., ::s, ::s].contiguous()}
    if s > 1:
        out["mean"] = y.double().mean(dim=(2, 3)).float()
        out["meanabs"] = y.double().abs().mean(dim=(2, 3)).float()
    return out
