"""Recipes of the MultiDiffusion golden cases (tests/golden/multi_diffusion.safetensors and multi_diffusion_tiles.json, written by
tools/make_golden_multi_diffusion.py from the REAL reference's SDXLMultiDiffusion / SD1MultiDiffusion, CPU float32, synthetic weights) and a
torch model of the three kernels (mi355x_md_gather, mi355x_md_target_step, mi355x_md_blend), index arithmetic included.

Everything is rebuilt from seeds: weights (seed 0), canvas and noise (`canvas_inputs`), per-target embeddings, init latents and opacity masks
(`build_targets`).  16 x 16 tiles keep a CPU forward at a few seconds."""
from __future__ import annotations

from typing import Any, Callable, Mapping, Optional, Sequence

import torch
from torch import Tensor

from refiners_amd import synth

STEPS = 30  # inference steps of every solver below

#: generate_latent_tiles recipes recorded into multi_diffusion_tiles.json: (height, width, tile height, tile width, min_overlap).
#: 41 / 16 / 4: four tiles with overlap 7, the last one clamped from 27 to 25; 24 x 27: case a; a tile larger than the image; no overlap at all.
TILE_RECIPES = [(24, 27, 16, 16, 4), (41, 41, 16, 16, 4), (16, 41, 16, 16, 4), (64, 100, 32, 48, 8), (128, 128, 96, 96, 8), (20, 12, 32, 32, 8), (32, 32, 16, 16, 0),
                (33, 50, 16, 24, 7), (16, 16, 16, 16, 4)]


def _t(tile: Sequence[int], **kw: Any) -> dict[str, Any]:
    return dict(dict(tile=tuple(tile), scale=5.0, weight=1, start_step=0, end_step=1000, init=False, mask=None, solver=("ddim", 0)), **kw)


MD_CASES: dict[str, dict[str, Any]] = {
    # generate_latent_tiles(24 x 27, tile 16 x 16, min_overlap 4): tops {0, 8} x lefts {0, 11} -- odd left, odd canvas stride, rows 8..15 x columns 11..15 under all four
    "a": dict(family="sdxl", canvas=(24, 27), steps=[11], input_seed=71, targets=[
        _t((0, 0, 16, 16), scale=5.0), _t((0, 11, 16, 27), scale=7.5, weight=2), _t((8, 0, 24, 16), scale=7.5), _t((8, 11, 24, 27), scale=5.0)]),
    # targets that leave rows 16..23 x columns 0..10 uncovered; a fractional mask with an all-zero block that nothing else covers; init latents noised on the
    # step taken; a target whose window ended; a 24 x 16 target (a second group)
    "b": dict(family="sdxl", canvas=(24, 27), steps=[11], input_seed=72, targets=[
        _t((0, 0, 16, 16), mask="fractional_zero_block"), _t((8, 11, 24, 27), init=True, start_step=11, scale=7.5), _t((4, 5, 20, 21), end_step=10),
        _t((0, 11, 24, 27), scale=7.5)]),
    # DPM-Solver++ 2M, steps 0 and 1 in sequence: the second-order update of step 1 reads each target's own data estimate of step 0
    "c": dict(family="sdxl", canvas=(16, 27), steps=[0, 1], input_seed=73, targets=[
        _t((0, 0, 16, 16), solver=("dpm", 0), scale=5.0), _t((0, 11, 16, 27), solver=("dpm", 0), scale=7.5)]),
    # SD1.5: a DDIM target and a DPM-Solver++ target (first-order on its first inference step) in one call: two timesteps, both update forms
    "d": dict(family="sd1", canvas=(16, 24), steps=[11], input_seed=74, targets=[
        _t((0, 0, 16, 16), scale=7.0), _t((0, 8, 16, 24), solver=("dpm", 11), scale=5.0, weight=3)]),
}


def canvas_inputs(case: Mapping[str, Any]) -> tuple[Tensor, Tensor]:
    h, w = case["canvas"]
    seed = case["input_seed"]
    return torch.randn((1, 4, h, w), generator=synth._gen("md.x", seed)), torch.randn((1, 4, h, w), generator=synth._gen("md.noise", seed))


def opacity_mask(kind: str, h: int, w: int, seed: int, index: int) -> Tensor:
    assert kind == "fractional_zero_block"
    m = torch.rand((1, 1, h, w), generator=synth._gen(f"md.mask{index}", seed)) * 0.9 + 0.1
    m[:, :, 4:10, 3:9] = 0.0
    return m


def build_targets(case: Mapping[str, Any], ns: Any, make_solver: Callable[[str, int], Any], device: Any = None, dtype: Any = None) -> list[Any]:
    """The case's target list out of `ns.Tile`, `ns.SDXLTarget` / `ns.SD1DiffusionTarget` (the mirror's or the reference's own classes) with one
    solver per target from `make_solver(kind, first_inference_step)`."""
    seed, out = case["input_seed"], []
    conv = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
    for i, r in enumerate(case["targets"]):
        top, left, bottom, right = r["tile"]
        h, w = bottom - top, right - left
        width = 2048 if case["family"] == "sdxl" else 768
        kw: dict[str, Any] = dict(tile=ns.Tile(top=top, left=left, bottom=bottom, right=right), solver=make_solver(*r["solver"]), weight=r["weight"],
                                  start_step=r["start_step"], end_step=r["end_step"], condition_scale=r["scale"],
                                  clip_text_embedding=conv(torch.randn((2, 77, width), generator=synth._gen(f"md.text{i}", seed))))
        if r["init"]:
            kw["init_latents"] = conv(torch.randn((1, 4, h, w), generator=synth._gen(f"md.init{i}", seed)))
        if r["mask"] is not None:
            kw["opacity_mask"] = conv(opacity_mask(r["mask"], h, w, seed, i))
        if case["family"] == "sdxl":
            kw["pooled_text_embedding"] = conv(torch.randn((2, 1280), generator=synth._gen(f"md.pooled{i}", seed)))
            kw["time_ids"] = torch.tensor([[1024, 1024, 0, 0, 1024, 1024]]).repeat(2, 1).to(device=device)
            out.append(ns.SDXLTarget(**kw))
        else:
            out.append(ns.SD1DiffusionTarget(**kw))
    return out


def mirror_namespace() -> Any:
    from refiners_amd.latent_diffusion import multi_diffusion as md

    return md


def mirror_solver(kind: str, first: int, device: Any = "cpu", dtype: torch.dtype = torch.float32) -> Any:
    from refiners_amd.latent_diffusion.sampling import DDIM
    from refiners_amd.latent_diffusion.solvers import DPMSolver

    return DDIM(STEPS, first_inference_step=first, device=device, dtype=dtype) if kind == "ddim" else DPMSolver(STEPS, first_inference_step=first, device=device, dtype=dtype)


# ------------------------------------------------------------------------------------------------ torch model of the kernels
def gather_model(canvas: Tensor, noise: Optional[Tensor], init: Optional[Tensor], rows: Sequence[tuple], h: int, w: int) -> tuple[Tensor, Tensor]:
    """mi355x_md_gather: rows = [(kind, top, left, init_row, a, b, s)] -> (view [T, C, h, w], model_in [2T, C, h, w]).  float32 arithmetic, the view is
    rounded to the storage type before it is scaled."""
    _, C, H, W = canvas.shape
    i = torch.arange(C * h * w, device=canvas.device)
    c, y, x = i // (h * w), i % (h * w) // w, i % w
    views = []
    for kind, top, left, init_row, a, b, _s in rows:
        src = (c * H + top + y) * W + left + x
        if kind == 1:
            f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=canvas.device)  # noqa: E731
            v = (f32(a) * init[init_row].reshape(-1).float() + f32(b) * noise.reshape(-1)[src].float()).to(canvas.dtype)
        else:
            v = canvas.reshape(-1)[src]
        views.append(v.view(C, h, w))
    view = torch.stack(views)
    s = torch.tensor([r[6] for r in rows], dtype=torch.float32, device=canvas.device).view(-1, 1, 1, 1)
    scaled = (s * view.float()).to(canvas.dtype)
    return view, torch.cat((scaled, scaled))


def target_step_model(view: Tensor, unet_out: Tensor, hist: Optional[Tensor], coef: Tensor, linear: bool) -> tuple[Tensor, Optional[Tensor]]:
    """mi355x_md_target_step in float64 (the kernel's float32 contracts some products into fused multiply-adds, so the comparison carries a tolerance):
    (stepped, new hist)."""
    T = view.shape[0]
    k = coef.double().view(T, 8, 1, 1, 1)
    x, u, c = view.double(), unet_out[:T].double(), unet_out[T:].double()
    eps = u + k[:, 0] * (c - u)
    if not linear:
        x0 = (x - k[:, 2] * eps) / k[:, 1]
        return (k[:, 3] * x0 + k[:, 4] * eps).to(view.dtype), None
    d = k[:, 1] * x + k[:, 2] * eps
    xn = k[:, 3] * x + k[:, 4] * eps + k[:, 5] * d + k[:, 6] * hist.double()
    return xn.to(view.dtype), d.to(view.dtype)


def blend_model(canvas: Tensor, stepped: Tensor, rows: Sequence[tuple]) -> Tensor:
    """mi355x_md_blend: rows = [(top, left, h, w, weight, stepped_off, mask or None)], `stepped` flat; one (product, sum) per target and element in
    float32, targets in list order, then where(num > 0, cum / num, canvas)."""
    _, C, H, W = canvas.shape
    flat, st = canvas.reshape(-1), stepped.reshape(-1)
    i = torch.arange(C * H * W, device=canvas.device)
    c, y, x = i // (H * W), i % (H * W) // W, i % W
    num = torch.zeros(C * H * W, dtype=torch.float32, device=canvas.device)
    cum = torch.zeros_like(num)
    for top, left, h, w, weight, off, mask in rows:
        ty, tx = y - top, x - left
        inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
        tile_index = torch.where(inside, (c * h + ty) * w + tx, 0)
        wgt = torch.full_like(num, float(weight))
        if mask is not None:
            m = mask.float().expand(1, C, h, w) if mask.dim() == 4 else mask.float().expand(C, h, w)
            wgt = wgt * m.reshape(-1)[tile_index]
        num = torch.where(inside, num + wgt, num)
        cum = torch.where(inside, cum + wgt * st[off + tile_index].float(), cum)
    return torch.where(num > 0, (cum / num).to(canvas.dtype), flat).view(canvas.shape)


def model_call(x: Tensor, noise: Tensor, step: int, targets: Sequence[Any], diffuse: Callable[[Tensor, int, Any], Tensor]) -> Tensor:
    """MultiDiffusion.__call__ expressed through the kernel models: gather per target, `diffuse(view, step, target)` in place of the UNet and the
    solver update, one blend.  With a deterministic `diffuse` it equals the mirror bit for bit in float32."""
    tiles, rows, off = [], [], 0
    for t in targets:
        top, left = t.offset
        h, w = t.size
        if step == t.start_step and t.init_latents is not None:
            i = t.solver._noise_index(step) if hasattr(t.solver, "_noise_index") else t.solver.timesteps[step]
            a, b = float(t.solver.cumulative_scale_factors[i]), float(t.solver.noise_std[i])
            view, _ = gather_model(x, noise, t.init_latents, [(1, top, left, 0, a, b, 1.0)], h, w)
        elif t.start_step <= step <= t.end_step:
            view, _ = gather_model(x, None, None, [(0, top, left, 0, 1.0, 0.0, 1.0)], h, w)
        else:
            continue
        tiles.append(diffuse(view, step, t).reshape(-1))
        rows.append((top, left, h, w, t.weight, off, t.opacity_mask))
        off += tiles[-1].numel()
    if not rows:
        return x.clone()
    return blend_model(x, torch.cat(tiles), rows)
