"""Cases of the stochastic-sampling fixtures (tests/golden/stochastic.safetensors + stochastic.json, written by tools/make_golden_stochastic.py
from the REAL reference's StableDiffusion_1 on CPU float32 with synthetic weights): SDE DPM-Solver++, sigma schedules, Restart sampling.
Seeds, shapes, seeded inputs and the solver builder both the tool (on the reference's classes) and the tests (on the mirror's) go through.
Golden keys of a trajectory case: `<case>.x<s>` the latents after step s, `<case>.eps<s>` the (guided) noise prediction the solver was given,
`<case>.noise<s>` the solver's draw of that step (SDE cases).  `restart`: `restart.x<s>` the DDIM trajectory, then per iteration k
`restart.r<k>.noise`, `restart.r<k>.noised` (after add_noise_interval) and `restart.r<k>.x<s>` after every inner step.  The JSON holds every
case's timesteps and the `timesteps` / `sigmas` tables of the reference's DPMSolver for TABLE_STEPS x TABLE_SCHEDULES."""
from __future__ import annotations

from typing import Any

SEED = dict(weight_seed=0, input_seed=83)
TOKENS = 77
#: the smallest set that reaches every branch: first / second order, a first-order last step, a late first step, guided / guidance-free, a schedule
#: with and without the draw, and latents that are (16 x 16, 12 x 20: bfloat16 vectors) or are not (3 x 4 x 6 x 10, 5 x 7) whole 16-byte vectors
CASES: dict[str, dict[str, Any]] = {
    "sde": dict(kind="dpm", steps=6, first=0, last_first_order=False, sde=True, schedule=None, cfg=True, scale=7.5, n=1, hw=(16, 16), noise_seed=1301),
    "sde_free": dict(kind="dpm", steps=6, first=2, last_first_order=True, sde=True, schedule=None, cfg=False, scale=7.5, n=3, hw=(6, 10), noise_seed=1302),
    "karras": dict(kind="dpm", steps=6, first=0, last_first_order=False, sde=False, schedule="karras", cfg=True, scale=7.5, n=1, hw=(12, 20), noise_seed=1303),
    "sde_karras": dict(kind="dpm", steps=6, first=0, last_first_order=False, sde=True, schedule="karras", cfg=False, scale=7.5, n=1, hw=(5, 7), noise_seed=1304),
    # the same three on latents the SD1.5 UNet's three halvings divide (the lowering takes exact 2x upsampling only: the geometries above reach the
    # engine's stock-forward path, these its lowered program and captured graph)
    "sde_free_8x16": dict(kind="dpm", steps=6, first=2, last_first_order=True, sde=True, schedule=None, cfg=False, scale=7.5, n=3, hw=(8, 16), noise_seed=1306),
    "karras_8x24": dict(kind="dpm", steps=6, first=0, last_first_order=False, sde=False, schedule="karras", cfg=True, scale=7.5, n=1, hw=(8, 24), noise_seed=1307),
    "sde_karras_8x8": dict(kind="dpm", steps=6, first=0, last_first_order=False, sde=True, schedule="karras", cfg=False, scale=7.5, n=1, hw=(8, 8), noise_seed=1308),
    "restart": dict(kind="restart", steps=10, first=0, num_steps=4, num_iterations=2, cfg=True, scale=7.5, n=1, hw=(16, 16), noise_seed=1305),
}
TRAJECTORIES = [k for k, c in CASES.items() if c["kind"] == "dpm"]
TABLE_STEPS = (2, 6, 18)
TABLE_SCHEDULES = (None, "uniform", "quadratic", "karras")


def _gen(what: str):
    from refiners_amd import synth

    return synth._gen(what, SEED["input_seed"])


def inputs(name: str) -> dict:
    """Latents and the text stack ([negative ; conditional] when guided) of a case; rows differ."""
    import torch

    case = CASES[name]
    (h, w), n = case["hw"], case["n"]
    return {"x": torch.randn((n, 4, h, w), generator=_gen(f"{name}.x")),
            "text": torch.randn(((2 if case["cfg"] else 1) * n, TOKENS, 768), generator=_gen(f"{name}.text"))}


def make_solver(name: str, api: Any) -> Any:
    """`api`: `DDIM(steps)` and `dpm(steps, first, last_first_order, sde, schedule)` of the reference or of the mirror."""
    case = CASES[name]
    if case["kind"] == "restart":
        return api.DDIM(case["steps"])
    return api.dpm(case["steps"], case["first"], case["last_first_order"], case["sde"], case["schedule"])


def generator(name: str):
    """The stream the reference run drew from: `torch.manual_seed(noise_seed)` on the default CPU generator gives the same numbers."""
    import torch

    return torch.Generator().manual_seed(CASES[name]["noise_seed"])


def lowered(name: str) -> bool:
    """Whether CompiledSDXL lowers the SD1.5 UNet at the case's latents: three stride-2 convolutions down, exact 2x nearest upsampling back up."""
    return all(v % 8 == 0 for v in CASES[name]["hw"])


def run_steps(name: str) -> range:
    case = CASES[name]
    return range(case["first"], case["steps"])
