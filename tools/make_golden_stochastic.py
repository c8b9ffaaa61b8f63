"""Golden vectors of stochastic sampling: the REAL reference's StableDiffusion_1 (SD1UNet(4), synthetic weights, CPU float32, Identity chains for
the autoencoder and the text encoder) under DPM-Solver++ with `SolverParams(sde_variance=1.0)` and / or `sigma_schedule=...`, and a DDIM trajectory
followed by `Restart`, per case of tests/stochastic_cases.py:
    <case>.x<s>  <case>.eps<s>  <case>.noise<s>      latents after step s, the noise prediction the solver got, the solver's draw (SDE cases)
    restart.x<s>; restart.r<k>.noise / .noised / .x<s>   the DDIM trajectory; per Restart iteration the draw, the re-noised latents, every inner step
and tests/golden/stochastic.json: every case's timesteps, Restart's timesteps, and the reference DPMSolver's `timesteps` / `sigmas` tables for
2, 6 and 18 steps under every sigma schedule.  Only the reference's OUTPUTS are stored.  Run where refiners' sources are, not on a GPU box:
    python tools/make_golden_stochastic.py
-> tests/golden/stochastic.safetensors, tests/golden/stochastic.json"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

from oracle.make_golden import reference_model  # noqa: E402  (puts the reference package and the jaxtyping shim on sys.path)

import refiners.fluxion.layers as rfl  # noqa: E402
from refiners.foundationals.latent_diffusion.restart import Restart, add_noise_interval  # noqa: E402
from refiners.foundationals.latent_diffusion.solvers import DDIM, DPMSolver, NoiseSchedule, SolverParams  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.model import StableDiffusion_1  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet  # noqa: E402

from refiners_amd import synth  # noqa: E402
from tests import stochastic_cases as SC  # noqa: E402

GOLD = ROOT / "tests" / "golden"
NOTHING = lambda: rfl.Chain(rfl.Identity())  # noqa: E731


def ref_dpm(steps: int, first: int = 0, last_first_order: bool = False, sde: bool = False, schedule: str | None = None) -> DPMSolver:
    params = SolverParams(sde_variance=1.0 if sde else 0.0, sigma_schedule=None if schedule is None else NoiseSchedule(schedule))
    return DPMSolver(steps, first_inference_step=first, params=params, last_step_first_order=last_first_order)


API = SimpleNamespace(DDIM=DDIM, dpm=ref_dpm)


def main() -> None:
    shapes4 = synth.model_shapes(SD1UNet(4, device="meta"))
    assert {k: list(v) for k, v in shapes4.items()} == json.loads((GOLD / "sd1_unet_keys.json").read_text())
    unet = reference_model(SD1UNet, shapes4, SC.SEED["weight_seed"])
    out: dict[str, torch.Tensor] = {}
    meta: dict = {"timesteps": {}, "tables": {}}
    with torch.no_grad():
        for name, case in SC.CASES.items():
            t0 = time.time()
            sd = StableDiffusion_1(unet=unet, lda=NOTHING(), clip_text_encoder=NOTHING(), solver=SC.make_solver(name, API))  # type: ignore[arg-type]
            sd.classifier_free_guidance = case["cfg"]
            meta["timesteps"][name] = [int(t) for t in sd.solver.timesteps]
            inp = SC.inputs(name)
            kw = dict(clip_text_embedding=inp["text"], condition_scale=case["scale"])
            seen: list[torch.Tensor] = []
            hook = unet.register_forward_hook(lambda _m, _a, y: seen.append(y.detach().clone()))
            x = inp["x"]
            if case.get("sde"):
                g = SC.generator(name)
                for s in SC.run_steps(name):
                    out[f"{name}.noise{s}"] = torch.randn(x.shape, generator=g)
            torch.manual_seed(case["noise_seed"])  # the reference's forward hands the solver no generator: it draws from the default one
            for s in SC.run_steps(name):
                x = sd(x, step=s, **kw).contiguous()
                out[f"{name}.x{s}"] = x
                y = seen[-1]
                if case["cfg"]:  # latent_diffusion/model.py: unconditional + scale * (conditional - unconditional)
                    u, c = y.chunk(2)
                    y = u + case["scale"] * (c - u)
                out[f"{name}.eps{s}"] = y.contiguous()
            hook.remove()
            if case["kind"] == "restart":
                restart = Restart(ldm=sd, num_steps=case["num_steps"], num_iterations=case["num_iterations"])
                ts = restart.timesteps
                meta["restart"] = {"timesteps": [int(t) for t in ts], "start_step": restart.start_step, "end_timestep": restart.end_timestep}
                g = SC.generator(name)
                inner: list[torch.Tensor] = []
                hook = sd.register_forward_hook(lambda _m, _a, y: inner.append(y.detach().clone().contiguous()))
                torch.manual_seed(case["noise_seed"])
                final = restart(x, **kw)
                hook.remove()
                per = len(ts) - 1
                assert len(inner) == per * case["num_iterations"] and torch.equal(final, inner[-1])
                start = x
                for k in range(case["num_iterations"]):
                    noise = torch.randn(x.shape, generator=g)
                    out[f"{name}.r{k}.noise"] = noise
                    out[f"{name}.r{k}.noised"] = add_noise_interval(DDIM(case["steps"]), x=start, noise=noise, initial_timestep=ts[-1], target_timestep=ts[0]).contiguous()
                    for s in range(per):
                        out[f"{name}.r{k}.x{s}"] = inner[k * per + s]
                    start = inner[k * per + per - 1]
            print(name, tuple(x.shape), [f"{float(out[f'{name}.x{s}'].std()):.3f}" for s in SC.run_steps(name)], f"{time.time() - t0:.1f}s", flush=True)
    for n in SC.TABLE_STEPS:
        for schedule in SC.TABLE_SCHEDULES:
            solver = ref_dpm(n, schedule=schedule)
            meta["tables"][f"{n}.{schedule}"] = {"timesteps": [int(t) for t in solver.timesteps], "sigmas": [float(v) for v in solver.sigmas.double()]}
    save_file(out, str(GOLD / "stochastic.safetensors"))
    (GOLD / "stochastic.json").write_text(json.dumps(meta, indent=1) + "\n")
    print((GOLD / "stochastic.safetensors").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
