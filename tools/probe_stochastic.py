"""What the SDE form of DPM-Solver++ costs per step: SD1.5 at 512 x 512 (64 x 64 latents), classifier-free-guidance pair, bfloat16, 77 CLIP
tokens, DPMSolver(30), synthetic weights (refiners_amd.synth).  In ONE process, on one UNet:
    ode_step          CompiledSDXL.step under the deterministic solver: one HIP-graph replay whose last launch is mi355x_cfg_linear_step
    sde_step_device   the same under DPMSolver(sde_variance=1.0), the draw from a generator on the GPU: torch.randn + copy into the engine's buffer, then
                      the replay, whose last launch is mi355x_cfg_sde_step
    sde_step_cpu      the same with a CPU generator (the draw is made on the host and copied over: what pins a trajectory to a CPU recording)
the three alternating, three repeats each, every path warmed first; times are a host clock around work that ends in a device synchronise; the
spread of the repeats is written beside every median.  Then the two parts the SDE step adds, on their own:
    draw_device / draw_cpu     CompiledSDXL._draw (randn of the latents' shape and dtype + copy_ into the resident buffer)
    update_sde / update_ode    mi355x_cfg_sde_step / mi355x_cfg_linear_step on the step's operands, back to back (launch-bound at 16 K elements)
Needs a GPU (no fallback).
    python tools/probe_stochastic.py --json profiles/stochastic_probe.json"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import native, synth  # noqa: E402
from refiners_amd.engine.compiled import CompiledSDXL  # noqa: E402
from refiners_amd.latent_diffusion.sd1 import SD1UNet  # noqa: E402
from refiners_amd.latent_diffusion.solvers import DPMSolver  # noqa: E402


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_stochastic needs a GPU"
    dev, dt, L, steps = torch.device("cuda"), torch.bfloat16, a.latent, 30
    g = torch.Generator().manual_seed(1)
    unet = SD1UNet(4, device="meta")
    unet.load_state_dict({k: v.to(device=dev, dtype=dt) for k, v in synth.synth_state_dict(synth.model_shapes(unet), 0).items()}, assign=True)
    x = torch.randn((1, 4, L, L), generator=g).to(dev, dt)
    clip = torch.randn((2, 77, 768), generator=g).to(dev, dt)
    ode = CompiledSDXL(unet, solver=DPMSolver(steps), condition_scale=7.5)
    sde_d = CompiledSDXL(unet, solver=DPMSolver(steps, sde_variance=1.0), condition_scale=7.5)
    sde_c = CompiledSDXL(unet, solver=DPMSolver(steps, sde_variance=1.0), condition_scale=7.5)
    ode.set_inputs(x, clip_text_embedding=clip)
    sde_d.set_inputs(x, clip_text_embedding=clip, generator=torch.Generator(device=dev).manual_seed(2))
    sde_c.set_inputs(x, clip_text_embedding=clip, generator=torch.Generator().manual_seed(2))
    paths = (ode, sde_d, sde_c)
    for p in paths:
        p.step(0)
        assert p.engine.stats["fallback_nodes"] == [], "the native path did not run"
    for _ in range(3):  # warm every path: the second step captures the graph
        for p in paths:
            p.step(3)
    assert all(p.graph is not None for p in paths)
    runs = [tuple(timeit(lambda p=p: p.step(3), a.iters) for p in paths) for _ in range(3)]
    med = lambda r, i: sorted(v[i] for v in r)[1]  # noqa: E731
    span = lambda r, i: [round(min(v[i] for v in r), 4), round(max(v[i] for v in r), 4)]  # noqa: E731

    # the parts, on their own
    io = sde_d.engine.io
    n_part = 10 * a.iters
    parts = [(timeit(lambda: sde_d._draw(sde_d.generator), n_part), timeit(lambda: sde_c._draw(sde_c.generator), n_part),
              timeit(lambda: native.cfg_sde_step(sde_d.x, io.out, sde_d.hist, sde_d.sde_noise, io.x, sde_d.coef), n_part),
              timeit(lambda: native.cfg_linear_step(ode.x, ode.engine.io.out, ode.hist, ode.engine.io.x, ode.coef), n_part)) for _ in range(3)]
    res = {
        "device": torch.cuda.get_device_name(0), "shape": {"images": 1, "cfg_pair": True, "latent": L, "clip_tokens": 77, "dtype": "bfloat16", "solver": f"DPMSolver({steps})"},
        "iters": a.iters, "part_iters": n_part,
        "ode_step_ms": round(med(runs, 0), 4), "ode_step_ms_min_max": span(runs, 0),
        "sde_step_device_generator_ms": round(med(runs, 1), 4), "sde_step_device_generator_ms_min_max": span(runs, 1),
        "sde_step_cpu_generator_ms": round(med(runs, 2), 4), "sde_step_cpu_generator_ms_min_max": span(runs, 2),
        "sde_over_ode_device_generator": round(med(runs, 1) / med(runs, 0), 4), "sde_over_ode_cpu_generator": round(med(runs, 2) / med(runs, 0), 4),
        "step_launches": {"ode": ode.engine.stats["step_ops"] + 1, "sde": sde_d.engine.stats["step_ops"] + 1},  # (+ the solver update)
        "draw_device_generator_ms": round(med(parts, 0), 4), "draw_device_generator_ms_min_max": span(parts, 0),
        "draw_cpu_generator_ms": round(med(parts, 1), 4), "draw_cpu_generator_ms_min_max": span(parts, 1),
        "update_sde_ms": round(med(parts, 2), 4), "update_sde_ms_min_max": span(parts, 2),
        "update_ode_ms": round(med(parts, 3), 4), "update_ode_ms_min_max": span(parts, 3),
    }
    print(json.dumps(res, indent=1))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
