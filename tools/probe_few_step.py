"""Few-step SDXL at 1024 x 1024 (128 x 128 latents) in bf16 with `SDXLLcmAdapter` injected and a rank-64 LCM-shaped LoRA live (every layer an
LCM-LoRA file adapts, tests/few_step_cases.lcm_lora_targets), LCMSolver(4), `CompiledSDXL(classifier_free_guidance=False)`:
  * steps       the guidance-free step in ms at n = 1, 2 and 4 images, and the GUIDED step of the same tree (n = 1) in the same process,
  * trajectory  a whole 4-step trajectory at n = 1 -- set_inputs with a NEW prompt (so the prologue runs), 4 steps, the host waiting for the result.
Random weights drawn on the GPU (times do not depend on the values).  Every part runs in a child process of its own under its own time limit,
one after the other, and a part that fails ends the run:  `python tools/probe_few_step.py [--json FILE]`"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PARTS = {"steps": 420, "trajectory": 300}  # part -> its time limit in seconds
HW, RANK, STEPS = (128, 128), 64, 4


def build():
    import torch

    from refiners_amd import native
    from refiners_amd.engine.compiled import CompiledSDXL
    from refiners_amd.latent_diffusion.adapters import SDLoraManager
    from refiners_amd.latent_diffusion.lcm import SDXLLcmAdapter, add_lcm_lora
    from refiners_amd.latent_diffusion.sdxl import SDXLUNet
    from refiners_amd.latent_diffusion.solvers import LCMSolver
    from tests.few_step_cases import lcm_lora_targets

    native.load()
    dev, dt = torch.device("cuda"), torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)

    def draw(shape, gain=1.0):
        fan_in = 1
        for d in shape[1:]:
            fan_in *= d
        return (torch.randn(tuple(shape), device=dev, generator=g) * (gain / max(fan_in, 1) ** 0.5)).to(dt)

    unet = SDXLUNet(4, device="meta")
    shapes = {k: tuple(v.shape) for k, v in unet.state_dict().items()}
    sd = {}
    for k, s in shapes.items():
        norm = "Norm" in k.split(".")[-2]
        sd[k] = (torch.ones(s, device=dev, dtype=dt) if norm and k.endswith("weight") else torch.zeros(s, device=dev, dtype=dt) if len(s) < 2 else draw(s))
    unet.load_state_dict(sd, assign=True)
    tensors = {}
    for key, w in lcm_lora_targets(shapes):
        tensors[f"lora_unet_{key}.lora_down.weight"] = draw((RANK, *w[1:]))
        tensors[f"lora_unet_{key}.lora_up.weight"] = draw((w[0], RANK) + ((1, 1) if len(w) == 4 else ()), gain=0.25)
    add_lcm_lora(SDLoraManager(SimpleNamespace(unet=unet, device=dev, dtype=dt)), tensors, scale=8.0 / 64.0)  # (before the adapter: its validity check reads paths from the UNet down)
    adapter = SDXLLcmAdapter(unet, condition_scale=8.0).inject()
    block = next(m for m in unet.modules() if type(m).__name__ == "ConditionScaleBlock")
    block.Linear.weight = torch.nn.Parameter(draw((320, 256)), requires_grad=False)
    pipe = CompiledSDXL(unet, solver=LCMSolver(STEPS, device=dev, dtype=dt), classifier_free_guidance=False)
    return torch, pipe, adapter, dev, dt


def inputs(torch, dev, dt, n, rows, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g).to(dt)  # noqa: E731
    return r(n, 4, *HW), dict(clip_text_embedding=r(rows, 77, 2048), pooled_text_embedding=r(rows, 1280),
                              time_ids=torch.tensor([[1024, 1024, 0, 0, 1024, 1024]], device=dev).repeat(rows, 1))


def step_ms(torch, pipe, x, kw, reps=8):
    """Median over `reps` trajectories of (device time of the 4 steps) / 4; the first two trajectories (lowering, capture) are not timed."""
    out = []
    for r in range(reps + 2):
        pipe.set_inputs(x, **kw)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(STEPS):
            pipe.step(i)
        e.record()
        torch.cuda.synchronize()
        if r >= 2:
            out.append(s.elapsed_time(e) / STEPS)
    return round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)


def part_steps():
    torch, pipe, _adapter, dev, dt = build()
    res = {}
    for n in (1, 2, 4):
        x, kw = inputs(torch, dev, dt, n, n, seed=n)
        res[f"guidance_free_n{n}"] = dict(zip(("median_ms", "min_ms", "max_ms"), step_ms(torch, pipe, x, kw)))
        st = pipe.engine.stats
        assert st["fallback_nodes"] == [] and st["lcm_condition_scale_folded"] and pipe.engine.io.x.shape[0] == n
        res[f"guidance_free_n{n}"]["launches"] = st["step_ops"]
    pipe.classifier_free_guidance = True  # the guided step of the same tree, same process (the reference warns against it for LCM: a cost comparison only)
    x, kw = inputs(torch, dev, dt, 1, 2, seed=9)
    res["guided_n1"] = dict(zip(("median_ms", "min_ms", "max_ms"), step_ms(torch, pipe, x, kw)), launches=pipe.engine.stats["step_ops"])
    res["gemm_tuning"] = pipe.engine.stats.get("gemm_tuning")
    return res


def part_trajectory():
    torch, pipe, _adapter, dev, dt = build()
    walls = []
    for r in range(7):  # a NEW prompt every time: set_inputs stages it and the first step runs the prologue
        x, kw = inputs(torch, dev, dt, 1, 1, seed=100 + r)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.set_inputs(x, **kw)
        pipe.sample()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    st = pipe.engine.stats
    assert st["fallback_nodes"] == [] and st["lowerings"] == 1 and st["prologue_runs"] == 7
    timed = walls[2:]
    return {"trajectory_n1_ms": {"median": round(statistics.median(timed), 2), "min": round(min(timed), 2), "max": round(max(timed), 2)},
            "first_trajectory_ms_with_lowering_and_capture": round(walls[0], 1), "prologue_launches": st["prologue_ops"], "step_launches": st["step_ops"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=list(PARTS))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.part:
        print("RESULT " + json.dumps({"steps": part_steps, "trajectory": part_trajectory}[args.part]()), flush=True)
        return
    out = {}
    for part, limit in PARTS.items():
        r = subprocess.run([sys.executable, __file__, "--part", part], timeout=limit, capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
            raise SystemExit(f"part {part} failed (exit status {r.returncode}); nothing more is started")
        out[part] = json.loads(line[len("RESULT "):])
        print(json.dumps({part: out[part]}), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
