"""Time per MultiDiffusion step on a 2 x 2 grid of 128 x 128 tiles (canvas 240 x 240 latents, overlap 16), SDXL, bf16, DDIM:
  * `CompiledMultiDiffusion` at tile_batch 1 / 2 / 4  (md1, md2, md4)
  * the best alternative without it (loop): a Python loop over the targets of `CompiledSDXL.set_inputs` + `step` on the cropped tile, with the
    canvas arithmetic of MultiDiffusion.__call__ in torch.
Wall-clock per step over `--steps` steps after `--warmup` (host work is part of what is compared), one synchronisation at each end.  Every variant runs
in a child process of its own under its own time limit; the parent never opens the GPU.
    python tools/probe_multi_diffusion.py [--steps 20] [--warmup 4] [--json profiles/multi_diffusion_probe.json]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

VARIANTS = ("loop", "md1", "md2", "md4")
CANVAS, TILE, OVERLAP, NUM_STEPS = 240, 128, 16, 30


def run_variant(name: str, steps: int, warmup: int) -> dict:
    import torch

    import bench
    from refiners_amd.engine.compiled import CompiledSDXL
    from refiners_amd.engine.multi_diffusion import CompiledMultiDiffusion
    from refiners_amd.latent_diffusion import multi_diffusion as M
    from refiners_amd.latent_diffusion.sampling import DDIM
    from refiners_amd.latent_diffusion.sdxl import SDXLUNet

    dev, dt = torch.device("cuda"), torch.bfloat16
    unet = SDXLUNet(4, device="meta")
    bench.gpu_weights(unet, 0, dt, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev).to(dt)  # noqa: E731
    tiles = M.MultiDiffusion.generate_latent_tiles(M.Size(CANVAS, CANVAS), M.Size(TILE, TILE), min_overlap=OVERLAP)
    assert len(tiles) == 4
    ids = torch.tensor([[1024, 1024, 0, 0, 1024, 1024]], device=dev).repeat(2, 1)
    targets = [M.SDXLTarget(tile=t, solver=DDIM(NUM_STEPS), clip_text_embedding=rnd(2, 77, 2048), pooled_text_embedding=rnd(2, 1280), time_ids=ids, condition_scale=5.0 + i)
               for i, t in enumerate(tiles)]
    x0, noise = rnd(1, 4, CANVAS, CANVAS), rnd(1, 4, CANVAS, CANVAS)

    if name == "loop":
        pipes = [CompiledSDXL(unet, num_inference_steps=NUM_STEPS, condition_scale=t.condition_scale) for t in targets]  # one per target: its own graph and prologue
        for p in pipes[1:]:
            p.engine.cache = pipes[0].engine.cache

        def one(x, s):
            num, cum = torch.zeros_like(x), torch.zeros_like(x)
            for p, t in zip(pipes, targets):
                p.set_inputs(t.crop(x), clip_text_embedding=t.clip_text_embedding, pooled_text_embedding=t.pooled_text_embedding, time_ids=t.time_ids)
                view = p.step(s)
                num = t.paste(num, crop=t.crop(num) + t.weight)
                cum = t.paste(cum, crop=t.crop(cum) + t.weight * view)
            return torch.where(num > 0, cum / num, x)
    else:
        md = CompiledMultiDiffusion(unet, tile_batch=int(name[2:]))

        def one(x, s):
            return md(x, noise=noise, step=s, targets=targets)

    x = x0.clone()
    for s in range(warmup):
        x = one(x, s % NUM_STEPS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(warmup, warmup + steps):
        x = one(x, s % NUM_STEPS)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert bool(torch.isfinite(x.float()).all())
    out = {"variant": name, "ms_per_step": round(ms, 3), "steps": steps, "warmup": warmup}
    if name != "loop":
        out["chunks"], out["graph_replayed"] = len(md.stats["chunks"]), md.stats["graph_replayed"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds a variant's child process may take")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.variant:
        print("RESULT " + json.dumps(run_variant(args.variant, args.steps, args.warmup)), flush=True)
        return
    results = []
    for name in VARIANTS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--variant", name, "--steps", str(args.steps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:  # nothing more is started on the GPU after a variant that did not end well
            print(r.stdout[-4000:], file=sys.stderr)
            raise SystemExit(f"{name}: exit status {r.returncode}")
        results.append(json.loads(line[7:]))
        print(json.dumps(results[-1]), flush=True)
    loop = results[0]["ms_per_step"]
    out = {"workload": f"SDXL bf16, DDIM, canvas {CANVAS} x {CANVAS} latents, 4 targets of {TILE} x {TILE} (overlap {OVERLAP}), wall-clock ms per MultiDiffusion step",
           "results": results, "speedup_over_loop": {r["variant"]: round(loop / r["ms_per_step"], 3) for r in results[1:]}}
    print(json.dumps(out["speedup_over_loop"]), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
