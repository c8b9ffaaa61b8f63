"""Time of one tiled VAE decode of a 2048 x 2048 image (256 x 256 latents) at tile 512 / blending 64 (a 5 x 5 grid), SDXL autoencoder, bf16:
  * `CompiledTiledVAE` at tile_batch 1 / 2 / 4  (tv1, tv2, tv4), statistics from calibrate() on a random 512 x 512 tensor
  * the best alternative without it (loop): a Python loop of `CompiledVAEDecoder` per tile with the masks and the accumulate / divide of _tiled_decode in
    torch.  That loop recomputes the GroupNorm statistics per tile, so its IMAGE is not the tiled result (seams); only its time is compared.
Wall-clock per decode over `--steps` decodes after `--warmup` (host work is part of what is compared), one synchronisation at each end.  Every variant
runs in a child process of its own under its own time limit; the parent never opens the GPU.  Not run yet: no figure from it is recorded anywhere.
    python tools/probe_tiled_vae.py [--steps 5] [--warmup 2] [--json profiles/tiled_vae_probe.json]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

VARIANTS = ("loop", "tv1", "tv2", "tv4")
LATENT, TILE, BLENDING = 256, (512, 512), 64


def run_variant(name: str, steps: int, warmup: int) -> dict:
    import torch

    import bench
    from refiners_amd.engine.tiled_vae import CompiledTiledVAE, latent_grid
    from refiners_amd.engine.vae import CompiledVAEDecoder
    from refiners_amd.latent_diffusion.vae import SDXLAutoencoder, _create_blending_mask, _ImageSize

    dev, dt = torch.device("cuda"), torch.bfloat16
    vae = SDXLAutoencoder(device="meta")
    bench.gpu_weights(vae, 0, dt, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    z = (torch.randn(1, 4, LATENT, LATENT, generator=g, device=dev) * 0.13).to(dt)
    grid = latent_grid((LATENT, LATENT), TILE, BLENDING)

    if name == "loop":
        dec = CompiledVAEDecoder(vae)
        masks = {}
        for top, left, bottom, right in grid.tiles:
            edge = (top == 0, bottom == LATENT, left == 0, right == LATENT)
            masks[(top, left)] = _create_blending_mask(_ImageSize(8 * (bottom - top), 8 * (right - left)), BLENDING, 3, device=dev, dtype=dt, is_edge=edge)

        def one():
            result = torch.zeros(1, 3, 8 * LATENT, 8 * LATENT, device=dev, dtype=dt)
            weights = torch.zeros_like(result)
            for top, left, bottom, right in grid.tiles:
                tile = dec(z[:, :, top:bottom, left:right])  # (tiles of another size re-lower: CompiledVAEDecoder keeps one program)
                result[:, :, 8 * top : 8 * bottom, 8 * left : 8 * right] += tile * masks[(top, left)]
                weights[:, :, 8 * top : 8 * bottom, 8 * left : 8 * right] += masks[(top, left)]
            return result / weights
    else:
        eng = CompiledTiledVAE(vae, tile_size=TILE, blending=BLENDING, tile_batch=int(name[2:]))
        eng.calibrate((torch.rand(1, 3, TILE[1], TILE[0], generator=g, device=dev) * 2 - 1).to(dt))

        def one():
            return eng.decode(z)

    for _ in range(warmup):
        img = one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        img = one()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert bool(torch.isfinite(img.float()).all())
    out = {"variant": name, "ms_per_decode": round(ms, 3), "steps": steps, "warmup": warmup, "tiles": len(grid.tiles)}
    if name != "loop":
        out["tile_groups"], out["graph_replayed"], out["program_launches"] = len(eng.stats["tile_groups"]), eng.stats["graph_replayed"], sorted(eng.stats["program_launches"].values())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS, default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
    loop = results[0]["ms_per_decode"]
    out = {"workload": f"SDXL autoencoder bf16, decode of {LATENT} x {LATENT} latents at tile {TILE} / blending {BLENDING}, wall-clock ms per decode",
           "results": results, "speedup_over_loop": {r["variant"]: round(loop / r["ms_per_decode"], 3) for r in results[1:]}}
    print(json.dumps(out["speedup_over_loop"]), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
