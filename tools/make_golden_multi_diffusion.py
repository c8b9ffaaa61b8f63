"""Golden vectors of MultiDiffusion: the REAL reference's SDXLMultiDiffusion / SD1MultiDiffusion (`md(x, noise=, step=, targets=)`) over UNets of
synthetic weights, CPU float32, per case of tests/multi_diffusion_cases.py and per step s the case takes:
    <case>.canvas<s>             the canvas after the call at step s (case c: step 1 is called on the canvas step 0 returned)
    <case>.target<i>.step<s>     what diffuse_target returned for target i (absent where the target's window excludes the step)
and the tile lists `MultiDiffusion.generate_latent_tiles` returns for TILE_RECIPES.
Run where refiners' sources are (the build container), not on a GPU box:
    python tools/make_golden_multi_diffusion.py
-> tests/golden/multi_diffusion.safetensors, tests/golden/multi_diffusion_tiles.json"""
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
from refiners.foundationals.latent_diffusion.multi_diffusion import MultiDiffusion, Size, Tile  # noqa: E402
from refiners.foundationals.latent_diffusion.solvers import DDIM, DPMSolver  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.model import StableDiffusion_1  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.multi_diffusion import SD1DiffusionTarget, SD1MultiDiffusion  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_xl.model import StableDiffusion_XL  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_xl.multi_diffusion import SDXLMultiDiffusion, SDXLTarget  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_xl.unet import SDXLUNet  # noqa: E402

from refiners_amd import synth  # noqa: E402
from tests.multi_diffusion_cases import MD_CASES, STEPS, TILE_RECIPES, build_targets, canvas_inputs  # noqa: E402

GOLD = ROOT / "tests" / "golden"
REF_NS = SimpleNamespace(Tile=Tile, SDXLTarget=SDXLTarget, SD1DiffusionTarget=SD1DiffusionTarget)


def reference_solver(kind: str, first: int):
    return (DDIM if kind == "ddim" else DPMSolver)(num_inference_steps=STEPS, first_inference_step=first)


def main() -> None:
    tiles = [{"size": [h, w], "tile_size": [th, tw], "min_overlap": ov,
              "tiles": [list(t) for t in MultiDiffusion.generate_latent_tiles(Size(h, w), Size(th, tw), min_overlap=ov)]} for h, w, th, tw, ov in TILE_RECIPES]
    (GOLD / "multi_diffusion_tiles.json").write_text(json.dumps(tiles, indent=1) + "\n")
    out = {}
    models: dict[str, object] = {}
    ident = lambda: rfl.Chain(rfl.Identity())  # noqa: E731  (the text encoders and the VAE are not called)
    with torch.no_grad():
        for name, case in MD_CASES.items():
            t0 = time.time()
            fam = case["family"]
            if fam not in models:
                cls = SDXLUNet if fam == "sdxl" else SD1UNet
                models[fam] = reference_model(cls, synth.model_shapes(cls(4, device="meta")), 0)
            sd_cls, md_cls = (StableDiffusion_XL, SDXLMultiDiffusion) if fam == "sdxl" else (StableDiffusion_1, SD1MultiDiffusion)
            sd = sd_cls(unet=models[fam], lda=ident(), clip_text_encoder=ident(), solver=DDIM(num_inference_steps=STEPS))  # type: ignore[arg-type]
            md = md_cls(sd)
            targets = build_targets(case, REF_NS, reference_solver)
            inner, seen = md.diffuse_target, {}

            def record(x, step, target, inner=inner, seen=seen, targets=targets):
                y = inner(x=x, step=step, target=target)
                seen[(next(i for i, t in enumerate(targets) if t is target), step)] = y.clone()
                return y

            md.diffuse_target = record  # type: ignore[method-assign]
            x, noise = canvas_inputs(case)
            for s in case["steps"]:
                x = md(x, noise=noise, step=s, targets=targets)
                out[f"{name}.canvas{s}"] = x.contiguous().clone()
            for (i, s), y in seen.items():
                out[f"{name}.target{i}.step{s}"] = y.contiguous()
            print(name, sorted(k for k in out if k.startswith(name + ".")), f"{time.time() - t0:.1f}s", flush=True)
    save_file(out, str(GOLD / "multi_diffusion.safetensors"))
    print((GOLD / "multi_diffusion.safetensors").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
