"""Golden vectors of the few-step workflows: the REAL reference's StableDiffusion_XL with `classifier_free_guidance = False` (LCM with
`SDXLLcmAdapter`, Euler with trailing timesteps in noise and sample prediction, DDIM, DPM-Solver++) and an LCM-LoRA-shaped LoRA attached by
refiners' `add_lcm_lora`, on an SDXL UNet of synthetic weights, CPU float32, per case of tests/few_step_cases.py:
    <case>.x<s>          the latents after step s (every step of the trajectory)
    <case>.unet_out      the UNet's output at the first step
    a.noise<s>           LCM's noise draw of step s;  a.alt_x0: x after step 0 with set_condition_scale(alt_scale), run after the trajectory (the stream's next draw)
and tests/golden/sdxl_few_step.json: the timesteps of every case, and for the LoRA cases the length and SHA-256 of refiners' `debug_map` (key -> module
path).  The map itself (788 pairs) is the "debug_map" entry of the safetensors file's metadata, kept there so that the JSON stays small.
Run where refiners' sources are (the build container), not on a GPU box:
    python tools/make_golden_few_step.py
-> tests/golden/sdxl_few_step.safetensors, tests/golden/sdxl_few_step.json"""
from __future__ import annotations

import hashlib
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
import refiners.foundationals.latent_diffusion.stable_diffusion_xl.lcm_lora as ref_lcm_lora  # noqa: E402
from refiners.fluxion.adapters.lora import auto_attach_loras as ref_auto_attach  # noqa: E402
from refiners.foundationals.latent_diffusion.lora import SDLoraManager  # noqa: E402
from refiners.foundationals.latent_diffusion.solvers import DDIM, DPMSolver, Euler, LCMSolver, ModelPredictionType, SolverParams, TimestepSpacing  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_xl.lcm import SDXLLcmAdapter  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_xl.model import StableDiffusion_XL  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_xl.unet import SDXLUNet  # noqa: E402

from refiners_amd import synth  # noqa: E402
from tests.few_step_cases import FEW_STEP_CASES, LORA_SCALE, case_inputs, lcm_lora_tensors, load_condition_scale_weight, make_solver, noise_draws  # noqa: E402

GOLD = ROOT / "tests" / "golden"
REF_SOLVERS = SimpleNamespace(
    DDIM=DDIM, DPMSolver=DPMSolver, LCMSolver=LCMSolver,
    euler=lambda n, spacing, prediction: Euler(n, params=SolverParams(timesteps_spacing=TimestepSpacing(spacing), model_prediction_type=ModelPredictionType(prediction))))


def main() -> None:
    shapes = synth.model_shapes(SDXLUNet(4, device="meta"))
    out: dict[str, torch.Tensor] = {}
    meta: dict = {"timesteps": {}, "lora_scale": LORA_SCALE}
    debug_map = None
    unet = reference_model(SDXLUNet, shapes, 0)
    with torch.no_grad():
        for name, case in FEW_STEP_CASES.items():
            assert case["weight_seed"] == 0
            t0 = time.time()
            sd = StableDiffusion_XL(unet=unet, lda=rfl.Chain(rfl.Identity()), clip_text_encoder=rfl.Chain(rfl.Identity()),  # type: ignore[arg-type]
                                    solver=make_solver(case, REF_SOLVERS))
            sd.classifier_free_guidance = case["cfg"]
            meta["timesteps"][name] = [float(t) for t in sd.solver.timesteps]
            adapter = manager = None
            if case.get("lcm_scale") is not None:
                adapter = SDXLLcmAdapter(unet, condition_scale=case["lcm_scale"]).inject()
                load_condition_scale_weight(unet)
            if case["lora"]:
                manager = SDLoraManager(sd)
                seen_map: list[tuple[str, str]] = []

                def spy(loras, target, /, **kw):  # add_lcm_lora keeps its debug_map to itself: listen at auto_attach_loras
                    mine: list[tuple[str, str]] = []
                    r = ref_auto_attach(loras, target, **dict(kw, debug_map=mine))
                    seen_map.extend(mine)
                    if kw.get("debug_map") is not None:
                        kw["debug_map"].extend(mine)
                    return r

                import refiners.foundationals.latent_diffusion.lora as ref_lora_module

                saved = (ref_lcm_lora.auto_attach_loras, ref_lora_module.auto_attach_loras)
                ref_lcm_lora.auto_attach_loras = ref_lora_module.auto_attach_loras = spy
                try:
                    ref_lcm_lora.add_lcm_lora(manager, lcm_lora_tensors(shapes), scale=LORA_SCALE)
                finally:
                    ref_lcm_lora.auto_attach_loras, ref_lora_module.auto_attach_loras = saved
                pairs = [list(p) for p in seen_map]
                if debug_map is None:
                    debug_map = pairs
                assert pairs == debug_map, "the LoRA cases attach the same state dict to the same tree"
                meta.setdefault("debug_map", {})[name] = {"pairs": len(pairs), "sha256": hashlib.sha256(json.dumps(pairs).encode()).hexdigest()}
            inp = case_inputs(case)
            kw = dict(clip_text_embedding=inp["text"], pooled_text_embedding=inp["pooled"], time_ids=inp["time_ids"], condition_scale=case.get("condition_scale", 7.5))
            seen: list[torch.Tensor] = []
            hook = unet.register_forward_hook(lambda _m, _a, y: seen.append(y.detach().clone()))
            if case["solver"] == "lcm":
                for s, d in enumerate(noise_draws(case)):
                    out[f"{name}.noise{s}"] = d
                torch.manual_seed(case["noise_seed"])  # the reference's forward hands the solver no generator: it draws from the default one
            x = inp["x"]
            for s in range(case.get("run_steps", case["steps"])):
                x = sd(x, step=s, **kw).contiguous()
                out[f"{name}.x{s}"] = x
            hook.remove()
            out[f"{name}.unet_out"] = seen[0].contiguous()
            if case.get("alt_scale") is not None:
                assert adapter is not None
                adapter.set_condition_scale(case["alt_scale"])
                out[f"{name}.alt_x0"] = sd(inp["x"], step=0, **kw).contiguous()
                moved = float((out[f"{name}.alt_x0"] - out[f"{name}.x0"]).norm() / out[f"{name}.x0"].norm())
                print(f"{name}: condition scale {case['lcm_scale']} -> {case['alt_scale']} moves x0 by {moved:.2e}", flush=True)
            if adapter is not None:
                adapter.eject()
            if manager is not None:
                manager.remove_all()
            print(name, tuple(out[f"{name}.unet_out"].shape), f"{time.time() - t0:.1f}s", flush=True)
    save_file(out, str(GOLD / "sdxl_few_step.safetensors"), metadata={"debug_map": json.dumps(debug_map)})
    (GOLD / "sdxl_few_step.json").write_text(json.dumps(meta, indent=1) + "\n")
    print((GOLD / "sdxl_few_step.safetensors").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
