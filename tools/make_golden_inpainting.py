"""Golden vectors of the pipelines whose UNet reads step-constant channels behind the latents: the REAL reference's StableDiffusion_1_Inpainting
(SD1UNet(9); DPM-Solver++, DDIM on a pair of pictures, Euler, guidance-free, Self-Attention Guidance, with an SD1ControlnetAdapter) and ICLight
(SD1UNet(4) widened to 8 channels + a seeded synthetic weight patch), synthetic weights, CPU float32, per case of tests/inpainting_cases.py:
    <case>.x<s>          the latents after step s (every step that is run)
    <case>.unet_out      the UNet's output at step 0
    conditions.<h>x<w>.mask_latents / .target_image_latents     set_inpainting_conditions on a seeded uint8 picture and mask, synthetic autoencoder
Only the reference's OUTPUTS are stored.  Run where refiners' sources are (the build container), not on a GPU box:
    python tools/make_golden_inpainting.py
-> tests/golden/sd1_inpainting.safetensors (sharded by tensor rows as tests/support.golden reads them, should it outgrow a committed file)"""
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
from refiners.foundationals.latent_diffusion.solvers import DDIM, DPMSolver, Euler  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.controlnet import SD1ControlnetAdapter  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.ic_light import ICLight  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.model import SD1Autoencoder, StableDiffusion_1_Inpainting  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet  # noqa: E402

from refiners_amd import synth  # noqa: E402
from tests import inpainting_cases as IC  # noqa: E402

GOLD = ROOT / "tests" / "golden"
LIMIT = 1 << 20  # bytes of a committed file
NOTHING = lambda: rfl.Chain(rfl.Identity())  # noqa: E731  (text encoder / autoencoder of a pipeline that is given embeddings and latents)
API = SimpleNamespace(
    Inpainting=lambda unet, solver: StableDiffusion_1_Inpainting(unet=unet, lda=NOTHING(), clip_text_encoder=NOTHING(), solver=solver),  # type: ignore[arg-type]
    ICLight=lambda patch, unet, solver: ICLight(patch, unet=unet, lda=NOTHING(), clip_text_encoder=NOTHING(), solver=solver),  # type: ignore[arg-type]
    SD1ControlnetAdapter=SD1ControlnetAdapter)
SOLVERS = SimpleNamespace(DDIM=DDIM, DPMSolver=DPMSolver, Euler=Euler)


def save_sharded(out: dict[str, torch.Tensor], stem: str) -> None:
    """One file while it fits; otherwise whole tensors are dealt to `<stem>.safetensors`, `<stem>.1.safetensors`, ... (support.golden joins tensors of
    one name along dim 0, so a tensor larger than a file would be cut by rows; none here is)."""
    shards: list[dict[str, torch.Tensor]] = [{}]
    size = 0
    for k, v in out.items():
        b = v.numel() * v.element_size() + 256
        assert b < LIMIT
        if size + b > LIMIT - 4096:
            shards.append({})
            size = 0
        shards[-1][k] = v
        size += b
    for i, sh in enumerate(shards):
        p = GOLD / (f"{stem}.safetensors" if i == 0 else f"{stem}.{i}.safetensors")
        save_file(sh, str(p))
        print(p.name, p.stat().st_size, "bytes")


def main() -> None:
    shapes4 = synth.model_shapes(SD1UNet(4, device="meta"))
    assert {k: list(v) for k, v in shapes4.items()} == json.loads((GOLD / "sd1_unet_keys.json").read_text())
    shapes9 = synth.model_shapes(SD1UNet(9, device="meta"))
    assert shapes9 == IC.unet_shapes(shapes4, 9)
    cn_shapes = {k: tuple(v) for k, v in json.loads((GOLD / "sd1_controlnet_keys.json").read_text()).items()}
    out: dict[str, torch.Tensor] = {}
    unet9 = reference_model(lambda _c, device: SD1UNet(9, device=device), shapes9, IC.SEED["weight_seed"])
    with torch.no_grad():
        for name, case in IC.CASES.items():
            t0 = time.time()
            unet = unet9 if case["tree"] == "inpainting" else reference_model(SD1UNet, shapes4, IC.SEED["weight_seed"])
            sd, undo = IC.build(name, API, unet, IC.make_solver(name, SOLVERS), shapes4,
                                controlnet_weights=synth.synth_state_dict(cn_shapes, IC.SEED["weight_seed"] + IC.SEED["controlnet_seed"]))
            if case["tree"] == "iclight":
                sdict = sd.unet.state_dict()
                assert tuple(sdict[IC.conv_in_key(shapes4)].shape) == (320, 8, 3, 3) and set(sdict) == set(shapes4)
            seen: list[torch.Tensor] = []
            hook = sd.unet.register_forward_hook(lambda _m, _a, y: seen.append(y.detach().clone()))
            xs = IC.run(sd, name)
            hook.remove()
            undo()
            for s, x in enumerate(xs):
                out[f"{name}.x{s}"] = x
            out[f"{name}.unet_out"] = seen[0].contiguous()
            print(name, tuple(seen[0].shape), [f"{float(x.std()):.3f}" for x in xs], f"{time.time() - t0:.1f}s", flush=True)
        # set_inpainting_conditions: PIL picture and mask -> mask latents and the latents of the masked picture
        from PIL import Image

        vae_shapes = {k: tuple(v) for k, v in json.loads((GOLD / "vae_keys.json").read_text()).items()}
        lda = SD1Autoencoder(device="meta")
        assert synth.model_shapes(lda) == vae_shapes
        lda.load_state_dict(synth.synth_state_dict(vae_shapes, IC.SEED["vae_seed"]), assign=True)
        sd = StableDiffusion_1_Inpainting(unet=unet9, lda=lda, clip_text_encoder=NOTHING())  # type: ignore[arg-type]
        image, mask = IC.conditions_inputs()
        for size in IC.CONDITIONS["latents_sizes"]:
            ml, tl = sd.set_inpainting_conditions(Image.fromarray(image.numpy(), mode="RGB"), Image.fromarray(mask.numpy(), mode="L"), latents_size=size)
            out[f"conditions.{size[0]}x{size[1]}.mask_latents"] = ml.contiguous()
            out[f"conditions.{size[0]}x{size[1]}.target_image_latents"] = tl.contiguous()
            print("conditions", size, tuple(ml.shape), tuple(tl.shape), float(ml.mean()), float(tl.std()), flush=True)
    save_sharded(out, "sd1_inpainting")


if __name__ == "__main__":
    main()
