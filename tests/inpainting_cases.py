"""Cases of the inpainting / IC-Light fixtures (tests/golden/sd1_inpainting.safetensors, written by tools/make_golden_inpainting.py from the
reference's own StableDiffusion_1_Inpainting / ICLight on CPU float32 with synthetic weights): seeds, shapes, seeded inputs, and the builder both
the tool (on the reference's classes) and the tests (on the mirror's) go through.  Golden keys: `<case>.x<s>` the latents after step s (every
step that is run), `<case>.unet_out` the UNet's output at step 0; `conditions.<h>x<w>.mask_latents` / `.target_image_latents`."""
from __future__ import annotations

from typing import Any

SEED = dict(weight_seed=0, input_seed=71, controlnet_seed=11, patch_seed=9, vae_seed=0)
TOKENS = 77
STEPS = 30  # inference steps of every solver; `run` of them are executed
#: name -> what is run.  tree: the UNet the case needs ("inpainting": SD1UNet(9); "iclight": SD1UNet(4) widened and patched by ICLight)
CASES: dict[str, dict[str, Any]] = {
    "dpm": dict(tree="inpainting", hw=(32, 32), n=1, solver="dpm", cfg=True, scale=7.5, run=3),
    "ddim_pair": dict(tree="inpainting", hw=(24, 40), n=2, solver="ddim", cfg=True, scale=7.5, run=2),  # two pictures: masks and latents differ
    "euler": dict(tree="inpainting", hw=(32, 32), n=1, solver="euler", cfg=True, scale=7.5, run=3),  # input scale != 1: constants rescaled every step
    "free": dict(tree="inpainting", hw=(32, 32), n=1, solver="ddim", cfg=False, scale=7.5, run=2),
    "sag": dict(tree="inpainting", hw=(32, 32), n=1, solver="ddim", cfg=True, scale=7.5, run=2, sag=0.75),
    "iclight": dict(tree="iclight", hw=(32, 32), n=1, solver="dpm", cfg=True, scale=1.5, run=2),
    "controlnet": dict(tree="inpainting", hw=(32, 32), n=1, solver="dpm", cfg=True, scale=7.5, run=1, controlnet=dict(name="canny", scale=0.8, scale_decay=0.9)),
}
CONDITIONS = dict(image_hw=(40, 56), latents_sizes=[(5, 7), (7, 9)], mask_values=(0, 127, 128, 255))  # (7, 9): a non-integer ratio
PATCH_GAIN = 0.05  # IC-Light's synthetic weight patch: small deltas on EVERY key


def _gen(what: str):
    from refiners_amd import synth

    return synth._gen(what, SEED["input_seed"])


def inputs(name: str) -> dict:
    """Latents, the text stack ([negative ; conditional] when guided) and the step-constant channels of a case; rows differ."""
    import torch

    case = CASES[name]
    (h, w), n = case["hw"], case["n"]
    out = {"x": torch.randn((n, 4, h, w), generator=_gen(f"{name}.x")),
           "text": torch.randn(((2 if case["cfg"] else 1) * n, TOKENS, 768), generator=_gen(f"{name}.text"))}
    if case["tree"] == "inpainting":
        out["mask_latents"] = (torch.rand((n, 1, h, w), generator=_gen(f"{name}.mask")) > 0.6).float()
        out["target_image_latents"] = torch.randn((n, 4, h, w), generator=_gen(f"{name}.target")) * 0.8
        out["condition"] = torch.cat((out["mask_latents"], out["target_image_latents"]), dim=1)
    else:
        out["condition"] = torch.randn((1, 4, h, w), generator=_gen(f"{name}.condition")) * 0.8  # ONE condition of batch 1
    if case.get("controlnet"):
        out["picture"] = torch.rand((1, 3, 8 * h, 8 * w), generator=_gen(f"{name}.picture"))
    return out


def unet_shapes(shapes4: dict, in_channels: int) -> dict:
    """State-dict shapes of SD1UNet(in_channels) from the bare 4-channel UNet's: only the first convolution's weight differs."""
    key = conv_in_key(shapes4)
    return {k: ((v[0], in_channels) + tuple(v[2:]) if k == key else tuple(v)) for k, v in shapes4.items()}


def conv_in_key(shapes4: dict) -> str:
    return next(k for k, v in shapes4.items() if tuple(v) == (320, 4, 3, 3) and "DownBlocks" in k)


def iclight_patch(shapes4: dict) -> dict:
    """The synthetic weight patch: a seeded delta for every key of the widened (8 input channels) UNet."""
    from refiners_amd import synth

    return {k: PATCH_GAIN * synth.synth_tensor("ic_light_patch." + k, s, SEED["patch_seed"]) for k, s in unet_shapes(shapes4, 8).items()}


def make_solver(name: str, ns: Any, device: Any = "cpu", dtype: Any = None) -> Any:
    """ns: DDIM, DPMSolver, Euler of the reference or of the mirror (same constructor defaults)."""
    import torch

    kind = CASES[name]["solver"]
    cls = {"ddim": ns.DDIM, "dpm": ns.DPMSolver, "euler": ns.Euler}[kind]
    return cls(STEPS, device=device, dtype=dtype or torch.float32)


def build(name: str, api: Any, unet: Any, solver: Any, shapes4: dict, controlnet_weights: Any = None, device: Any = "cpu", dtype: Any = None) -> tuple[Any, Any]:
    """The case's pipeline on `unet` (SD1UNet(9) with its weights loaded, or for IC-Light SD1UNet(4): widened and patched here) -> (pipeline, undo).
    api: `Inpainting(unet, solver)`, `ICLight(patch, unet, solver)` -> pipeline; `SD1ControlnetAdapter`.  Conditions are set from inputs(name)."""
    import torch

    case, inp = CASES[name], inputs(name)
    to = lambda t: t.to(device=device, dtype=dtype or torch.float32)  # noqa: E731
    undo = []
    if case["tree"] == "iclight":
        sd = api.ICLight({k: to(v) for k, v in iclight_patch(shapes4).items()}, unet, solver)
        sd._ic_light_condition = to(inp["condition"])
    else:
        sd = api.Inpainting(unet, solver)
        sd.mask_latents, sd.target_image_latents = to(inp["mask_latents"]), to(inp["target_image_latents"])  # assigned directly: the VAE is not part of these cases
    sd.classifier_free_guidance = case["cfg"]
    if case.get("sag"):
        sd.set_self_attention_guidance(True, scale=case["sag"])
        undo.append(lambda: sd.set_self_attention_guidance(False))
    if case.get("controlnet"):
        cn = case["controlnet"]
        adapter = api.SD1ControlnetAdapter(unet, name=cn["name"], scale=cn["scale"], scale_decay=cn["scale_decay"])
        adapter.controlnet.load_state_dict({k: to(v) for k, v in controlnet_weights.items()}, assign=True)
        adapter.inject()
        adapter.set_controlnet_condition(to(inp["picture"]))
        undo.append(adapter.eject)
        sd.controlnet_adapter = adapter

    def undo_all() -> None:
        for f in reversed(undo):
            f()

    return sd, undo_all


def run(sd: Any, name: str, device: Any = "cpu", dtype: Any = None) -> list:
    """The stock forward of the (reference's or mirror's) pipeline: x after every step that is run."""
    import torch

    case, inp = CASES[name], inputs(name)
    x = inp["x"].to(device=device, dtype=dtype or torch.float32)
    text = inp["text"].to(device=device, dtype=dtype or torch.float32)
    xs = []
    with torch.no_grad():
        for s in range(case["run"]):
            if case.get("controlnet"):  # the context store is reset by every UNet call
                sd.controlnet_adapter.set_controlnet_condition(inp["picture"].to(device=device, dtype=dtype or torch.float32))
            x = sd(x, step=s, clip_text_embedding=text, condition_scale=case["scale"]).contiguous()
            xs.append(x)
    return xs


def conditions_inputs() -> tuple[Any, Any]:
    """A seeded uint8 RGB picture [H, W, 3] and a uint8 mask [H, W] whose values are 0, 127, 128 and 255 (the threshold sits between the middle two)."""
    import torch

    H, W = CONDITIONS["image_hw"]
    image = torch.randint(0, 256, (H, W, 3), generator=_gen("conditions.image"), dtype=torch.uint8)
    mask = torch.tensor(CONDITIONS["mask_values"], dtype=torch.uint8)[torch.randint(0, 4, (H, W), generator=_gen("conditions.mask"))]
    return image, mask
