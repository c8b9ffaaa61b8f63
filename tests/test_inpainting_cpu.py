"""The host mirror of the pipelines whose UNet reads step-constant channels behind the latents (refiners_amd/latent_diffusion/image_conditioned.py:
StableDiffusion_1_Inpainting, ICLight) against the REAL reference's trajectories (tests/golden/sd1_inpainting.safetensors, written by
tools/make_golden_inpainting.py), on CPU float32 through the stock Chain forward; the state dict IC-Light's two construction steps leave; the
conditions of an inpainting run; and the lowering's dry run on 9-channel trees (meta device: argument structs are built, nothing is launched).

Bar: the project's 1e-3 on relative l2 and relative maximum (tests/support.rel_err); the mirror repeats the reference's torch operations, so the
figures printed are ~1e-6."""
from types import SimpleNamespace

import pytest
import torch

from refiners_amd import synth
from refiners_amd.engine.packing import launches
from refiners_amd.engine.unet_lowering import UNetIO, UNetLowering
from refiners_amd.latent_diffusion import ICLight, SD1Autoencoder, StableDiffusion_1_Inpainting
from refiners_amd.latent_diffusion.controlnet import SD1ControlnetAdapter
from refiners_amd.latent_diffusion.sampling import DDIM
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from refiners_amd.latent_diffusion.solvers import DPMSolver, Euler
from tests import inpainting_cases as IC
from tests import support as S

TOL = 1e-3
API = SimpleNamespace(Inpainting=lambda unet, solver: StableDiffusion_1_Inpainting(unet=unet, solver=solver),
                      ICLight=lambda patch, unet, solver: ICLight(patch, unet=unet, solver=solver), SD1ControlnetAdapter=SD1ControlnetAdapter)
SOLVERS = SimpleNamespace(DDIM=DDIM, DPMSolver=DPMSolver, Euler=Euler)


@pytest.fixture(scope="module")
def gold():
    return S.golden("sd1_inpainting")


@pytest.fixture(scope="module")
def shapes4():
    return S.key_shapes("sd1")


@pytest.fixture(scope="module")
def unet9(shapes4):
    u = SD1UNet(9, device="meta")
    shapes9 = IC.unet_shapes(shapes4, 9)
    assert synth.model_shapes(u) == shapes9
    S.load_mirror_weights(u, synth.synth_state_dict(shapes9, IC.SEED["weight_seed"]))
    return u


def _unet4(shapes4):
    u = SD1UNet(4, device="meta")
    # clones: ICLight._apply_patch loads the patched state dict IN PLACE, and S.weights is a cache the other test files share
    S.load_mirror_weights(u, {k: v.clone() for k, v in S.weights("sd1", IC.SEED["weight_seed"]).items()})
    return u


def _controlnet_weights():
    import json

    shapes = {k: tuple(v) for k, v in json.loads((S.GOLD / "sd1_controlnet_keys.json").read_text()).items()}
    return synth.synth_state_dict(shapes, IC.SEED["weight_seed"] + IC.SEED["controlnet_seed"])


@pytest.mark.parametrize("name", list(IC.CASES))
def test_mirror_trajectory_matches_reference(name, gold, shapes4, unet9):
    case = IC.CASES[name]
    unet = unet9 if case["tree"] == "inpainting" else _unet4(shapes4)
    sd, undo = IC.build(name, API, unet, IC.make_solver(name, SOLVERS), shapes4, controlnet_weights=_controlnet_weights() if case.get("controlnet") else None)
    try:
        xs = IC.run(sd, name)
    finally:
        undo()
    assert len(xs) == case["run"]
    for s, x in enumerate(xs):
        l2, mx = S.rel_err(x, gold[f"{name}.x{s}"])
        print(f"{name} step {s}: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < TOL and mx < TOL, (name, s, l2, mx)


def test_constructor_defaults_are_the_reference_s():
    sd = StableDiffusion_1_Inpainting(device="meta")
    assert sd.mask_latents is None and sd.target_image_latents is None
    assert next(m for m in sd.unet.modules() if isinstance(m, torch.nn.Conv2d)).in_channels == 9  # SD1UNet(in_channels=9)
    assert isinstance(sd.solver, DPMSolver) and sd.solver.num_inference_steps == 30
    with pytest.raises(AssertionError):
        sd(torch.zeros(1, 4, 8, 8), step=0, clip_text_embedding=torch.zeros(2, 77, 768))  # conditions not set


def test_iclight_widens_conv_in_and_adds_the_patch(shapes4):
    key = IC.conv_in_key(shapes4)
    before = S.weights("sd1", IC.SEED["weight_seed"])
    zero_patch = {k: torch.zeros(s) for k, s in IC.unet_shapes(shapes4, 8).items()}
    sd = ICLight(zero_patch, unet=_unet4(shapes4))  # the widening alone
    got = sd.unet.state_dict()
    assert list(got) == list(shapes4), "same keys, same order"
    assert tuple(got[key].shape) == (320, 8, 3, 3)
    assert torch.equal(got[key][:, :4], before[key]) and not got[key][:, 4:].any(), "zeros in the new columns before the patch"
    assert all(torch.equal(got[k], before[k]) for k in shapes4 if k != key)
    patch = IC.iclight_patch(shapes4)
    assert all(float(p.abs().max()) > 0 for p in patch.values()), "the synthetic patch moves every key"
    sd = ICLight(patch, unet=_unet4(shapes4))
    got = sd.unet.state_dict()
    assert list(got) == list(shapes4) and tuple(got[key].shape) == (320, 8, 3, 3)
    assert torch.equal(got[key][:, :4], before[key] + patch[key][:, :4]) and torch.equal(got[key][:, 4:], patch[key][:, 4:])
    assert all(torch.equal(got[k], before[k] + patch[k]) for k in shapes4 if k != key)
    assert ICLight.compute_gray_composite.__name__ and hasattr(sd, "set_ic_light_condition")


def test_gray_composite_puts_127_under_a_black_mask():
    from PIL import Image

    image = Image.new("RGB", (4, 2), (10, 200, 30))
    mask = Image.new("L", (4, 2), 0)
    mask.putpixel((1, 0), 255)
    out = ICLight.compute_gray_composite(image, mask)
    assert out.getpixel((1, 0)) == (10, 200, 30) and out.getpixel((0, 0)) == (127, 127, 127)
    with pytest.raises(AssertionError):
        ICLight.compute_gray_composite(image, mask.convert("RGB"))


def test_set_inpainting_conditions_matches_reference(gold, unet9):
    import json

    from PIL import Image

    vae_shapes = {k: tuple(v) for k, v in json.loads((S.GOLD / "vae_keys.json").read_text()).items()}
    lda = SD1Autoencoder(device="meta")
    assert synth.model_shapes(lda) == vae_shapes
    lda.load_state_dict(synth.synth_state_dict(vae_shapes, IC.SEED["vae_seed"]), assign=True)
    sd = StableDiffusion_1_Inpainting(unet=unet9, lda=lda)
    image, mask = IC.conditions_inputs()
    assert set(mask.unique().tolist()) == set(IC.CONDITIONS["mask_values"])
    for size in IC.CONDITIONS["latents_sizes"]:
        with torch.no_grad():
            ml, tl = sd.set_inpainting_conditions(Image.fromarray(image.numpy(), mode="RGB"), Image.fromarray(mask.numpy(), mode="L"), latents_size=size)
        assert sd.mask_latents is ml and sd.target_image_latents is tl
        assert torch.equal(ml, gold[f"conditions.{size[0]}x{size[1]}.mask_latents"])
        l2, mx = S.rel_err(tl, gold[f"conditions.{size[0]}x{size[1]}.target_image_latents"])
        print(f"conditions {size}: target image latents l2 {l2:.2e} max {mx:.2e}")
        assert l2 < TOL and mx < TOL, (size, l2, mx)


# ---- the lowering's dry run --------------------------------------------------------------------------------------------------------------
def _dry(unet, channels, B=2, H=32, W=32, controlnet=False):
    dev = torch.device("meta")
    io = UNetIO(x=torch.empty(B, channels, H, W, device=dev), timestep=torch.empty(B, device=dev), out=torch.empty(B, 4, H, W, device=dev))
    io.tokens[("cross_attention_block", "clip_text_embedding")] = (torch.zeros(B * 128, 768, device=dev), 77)
    if controlnet:
        io.conditions["controlnet.condition_canny"] = torch.empty(1, 3, 8 * H, 8 * W, device=dev)
    low = UNetLowering(dev, torch.float32)
    low.lower(unet, io)
    return low


def _names(low):
    return [e[2] for e in low.step]


def _stem_ks(low):
    """K of the GEMM behind every im2col of the model input: the stems' im2col widths."""
    names = _names(low)
    at = [i for i, n in enumerate(names) if n == "mi355x_im2col3x3_nchw"]
    assert at and all(names[i + 1] == "mi355x_gemm" for i in at)
    return [int(low.step[i + 1][1][0]._obj.seg[0].k) for i in at]


def test_lowering_accepts_a_nine_channel_tree_and_leaves_the_four_channel_program_alone():
    low4 = _dry(SD1UNet(4, device="meta"), 4)
    low9 = _dry(SD1UNet(9, device="meta"), 9)
    assert low9.stats["fallback_nodes"] == [] and low4.stats["fallback_nodes"] == []
    # the only difference is the stem GEMM's K: 9 taps x 4 channels against 9 x 9, each padded to the K block
    assert _names(low9) == _names(low4) and launches(low9.step) == launches(low4.step)
    kblk = low4.kblk
    assert _stem_ks(low4) == [(36 + kblk - 1) // kblk * kblk] and _stem_ks(low9) == [(81 + kblk - 1) // kblk * kblk]
    from refiners_amd.engine.packing import Unsupported

    with pytest.raises(Unsupported, match="reads 4 channels, the model input has 9"):
        _dry(SD1UNet(4, device="meta"), 9)  # a model input the tree cannot read is refused, not mis-lowered


def test_lowering_accepts_a_controlnet_in_front_of_a_nine_channel_tree():
    u4, u9 = SD1UNet(4, device="meta"), SD1UNet(9, device="meta")
    SD1ControlnetAdapter(u4, name="canny").inject()
    SD1ControlnetAdapter(u9, name="canny").inject()
    low4, low9 = _dry(u4, 4, controlnet=True), _dry(u9, 9, controlnet=True)
    for low in (low4, low9):
        assert low.stats["controlnets"] == 1 and low.stats["fallback_nodes"] == []
    # the Controlnet's stem multiplies the same im2col layout as the UNet's (its weight zero-padded over the other channels): no launch more than today
    assert _names(low9) == _names(low4)
    kblk = low9.kblk
    assert _stem_ks(low9) == [(81 + kblk - 1) // kblk * kblk] * 2, "both stems read 81 (padded) im2col columns"
    assert _stem_ks(low4) == [(36 + kblk - 1) // kblk * kblk] * 2
