"""pytest -m gpu: step-constant UNet input channels on the MI355X -- `CompiledSDXL.set_inputs(..., input_condition=...)` on the trees of
StableDiffusion_1_Inpainting (SD1UNet(9)) and ICLight (SD1UNet(4) widened to 8 and patched) against the REAL reference's trajectories
(tests/golden/sd1_inpainting.safetensors, tools/make_golden_inpainting.py), in direct replay and as a captured graph; `CompiledInpaintConditions`
against the reference's set_inpainting_conditions.

Float32 bar: the project's (tests/test_engine_gpu.py): relative l2 and relative maximum < 1e-3 at EVERY recorded step.  bfloat16: at every recorded
step the relative l2 against the float32 golden is no larger than that of the mirror's unfused bfloat16 forward of the same tree on the same GPU
(both figures are printed)."""
import json
import warnings
from types import SimpleNamespace

import pytest
import torch

import refiners_amd.fluxion.layers as fl
from refiners_amd import native, synth
from refiners_amd.engine.compiled import CompiledSDXL
from refiners_amd.engine.image_conditioned import CompiledInpaintConditions
from refiners_amd.latent_diffusion import ICLight, SD1Autoencoder, StableDiffusion_1_Inpainting
from refiners_amd.latent_diffusion.controlnet import SD1ControlnetAdapter
from refiners_amd.latent_diffusion.sampling import DDIM
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from refiners_amd.latent_diffusion.solvers import DPMSolver, Euler
from tests import inpainting_cases as IC
from tests import support as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_TOL = 1e-3
API = SimpleNamespace(Inpainting=lambda unet, solver: StableDiffusion_1_Inpainting(unet=unet, solver=solver),
                      ICLight=lambda patch, unet, solver: ICLight(patch, unet=unet, solver=solver), SD1ControlnetAdapter=SD1ControlnetAdapter)
SOLVERS = SimpleNamespace(DDIM=DDIM, DPMSolver=DPMSolver, Euler=Euler)


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


@pytest.fixture(scope="module")
def gold():
    return S.golden("sd1_inpainting")


@pytest.fixture(scope="module")
def shapes4():
    return S.key_shapes("sd1")


def _unet9(shapes4, dtype):
    u = SD1UNet(9, device="meta")
    S.load_mirror_weights(u, synth.synth_state_dict(IC.unet_shapes(shapes4, 9), IC.SEED["weight_seed"]), device=DEV, dtype=dtype)
    return u


@pytest.fixture(scope="module")
def unet9(shapes4):
    """One float32 inpainting UNet on the GPU: the tests inject and eject their own adapters."""
    return _unet9(shapes4, torch.float32)


def _unet4(dtype=torch.float32):
    u = SD1UNet(4, device="meta")
    S.load_mirror_weights(u, S.weights("sd1", IC.SEED["weight_seed"]), device=DEV, dtype=dtype)  # (a copy on the device: ICLight patches it in place)
    return u


def _controlnet_weights():
    shapes = {k: tuple(v) for k, v in json.loads((S.GOLD / "sd1_controlnet_keys.json").read_text()).items()}
    return synth.synth_state_dict(shapes, IC.SEED["weight_seed"] + IC.SEED["controlnet_seed"])


class _Case:
    """The case's tree (adapters, IC-Light's patch) on a UNet through the shared builder, the mirror's pipeline beside it; taken off again on exit."""

    def __init__(self, name, unet, shapes4, dtype=torch.float32):
        self.name, self.unet, self.shapes4, self.dtype = name, unet, shapes4, dtype

    def __enter__(self):
        case = IC.CASES[self.name]
        self.pipeline, self.undo = IC.build(self.name, API, self.unet, IC.make_solver(self.name, SOLVERS, device=DEV, dtype=self.dtype), self.shapes4,
                                            controlnet_weights=_controlnet_weights() if case.get("controlnet") else None, device=DEV, dtype=self.dtype)
        return self

    def __exit__(self, *exc):
        self.undo()

    def engine(self, use_graph):
        case = IC.CASES[self.name]
        return CompiledSDXL(self.pipeline.unet, solver=IC.make_solver(self.name, SOLVERS, device=DEV), condition_scale=case["scale"],  # (host coefficients: float32 tables)
                            use_graph=use_graph, classifier_free_guidance=case["cfg"])

    def set_inputs(self, sd):
        inp = {k: v.to(DEV) for k, v in IC.inputs(self.name).items()}
        kw = {"conditions": {"controlnet.condition_canny": inp["picture"]}} if "picture" in inp else {}
        sd.set_inputs(inp["x"], clip_text_embedding=inp["text"], input_condition=inp["condition"], **kw)


@pytest.mark.parametrize("use_graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("name", list(IC.CASES))
def test_float32_trajectory_matches_reference(name, use_graph, gold, shapes4, unet9):
    case = IC.CASES[name]
    unet = unet9 if case["tree"] == "inpainting" else _unet4()
    with _Case(name, unet, shapes4) as c, warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # no whole-UNet fallback
        sd = c.engine(use_graph)
        c.set_inputs(sd)
        for s in range(case["run"]):
            x = sd.step(s)
            l2, mx = S.rel_err(x, gold[f"{name}.x{s}"])
            print(f"{name} step {s}: l2 {l2:.2e} max {mx:.2e}")
            assert l2 < F32_TOL and mx < F32_TOL, (name, s, l2, mx)
            if s == 0 and not case.get("sag"):  # (Self-Attention Guidance folds its second pass into the conditional half of the output)
                l2, mx = S.rel_err(sd.engine.io.out, gold[f"{name}.unet_out"])
                print(f"{name} unet_out: l2 {l2:.2e} max {mx:.2e}")
                assert l2 < F32_TOL and mx < F32_TOL, (name, "unet_out", l2, mx)
        st = sd.engine.stats
        assert st["fallback_nodes"] == [] and "whole_fallback" not in st
        E, n = IC.inputs(name)["condition"].shape[1], case["n"]
        assert tuple(sd.x.shape) == (n, 4) + case["hw"] and tuple(sd.engine.io.x.shape) == ((2 if case["cfg"] else 1) * n, 4 + E) + case["hw"]
        assert sd.engine_c is None, "with an input_condition the single program is kept"
        if case.get("controlnet"):
            assert st.get("controlnets") == 1
        if case.get("sag"):
            assert sd.engine2 is not None and tuple(sd.engine2.io.x.shape) == (n, 4 + E) + case["hw"]
        if use_graph:
            assert sd.graph is not None
            # the same trajectory again: the same program, the same captured graph, bit-equal
            low, graph, lowerings = sd.engine.low, sd.graph, st["lowerings"]
            first = sd.x.clone()
            c.set_inputs(sd)
            for s in range(case["run"]):
                sd.step(s)
            assert torch.equal(sd.x, first) and sd.engine.low is low and sd.graph is graph and sd.engine.stats["lowerings"] == lowerings


def test_cfg_split_keeps_the_single_program(gold, shapes4, unet9):
    with _Case("dpm", unet9, shapes4) as c:
        sd = CompiledSDXL(unet9, solver=IC.make_solver("dpm", SOLVERS, device=DEV), condition_scale=7.5, cfg_split=True)
        c.set_inputs(sd)
        x = sd.step(0)
        assert sd.engine_c is None
        l2, mx = S.rel_err(x, gold["dpm.x0"])
        assert l2 < F32_TOL and mx < F32_TOL, (l2, mx)


def test_a_new_condition_of_the_same_shape_keeps_the_program_and_the_graph(gold, unet9):
    """ddim_pair's two pictures, one after the other at n = 1: the second trajectory runs on the first one's program and graph."""
    inp = {k: v.to(DEV) for k, v in IC.inputs("ddim_pair").items()}
    n = IC.CASES["ddim_pair"]["n"]
    sd = CompiledSDXL(unet9, solver=IC.make_solver("ddim_pair", SOLVERS, device=DEV), condition_scale=7.5, use_graph=True)
    seen = []
    for i in range(n):
        sd.set_inputs(inp["x"][i : i + 1], clip_text_embedding=inp["text"][[i, n + i]], input_condition=inp["condition"][i : i + 1])
        for s in range(IC.CASES["ddim_pair"]["run"]):
            x = sd.step(s)
            l2, mx = S.rel_err(x, gold[f"ddim_pair.x{s}"][i : i + 1])
            print(f"ddim_pair picture {i} step {s}: l2 {l2:.2e} max {mx:.2e}")
            assert l2 < F32_TOL and mx < F32_TOL, (i, s, l2, mx)
        seen.append((sd.engine.low, sd.graph, sd.engine.stats["lowerings"], sd.cond.data_ptr()))
    assert seen[0][1] is not None
    assert seen[1][0] is seen[0][0] and seen[1][1] is seen[0][1] and seen[1][2:] == seen[0][2:], "no relowering, no new capture, the same buffer"
    # another E drops the graph and relowers; the stem's width is checked against 4 + E with both numbers named
    sd.set_inputs(inp["x"][:1], clip_text_embedding=inp["text"][[0, n]], input_condition=inp["condition"][:1, :4])
    assert sd.graph is None
    with pytest.raises(AssertionError, match=r"reads 9 channels.*4 \+ 4 != 9"):
        sd.step(0)


def _lda(dtype=torch.float32):
    vae_shapes = {k: tuple(v) for k, v in json.loads((S.GOLD / "vae_keys.json").read_text()).items()}
    lda = SD1Autoencoder(device="meta")
    lda.load_state_dict({k: v.to(device=DEV, dtype=dtype) for k, v in synth.synth_state_dict(vae_shapes, IC.SEED["vae_seed"]).items()}, assign=True)
    return lda


def test_compiled_inpaint_conditions_match_reference(gold):
    from PIL import Image

    cond = CompiledInpaintConditions(_lda())
    image, mask = IC.conditions_inputs()
    for size in IC.CONDITIONS["latents_sizes"]:
        ml, tl = cond(Image.fromarray(image.numpy(), mode="RGB"), Image.fromarray(mask.numpy(), mode="L"), latents_size=size)
        assert torch.equal(ml.cpu(), gold[f"conditions.{size[0]}x{size[1]}.mask_latents"])
        l2, mx = S.rel_err(tl, gold[f"conditions.{size[0]}x{size[1]}.target_image_latents"])
        print(f"conditions {size}: target image latents l2 {l2:.2e} max {mx:.2e}")
        assert l2 < F32_TOL and mx < F32_TOL, (size, l2, mx)
        ml2, tl2 = cond(image.to(DEV), mask.to(DEV), latents_size=size)  # uint8 tensors: the same launches
        assert torch.equal(ml2, ml) and torch.equal(tl2, tl)
        if tuple(ml.shape[2:]) == tuple(tl.shape[2:]):  # latents_size = the picture's size / 8: what set_inputs(input_condition=...) takes
            assert torch.cat((ml, tl), dim=1).shape[1] == 5


@pytest.mark.parametrize("name", ["dpm", "euler"])
def test_bfloat16_no_worse_than_unfused_torch(name, gold, shapes4):
    case = IC.CASES[name]
    unet = _unet9(shapes4, torch.bfloat16)
    with _Case(name, unet, shapes4, torch.bfloat16) as c:
        sd = c.engine(True)
        c.set_inputs(sd)
        native_x = [sd.step(s).float().clone() for s in range(case["run"])]
        assert sd.engine.stats["fallback_nodes"] == []
        torch_x = IC.run(c.pipeline, name, device=DEV, dtype=torch.bfloat16)  # the stock Chain forward on torch's bf16 kernels
    pairs = []
    for s in range(case["run"]):
        a, b = S.rel_err(native_x[s], gold[f"{name}.x{s}"])[0], S.rel_err(torch_x[s].float(), gold[f"{name}.x{s}"])[0]
        pairs.append((a, b))
        print(f"{name} bf16 step {s}: engine l2 {a:.3e}; torch-bf16 unfused l2 {b:.3e}; ratio {a / b:.3f}")
    assert all(a <= b for a, b in pairs), (name, pairs)


class _SkipFilter(fl.Concatenate):
    """FreeU's concatenator shape: reads the UNet's residuals from the context store at run time, so the whole tree takes the stock forward."""

    def __init__(self, n: int) -> None:
        super().__init__(fl.Identity(), fl.Chain(fl.UseContext(context="unet", key="residuals").compose(lambda r: r[n]), fl.Lambda(lambda t: t * 0.5)), dim=1)


def test_a_tree_the_lowering_refuses_still_steps_through_the_stock_forward(shapes4, unet9):
    from refiners_amd.latent_diffusion.blocks import ResidualConcatenator

    name = "euler"  # the solver that scales its model input: the fallback scales the whole concatenation
    block = unet9.layer(("UpBlocks", 0), fl.Chain)
    old, new = block.ensure_find(ResidualConcatenator), _SkipFilter(-2)
    block.replace(old, new)
    try:
        with _Case(name, unet9, shapes4) as c:
            sd = c.engine(True)
            c.set_inputs(sd)
            with pytest.warns(RuntimeWarning, match="not lowered"):
                got = [sd.step(s).clone() for s in range(2)]
            assert "whole_fallback" in sd.engine.stats
            want = IC.run(c.pipeline, name, device=DEV)[:2]
        for s in range(2):
            l2, mx = S.rel_err(got[s], want[s])
            print(f"9-channel tree with a context-reading node, step {s}: l2 {l2:.2e} max {mx:.2e}")
            assert l2 < F32_TOL and mx < F32_TOL, (s, l2, mx)
    finally:
        block.replace(new, old)


def test_four_channel_inputs_on_the_same_engine_object_still_match_their_goldens():
    """An input_condition the tree cannot read is refused with both numbers; the same CompiledSDXL then runs plain 4-channel inputs as before."""
    from refiners_amd.latent_diffusion.sdxl import SDXLUNet

    cfg = S.CASES["sdxl_bare"]
    unet = SDXLUNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sdxl", cfg["weight_seed"]), device=DEV, dtype=torch.float32)
    inp = {k: v.to(DEV) for k, v in synth.sdxl_inputs(cfg["images"], cfg["latent_hw"], cfg["input_seed"]).items()}
    kw = dict(clip_text_embedding=inp["text"], pooled_text_embedding=inp["pooled"], time_ids=inp["time_ids"])
    sd = CompiledSDXL(unet, num_inference_steps=cfg["num_steps"], condition_scale=cfg["condition_scale"])
    sd.set_inputs(inp["x"], input_condition=torch.zeros(1, 5, *cfg["latent_hw"], device=DEV), **kw)
    with pytest.raises(AssertionError, match=r"reads 4 channels.*4 \+ 5 != 4"):
        sd.step(cfg["step"])
    sd.set_inputs(inp["x"], **kw)
    l2, mx = S.rel_err(sd.step(cfg["step"]), S.golden("sdxl_bare")["x_next"])
    print(f"sdxl_bare after a refused input_condition: l2 {l2:.2e} max {mx:.2e}")
    assert l2 < F32_TOL and mx < F32_TOL and sd.cond is None, (l2, mx)
    del sd, unet
    # SD1.5: the bare golden is one UNet output at timestep 500, so the solver's first timestep is set to it and the UNet runs on x alone
    cfg = S.CASES["sd1_bare"]
    unet = _unet4()
    x = torch.randn((1, 4, *cfg["latent_hw"]), generator=synth._gen("in.x", cfg["input_seed"])).to(DEV)
    text = torch.randn((1, 77, 768), generator=synth._gen("in.text", cfg["input_seed"])).to(DEV)
    solver = DDIM(2)
    solver.timesteps = torch.tensor([cfg["timestep"], 1])
    sd = CompiledSDXL(unet, solver=solver, classifier_free_guidance=False)
    sd.set_inputs(x, clip_text_embedding=text, input_condition=torch.zeros(1, 4, *cfg["latent_hw"], device=DEV))
    with pytest.raises(AssertionError, match=r"reads 4 channels.*4 \+ 4 != 4"):
        sd.step(0)
    sd.set_inputs(x, clip_text_embedding=text)
    sd.step(0)
    l2, mx = S.rel_err(sd.engine.io.out, S.golden("sd1_bare")["unet_out"])
    print(f"sd1_bare after a refused input_condition: l2 {l2:.2e} max {mx:.2e}")
    assert l2 < F32_TOL and mx < F32_TOL, (l2, mx)
