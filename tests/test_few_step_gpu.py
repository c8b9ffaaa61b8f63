"""pytest -m gpu: few-step SDXL on the MI355X -- `CompiledSDXL(classifier_free_guidance=False)` with LCM (+ `SDXLLcmAdapter`), Euler in
trailing spacing (noise and sample prediction), DDIM and DPM-Solver++, and an LCM-LoRA-shaped LoRA attached by `add_lcm_lora` -- against the
REAL reference's trajectories (tests/golden/sdxl_few_step.*, tools/make_golden_few_step.py), in direct replay and as a captured graph.

Float32 bar: the project's (tests/test_engine_gpu.py): relative l2 and relative maximum < 1e-3 at EVERY stored step.  bfloat16: gated the way
tests/test_sam_hq_gpu.py gates it -- the native error against the float32 golden may be at most BF16_L2_FACTOR x the error of the mirror's
UNFUSED bfloat16 forward of the same tree on the same GPU; docs/MEASUREMENTS_few_step.md holds both measured columns."""
import os
import sys
import warnings
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from refiners_amd import native
from refiners_amd.engine.compiled import CompiledSDXL
from refiners_amd.latent_diffusion.adapters import SDLoraManager
from refiners_amd.latent_diffusion.lcm import SDXLLcmAdapter, add_lcm_lora
from refiners_amd.latent_diffusion.sampling import DDIM
from refiners_amd.latent_diffusion.sdxl import SDXLUNet
from refiners_amd.latent_diffusion.solvers import DPMSolver, Euler, LCMSolver
from tests import support as S
from tests.few_step_cases import FEW_STEP_CASES, LORA_SCALE, case_inputs, lcm_lora_tensors, load_condition_scale_weight, make_solver, noise_draws, noise_generator

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_TOL = 1e-3
BF16_L2_FACTOR = 1.5  # tests/test_sam_hq_gpu.py: the margin for another accumulation order on inputs rounded to 8 bits
ROOT = Path(__file__).resolve().parent.parent
REF = next((Path(c) for c in (os.environ.get("REFINERS_SRC"), ROOT / "oracle" / "_ref" / "src") if c and (Path(c) / "refiners").exists()), Path("/nonexistent"))
MIRROR_SOLVERS = SimpleNamespace(DDIM=DDIM, DPMSolver=DPMSolver, LCMSolver=LCMSolver,
                                 euler=lambda n, spacing, prediction: Euler(n, timesteps_spacing=spacing, model_prediction_type=prediction))


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


@pytest.fixture(scope="module")
def unet_f32():
    """One float32 SDXL UNet on the GPU: the tests inject and eject their own adapters."""
    u = SDXLUNet(4, device="meta")
    S.load_mirror_weights(u, S.weights("sdxl", 0), device=DEV, dtype=torch.float32)
    return u


class _Tree:
    """The case's adapters on a UNet, taken off again on exit."""

    def __init__(self, unet, case, dtype):
        self.unet, self.case, self.dtype = unet, case, dtype
        self.adapter = self.manager = None

    def __enter__(self):
        unet, case = self.unet, self.case
        if case.get("lcm_scale") is not None:
            self.adapter = SDXLLcmAdapter(unet, condition_scale=case["lcm_scale"]).inject()
            load_condition_scale_weight(unet, device=DEV, dtype=self.dtype)
        if case["lora"]:
            self.manager = SDLoraManager(SimpleNamespace(unet=unet, device=torch.device(DEV), dtype=self.dtype))
            add_lcm_lora(self.manager, lcm_lora_tensors(S.key_shapes("sdxl")), scale=LORA_SCALE)
        return self

    def __exit__(self, *exc):
        if self.manager is not None:
            self.manager.remove_all()
        if self.adapter is not None:
            self.adapter.eject()


def _kwargs(inp):
    return dict(clip_text_embedding=inp["text"], pooled_text_embedding=inp["pooled"], time_ids=inp["time_ids"])


def _generator(case, gold, name, after_trajectories=0):
    """LCM's noise: the draws of a generator with the case's seed ARE the reference run's (asserted first, so that another generator stream is
    reported as that and not as wrong latents); the engine then draws them itself from a fresh generator, where the solver lives (the CPU)."""
    if case["solver"] != "lcm":
        return None
    for s, d in enumerate(noise_draws(case)):
        assert torch.equal(d, gold[f"{name}.noise{s}"]), "the generator's stream differs from the reference run's"
    return noise_generator(case, after_trajectories)


def _trajectory(sd, case, inp, gold, name, check=True):
    sd.set_inputs(inp["x"], generator=_generator(case, gold, name), **_kwargs(inp))
    xs = []
    for s in range(case.get("run_steps", case["steps"])):
        x = sd.step(s)
        xs.append(x.clone())
        if check:
            l2, mx = S.rel_err(x, gold[f"{name}.x{s}"])
            print(f"{name} step {s}: l2 {l2:.2e} max {mx:.2e}")
            assert l2 < F32_TOL and mx < F32_TOL, (name, s, l2, mx)
    return xs


@pytest.mark.parametrize("use_graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("name", list(FEW_STEP_CASES))
def test_float32_trajectory_matches_reference(unet_f32, name, use_graph):
    case, gold = FEW_STEP_CASES[name], S.golden("sdxl_few_step")
    inp = {k: v.to(DEV) for k, v in case_inputs(case).items()}
    with _Tree(unet_f32, case, torch.float32) as tree, warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # no whole-UNet fallback
        sd = CompiledSDXL(unet_f32, solver=make_solver(case, MIRROR_SOLVERS), condition_scale=case.get("condition_scale", 7.5), use_graph=use_graph,
                          classifier_free_guidance=case["cfg"])
        first = _trajectory(sd, case, inp, gold, name)
        st = sd.engine.stats
        assert st["fallback_nodes"] == [] and "whole_fallback" not in st
        rows = case["images"] * (2 if case["cfg"] else 1)
        assert sd.engine.io.x.shape[0] == rows and sd.engine.io.out.shape[0] == rows  # no CFG pair without guidance
        if name == "a":
            assert st["lcm_condition_scale_folded"] is True
        if case["lora"]:
            assert st["lora_sites"] > 0
        # a second trajectory with the same seed: bit-equal, the same program, the same captured graph, the prologue not run again
        low, graph, lowerings, prologues = sd.engine.low, sd.graph, st["lowerings"], sd.engine.stats["prologue_runs"]
        assert (graph is not None) == use_graph
        again = _trajectory(sd, case, inp, gold, name, check=False)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        assert sd.engine.low is low and sd.graph is graph and sd.engine.stats["lowerings"] == lowerings and sd.engine.stats["prologue_runs"] == prologues
        if case.get("alt_scale") is not None:
            # set_condition_scale on the live tree: the prologue runs once more, nothing is lowered or captured again
            tree.adapter.set_condition_scale(case["alt_scale"])
            sd.set_inputs(inp["x"], generator=_generator(case, gold, name, after_trajectories=1), **_kwargs(inp))  # (the reference run's next draw)
            l2, mx = S.rel_err(sd.step(0), gold[f"{name}.alt_x0"])
            print(f"{name} after set_condition_scale({case['alt_scale']}): l2 {l2:.2e} max {mx:.2e}")
            assert l2 < F32_TOL and mx < F32_TOL, (name, "alt_x0", l2, mx)
            assert sd.engine.low is low and sd.graph is graph and sd.engine.stats["lowerings"] == lowerings
            assert sd.engine.stats["prologue_runs"] == prologues + 1


def test_first_unet_output_matches_reference(unet_f32):
    """The UNet's own output at the first step of case a (adapter folded) and of case c (sample prediction: the 'noise' IS x0)."""
    gold = S.golden("sdxl_few_step")
    for name in ("a", "c"):
        case = FEW_STEP_CASES[name]
        inp = {k: v.to(DEV) for k, v in case_inputs(case).items()}
        with _Tree(unet_f32, case, torch.float32):
            sd = CompiledSDXL(unet_f32, solver=make_solver(case, MIRROR_SOLVERS), use_graph=False, classifier_free_guidance=False)
            sd.set_inputs(inp["x"], generator=_generator(case, gold, name), **_kwargs(inp))
            sd.step(0)
            l2, mx = S.rel_err(sd.engine.io.out, gold[f"{name}.unet_out"])
            print(f"{name} unet_out: l2 {l2:.2e} max {mx:.2e}")
            assert l2 < F32_TOL and mx < F32_TOL, (name, l2, mx)


def test_toggling_guidance_round_trip_reproduces_the_guided_golden(unet_f32):
    """True -> False -> True on ONE CompiledSDXL: the guided step after the round trip is the existing `sdxl_bare` golden, bit-equal to the step
    before it; the guidance-free step in between ran on n rows."""
    cfg = S.CASES["sdxl_bare"]
    inp = {k: v.to(DEV) for k, v in S.synth.sdxl_inputs(cfg["images"], cfg["latent_hw"], cfg["input_seed"]).items()}
    n = cfg["images"]
    sd = CompiledSDXL(unet_f32, num_inference_steps=cfg["num_steps"], condition_scale=cfg["condition_scale"])
    sd.set_inputs(inp["x"], **_kwargs(inp))
    x_before = sd.step(cfg["step"]).clone()
    l2, mx = S.rel_err(x_before, S.golden("sdxl_bare")["x_next"])
    assert l2 < F32_TOL and mx < F32_TOL and sd.engine.io.x.shape[0] == 2 * n
    sd.classifier_free_guidance = False
    assert sd.graph is None
    sd.set_inputs(inp["x"], **{k: v[n:] for k, v in _kwargs(inp).items()})
    x_free = sd.step(cfg["step"]).clone()
    assert sd.engine.io.x.shape[0] == n and not torch.equal(x_free, x_before)
    sd.classifier_free_guidance = True
    sd.set_inputs(inp["x"], **_kwargs(inp))
    x_after = sd.step(cfg["step"])
    l2, mx = S.rel_err(x_after, S.golden("sdxl_bare")["x_next"])
    print(f"guided step after the round trip vs sdxl_bare: l2 {l2:.2e} max {mx:.2e}")
    assert l2 < F32_TOL and mx < F32_TOL and torch.equal(x_after, x_before) and sd.engine.io.x.shape[0] == 2 * n


@pytest.mark.parametrize("solver", ["ddim", "euler"])
def test_guidance_free_step_is_the_guided_step_on_equal_halves(unet_f32, solver):
    """Embeddings E without guidance against [E ; E] with guidance at condition_scale 3.0: u + 3 (c - u) with c = u."""
    case = FEW_STEP_CASES["d_ddim"]
    inp = {k: v.to(DEV) for k, v in case_inputs(case).items()}
    mk = (lambda: DDIM(4)) if solver == "ddim" else (lambda: Euler(4, timesteps_spacing="trailing"))
    free = CompiledSDXL(unet_f32, solver=mk(), classifier_free_guidance=False)
    free.set_inputs(inp["x"], **_kwargs(inp))
    guided = CompiledSDXL(unet_f32, solver=mk(), condition_scale=3.0)
    guided.set_inputs(inp["x"], **{k: torch.cat((v, v)) for k, v in _kwargs(inp).items()})
    for s in range(2):
        l2, mx = S.rel_err(free.step(s), guided.step(s))
        print(f"{solver} step {s}: guidance-free vs guided on [E; E]: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < 1e-3 and mx < 1e-3, (solver, s, l2, mx)


def test_sag_adapter_gets_no_second_pass_without_guidance(unet_f32):
    """The reference evaluates Self-Attention Guidance inside the CFG branch only: with guidance off the step is the bare tree's."""
    from refiners_amd.latent_diffusion.sag import SDXLSAGAdapter

    case, gold = FEW_STEP_CASES["d_ddim"], S.golden("sdxl_few_step")
    inp = {k: v.to(DEV) for k, v in case_inputs(case).items()}
    sag = SDXLSAGAdapter(unet_f32, scale=0.75).inject()
    try:
        sd = CompiledSDXL(unet_f32, solver=DDIM(4), classifier_free_guidance=False)
        sd.set_inputs(inp["x"], **_kwargs(inp))
        l2, mx = S.rel_err(sd.step(0), gold["d_ddim.x0"])
        assert l2 < F32_TOL and mx < F32_TOL and sd.engine2 is None and sd.engine.stats["fallback_nodes"] == []
    finally:
        sag.eject()


@pytest.mark.skipif(not (REF / "refiners").exists(), reason="no refiners checkout (REFINERS_SRC / oracle/_ref)")
def test_refiners_own_tree_with_its_own_lcm_adapter():
    """Case a on refiners' OWN SDXLUNet with refiners' OWN SDXLLcmAdapter: the lowering matches nodes by class name."""
    sys.path[:0] = [p for p in (str(ROOT / "oracle" / "shim"), str(REF)) if p not in sys.path]
    from refiners.foundationals.latent_diffusion.stable_diffusion_xl.lcm import SDXLLcmAdapter as RefAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_xl.unet import SDXLUNet as RefUNet

    name = "a"
    case, gold = FEW_STEP_CASES[name], S.golden("sdxl_few_step")
    unet = RefUNet(4, device="meta")
    unet.load_state_dict({k: v.to(DEV) for k, v in S.weights("sdxl", 0).items()}, assign=True)
    adapter = RefAdapter(unet, condition_scale=case["lcm_scale"]).inject()
    load_condition_scale_weight(unet, device=DEV, dtype=torch.float32)
    assert type(unet).__module__.startswith("refiners.") and type(adapter).__module__.startswith("refiners.")
    inp = {k: v.to(DEV) for k, v in case_inputs(case).items()}
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        sd = CompiledSDXL(unet, solver=LCMSolver(case["steps"]), classifier_free_guidance=False)
        _trajectory(sd, case, inp, gold, name)
        assert sd.engine.stats["fallback_nodes"] == [] and "whole_fallback" not in sd.engine.stats and sd.engine.stats["lcm_condition_scale_folded"] is True
        lowerings = sd.engine.stats["lowerings"]
        adapter.set_condition_scale(case["alt_scale"])
        sd.set_inputs(inp["x"], generator=_generator(case, gold, name, after_trajectories=1), **_kwargs(inp))
        l2, mx = S.rel_err(sd.step(0), gold[f"{name}.alt_x0"])
        assert l2 < F32_TOL and mx < F32_TOL and sd.engine.stats["lowerings"] == lowerings


# ------------------------------------------------------------------------------------------------ bfloat16
def _unfused_bf16(unet, case, inp, gold, name):
    """The mirror's UNFUSED bfloat16 forward of the same tree on the GPU, the solver's update (its `linear_step` row, the reference's
    formulas) as bfloat16 torch operations around it, the same noise draws."""
    solver = make_solver(case, MIRROR_SOLVERS)
    bf = torch.bfloat16
    x = inp["x"].to(bf)
    draws = [d.to(DEV, bf) for d in noise_draws(case)] if case["solver"] == "lcm" else []
    with torch.no_grad():
        for s in range(case["steps"]):
            unet.set_timestep(solver.timesteps[s].unsqueeze(0).to(DEV))
            unet.set_clip_text_embedding(inp["text"].to(bf))
            unet.set_pooled_text_embedding(inp["pooled"].to(bf))
            unet.set_time_ids(inp["time_ids"])
            eps = unet(x * solver.input_scale(s))
            _hx, _he, kx, ke, _kd, kp, _sn = solver.linear_step(s)
            x = kx * x + ke * eps
            if kp != 0.0:
                x = x + kp * draws[s]
    return x


@pytest.mark.parametrize("name", ["a", "b"])
def test_bfloat16_stays_with_the_unfused_bfloat16_forward(name):
    case, gold = FEW_STEP_CASES[name], S.golden("sdxl_few_step")
    bf = torch.bfloat16
    unet = SDXLUNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sdxl", 0), device=DEV, dtype=bf)
    inp = {k: v.to(DEV) for k, v in case_inputs(case).items()}
    last = f"{name}.x{case['steps'] - 1}"
    with _Tree(unet, case, bf):
        stock = S.rel_err(_unfused_bf16(unet, case, inp, gold, name).float(), gold[last])[0]
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            sd = CompiledSDXL(unet, solver=make_solver(case, MIRROR_SOLVERS), classifier_free_guidance=False)
            xs = _trajectory(sd, case, inp, gold, name, check=False)
        assert xs[-1].dtype == bf and sd.engine.stats["fallback_nodes"] == []
        native_ = S.rel_err(xs[-1].float(), gold[last])[0]
    print(f"few-step bf16 {name}: final latents l2 against the float32 golden: unfused {stock:.4e} native {native_:.4e}")
    assert native_ <= BF16_L2_FACTOR * stock, (name, native_, stock)
