"""pytest -m gpu: stochastic sampling on the MI355X -- `CompiledSDXL` under the mirror's DPMSolver with `sde_variance=1.0` and / or a sigma
schedule, and `CompiledSDXL.restart`, on an SD1UNet of synthetic weights against the REAL reference's trajectories
(tests/golden/stochastic.*, tools/make_golden_stochastic.py; cases in tests/stochastic_cases.py), in direct replay and as a captured graph.

The draws come from a CPU generator of the case's seed -- the stream the reference run drew from -- so the float32 goldens pin the GPU trajectory
step by step.  Float32 bar: the project's (tests/test_engine_gpu.py): relative l2 and relative maximum < 1e-3 at EVERY recorded step.
bfloat16 (case `sde`): the result is finite and gated the way tests/test_few_step_gpu.py gates it -- its error against the float32 golden is at
most BF16_L2_FACTOR x that of the mirror's UNFUSED bfloat16 forward of the same tree with the same draws on the same GPU."""
import json
import warnings
from types import SimpleNamespace

import pytest
import torch

from refiners_amd import native
from refiners_amd.engine.compiled import CompiledSDXL
from refiners_amd.latent_diffusion.sampling import DDIM
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from refiners_amd.latent_diffusion.solvers import DPMSolver
from tests import stochastic_cases as SC
from tests import support as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_TOL = 1e-3
BF16_L2_FACTOR = 1.5  # tests/test_few_step_gpu.py
API = SimpleNamespace(DDIM=DDIM, dpm=lambda steps, first, last_first_order, sde, schedule: DPMSolver(
    steps, first_inference_step=first, last_step_first_order=last_first_order, sigma_schedule=schedule, sde_variance=1.0 if sde else 0.0))


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


@pytest.fixture(scope="module")
def gold():
    return S.golden("stochastic")


@pytest.fixture(scope="module")
def meta():
    return json.loads((S.GOLD / "stochastic.json").read_text())


def _unet(dtype=torch.float32):
    u = SD1UNet(4, device="meta")
    S.load_mirror_weights(u, S.weights("sd1", SC.SEED["weight_seed"]), device=DEV, dtype=dtype)
    return u


@pytest.fixture(scope="module")
def unet():
    return _unet()


def _engine(unet, name, use_graph):
    case = SC.CASES[name]
    return CompiledSDXL(unet, solver=SC.make_solver(name, API), condition_scale=case["scale"], use_graph=use_graph, classifier_free_guidance=case["cfg"])


def _stage(sd, name, **kw):
    inp = {k: v.to(DEV) for k, v in SC.inputs(name).items()}
    sd.set_inputs(inp["x"], clip_text_embedding=inp["text"], generator=SC.generator(name), **kw)


@pytest.mark.parametrize("use_graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("name", SC.TRAJECTORIES)
def test_float32_trajectory_matches_reference(name, use_graph, gold, unet):
    case, lowered = SC.CASES[name], SC.lowered(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # no whole-UNet fallback ...
        sd = _engine(unet, name, use_graph)
        _stage(sd, name)
        assert sd.sde == case["sde"] and sd.coef_table.shape[1] == (9 if case["sde"] else 8) and sd.coef.numel() == sd.coef_table.shape[1]
        for s in SC.run_steps(name):
            if not lowered and s == case["first"]:
                # ... except at latents the UNet's three halvings do not divide, which no solver gets lowered at: the stock Chain forward with its
                # warning, and the update (draw included) still on the native kernel
                with pytest.warns(RuntimeWarning, match="only exact 2x nearest upsampling is lowered"):
                    x = sd.step(s)
            else:
                x = sd.step(s)
            l2, mx = S.rel_err(x, gold[f"{name}.x{s}"])
            print(f"{name} step {s}: l2 {l2:.2e} max {mx:.2e}")
            assert l2 < F32_TOL and mx < F32_TOL, (name, s, l2, mx)
            if case["sde"]:
                assert torch.equal(sd.sde_noise.cpu(), gold[f"{name}.noise{s}"]), "the step's draw is the reference's"
    st = sd.engine.stats
    if not lowered:
        assert "whole_fallback" in st and sd.graph is None
        return
    assert st["fallback_nodes"] == [] and "whole_fallback" not in st
    if use_graph:
        assert sd.graph is not None
        # the same trajectory again: the same program, the same captured graph, the same buffers, the same draws -- bit-equal
        low, graph, lowerings, buf = sd.engine.low, sd.graph, st["lowerings"], sd.sde_noise.data_ptr()
        first = sd.x.clone()
        _stage(sd, name)
        assert sd.sample() is sd.x
        assert torch.equal(sd.x, first) and sd.engine.low is low and sd.graph is graph and sd.engine.stats["lowerings"] == lowerings and sd.sde_noise.data_ptr() == buf


def test_every_step_draws_once_the_last_one_included(unet):
    """A caller who shares the generator finds the stream where the reference leaves it: steps x one draw of the latents' shape."""
    name = "sde"
    sd = _engine(unet, name, True)
    _stage(sd, name)
    g, g2 = sd.generator, SC.generator(name)
    sd.sample()
    for _ in SC.run_steps(name):
        torch.randn(tuple(sd.x.shape), generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())
    # a generator on the latents' device draws there: what the reference's own call does (torch.randn(x.shape, generator=..., device=x.device))
    gd, gd2 = torch.Generator(device=DEV).manual_seed(5), torch.Generator(device=DEV).manual_seed(5)
    inp = {k: v.to(DEV) for k, v in SC.inputs(name).items()}
    sd.set_inputs(inp["x"], clip_text_embedding=inp["text"], generator=gd)
    sd.step(0)
    assert torch.equal(sd.sde_noise, torch.randn(tuple(sd.x.shape), generator=gd2, device=DEV))


def test_restart_matches_reference_and_leaves_the_engine_as_it_was(gold, meta, unet):
    name = "restart"
    case = SC.CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        sd = _engine(unet, name, True)
        _stage(sd, name)
        sd.sample()
        last = case["steps"] - 1
        l2, mx = S.rel_err(sd.x, gold[f"{name}.x{last}"])
        print(f"restart: DDIM trajectory l2 {l2:.2e} max {mx:.2e}")
        assert l2 < F32_TOL and mx < F32_TOL, (l2, mx)
        mine, table, graph = sd.solver, sd.coef_table, sd.graph
        restart = SimpleNamespace(timesteps=torch.tensor(meta["restart"]["timesteps"]), num_iterations=1)
        g = SC.generator(name)
        per = len(restart.timesteps) - 1
        for k in range(case["num_iterations"]):  # one iteration per call, so that every iteration's end is compared
            x = sd.restart(restart, generator=g)
            assert torch.equal(sd.sde_noise.cpu(), gold[f"{name}.r{k}.noise"])
            l2, mx = S.rel_err(x, gold[f"{name}.r{k}.x{per - 1}"])
            print(f"restart iteration {k}: l2 {l2:.2e} max {mx:.2e}")
            assert l2 < F32_TOL and mx < F32_TOL, (k, l2, mx)
            assert sd.solver is mine and sd.coef_table is table and sd.graph is graph and graph is not None
        # both iterations in one call, from the DDIM trajectory's end
        sd.x.copy_(gold[f"{name}.x{last}"].to(DEV))
        x = sd.restart(SimpleNamespace(timesteps=restart.timesteps, num_iterations=case["num_iterations"]), generator=SC.generator(name))
        l2, mx = S.rel_err(x, gold[f"{name}.r{case['num_iterations'] - 1}.x{per - 1}"])
        print(f"restart, {case['num_iterations']} iterations in one call: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < F32_TOL and mx < F32_TOL, (l2, mx)
        # an ordinary trajectory afterwards: the caller's solver, table and graph
        _stage(sd, name)
        sd.sample()
        l2, mx = S.rel_err(sd.x, gold[f"{name}.x{last}"])
        assert l2 < F32_TOL and mx < F32_TOL and sd.graph is graph and sd.solver is mine, (l2, mx)
    assert sd.engine.stats["fallback_nodes"] == [] and "whole_fallback" not in sd.engine.stats


def test_restart_needs_ddim(unet):
    sd = _engine(unet, "sde", False)
    _stage(sd, "sde")
    with pytest.raises(AssertionError, match="only works with DDIM"):
        sd.restart(SimpleNamespace(timesteps=torch.tensor([500, 300, 100]), num_iterations=1))


def _unfused_bf16(unet, name, draws):
    """The mirror's UNFUSED bfloat16 forward of the same tree on the GPU, guidance and the solver's row as bfloat16 torch operations around it."""
    case, solver = SC.CASES[name], SC.make_solver(name, API)
    bf = torch.bfloat16
    inp = {k: v.to(DEV, bf) for k, v in SC.inputs(name).items()}
    x, hist = inp["x"], torch.zeros_like(inp["x"])
    with torch.no_grad():
        for s in SC.run_steps(name):
            unet.set_timestep(solver.timesteps[s].unsqueeze(0).to(DEV))
            unet.set_clip_text_embedding(inp["text"])
            u, c = unet(torch.cat((x, x))).chunk(2)
            eps = u + case["scale"] * (c - u)
            hx, he, kx, ke, kd, kp, _sn, kn = solver.linear_step(s)
            d = hx * x + he * eps
            x, hist = kx * x + ke * eps + kd * d + kp * hist + kn * draws[s], d
    return x


def test_bfloat16_stays_with_the_unfused_bfloat16_forward(gold):
    name, bf = "sde", torch.bfloat16
    unet = _unet(bf)
    g = SC.generator(name)
    shape = tuple(SC.inputs(name)["x"].shape)
    draws = {s: torch.randn(shape, generator=g, dtype=bf).to(DEV) for s in SC.run_steps(name)}  # as the engine draws them: x's dtype
    last = f"{name}.x{SC.CASES[name]['steps'] - 1}"
    stock = S.rel_err(_unfused_bf16(unet, name, draws).float(), gold[last])[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        sd = _engine(unet, name, True)
        _stage(sd, name)
        x = sd.sample()
    assert x.dtype == bf and bool(torch.isfinite(x).all()) and sd.engine.stats["fallback_nodes"] == []
    assert torch.equal(sd.sde_noise, draws[SC.CASES[name]["steps"] - 1])
    native_ = S.rel_err(x.float(), gold[last])[0]
    print(f"sde bf16: final latents l2 against the float32 golden: unfused {stock:.4e} native {native_:.4e}")
    assert native_ <= BF16_L2_FACTOR * stock, (native_, stock)


def test_combinations_without_a_golden_are_refused(unet):
    from refiners_amd.latent_diffusion.sag import SD1SAGAdapter

    name = "sde"
    sd = _engine(unet, name, False)
    h, w = SC.CASES[name]["hw"]
    _stage(sd, name, input_condition=torch.zeros(1, 4, h, w, device=DEV))
    with pytest.raises(AssertionError, match="stochastic DPMSolver.*input_condition.*mi355x_cond_step has no noise operand"):
        sd.step(0)
    _stage(sd, name)
    sag = SD1SAGAdapter(target=unet, scale=0.75).inject()
    try:
        with pytest.raises(AssertionError, match="stochastic DPMSolver.*Self-Attention Guidance"):
            sd.step(0)
    finally:
        sag.eject()
    # the deterministic form of the same solver is not refused on either account (the existing inpainting and SAG tests run it)
    assert not CompiledSDXL(unet, solver=DPMSolver(6, sigma_schedule="karras")).sde
