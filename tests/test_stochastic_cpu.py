"""Host side of stochastic sampling against the REAL reference's recordings (tests/golden/stochastic.safetensors + stochastic.json, written by
tools/make_golden_stochastic.py; cases in tests/stochastic_cases.py): the mirror's DPMSolver with `sigma_schedule=` / `sde_variance=`, the
nine-coefficient row mi355x_cfg_sde_step reads, `solver_tables`' refusals, Restart's timesteps and re-noising, and the binding's export list.

Bars: the mirror's `__call__` repeats the reference's float32 operations in its order, so a step from the recorded (x, eps) lands within 1e-6
relative l2 of the recorded next x (the reference's own float32 trajectory sits 1e-7 .. 8e-7 from the float64 row form); the row form evaluated in
float64 stays within 1e-5 of the float32 recording."""
import json
from enum import Enum
from types import SimpleNamespace

import pytest
import torch

from refiners_amd import native
from refiners_amd.engine.multi_diffusion import solver_tables
from refiners_amd.engine.packing import Unsupported
from refiners_amd.latent_diffusion.restart import Restart, add_noise_interval
from refiners_amd.latent_diffusion.sampling import DDIM
from refiners_amd.latent_diffusion.solvers import DPMSolver
from tests import stochastic_cases as SC
from tests import support as S

API = SimpleNamespace(DDIM=DDIM, dpm=lambda steps, first, last_first_order, sde, schedule: DPMSolver(
    steps, first_inference_step=first, last_step_first_order=last_first_order, sigma_schedule=schedule, sde_variance=1.0 if sde else 0.0))


@pytest.fixture(scope="module")
def gold():
    return S.golden("stochastic")


@pytest.fixture(scope="module")
def meta():
    return json.loads((S.GOLD / "stochastic.json").read_text())


@pytest.mark.parametrize("schedule", SC.TABLE_SCHEDULES, ids=str)
@pytest.mark.parametrize("steps", SC.TABLE_STEPS)
def test_tables_match_the_reference(steps, schedule, meta):
    want = meta["tables"][f"{steps}.{schedule}"]
    for sde in (0.0, 1.0):  # (the draw changes no table)
        solver = DPMSolver(steps, sigma_schedule=schedule, sde_variance=sde)
        assert [int(t) for t in solver.timesteps] == want["timesteps"]
        got, ref = solver.sigmas.double(), torch.tensor(want["sigmas"], dtype=torch.float64)
        worst = float(((got - ref).abs() / ref.abs()).max())
        print(f"{steps} steps, {schedule}: sigmas worst relative difference {worst:.2e}")
        assert got.shape == ref.shape and worst < 1e-6, worst


@pytest.mark.parametrize("name", SC.TRAJECTORIES)
def test_mirror_call_follows_the_recorded_trajectory(name, gold, meta):
    case = SC.CASES[name]
    solver = SC.make_solver(name, API)
    assert [int(t) for t in solver.timesteps] == meta["timesteps"][name]
    g, g2 = SC.generator(name), SC.generator(name)
    x = SC.inputs(name)["x"]
    for s in SC.run_steps(name):
        got = solver(x, gold[f"{name}.eps{s}"], s, generator=g)
        err = S.rel_err(got, gold[f"{name}.x{s}"])[0]
        print(f"{name} step {s}: mirror __call__ l2 {err:.2e}")
        assert err < 1e-6, (name, s, err)
        if case["sde"]:  # one draw per step, the last one included: the recorded stream, draw for draw
            assert torch.equal(torch.randn(x.shape, generator=g2), gold[f"{name}.noise{s}"])
        x = gold[f"{name}.x{s}"]
    assert torch.equal(g.get_state(), g2.get_state()) or not case["sde"], "the mirror drew more or less than once per step"
    if not case["sde"]:
        assert torch.equal(g.get_state(), SC.generator(name).get_state()), "a deterministic solver must leave the generator alone"


@pytest.mark.parametrize("name", SC.TRAJECTORIES)
def test_row_form_in_float64_follows_the_recorded_trajectory(name, gold):
    case = SC.CASES[name]
    solver = SC.make_solver(name, API)
    x = SC.inputs(name)["x"].double()
    hist = torch.zeros_like(x)
    for s in SC.run_steps(name):
        row = solver.linear_step(s)
        assert len(row) == (8 if case["sde"] else 7) and all(map(lambda v: v == v and abs(v) != float("inf"), row)), row
        hx, he, kx, ke, kd, kp, s_next = row[:7]
        kn = row[7] if case["sde"] else 0.0
        eps = gold[f"{name}.eps{s}"].double()
        noise = gold[f"{name}.noise{s}"].double() if case["sde"] else torch.zeros_like(x)
        d = hx * x + he * eps
        got = kx * x + ke * eps + kd * d + kp * hist + kn * noise
        err = S.rel_err(got, gold[f"{name}.x{s}"])[0]
        print(f"{name} step {s}: row form (float64) l2 {err:.2e}")
        assert err < 1e-5 and s_next == 1.0, (name, s, err)
        hist, x = d, gold[f"{name}.x{s}"].double()


@pytest.mark.parametrize("sde", [0.0, 1.0], ids=["ode", "sde"])
@pytest.mark.parametrize("schedule", [s for s in SC.TABLE_SCHEDULES if s], ids=str)
@pytest.mark.parametrize("steps", SC.TABLE_STEPS)
def test_last_step_of_a_schedule_has_finite_coefficients_and_no_ratio_term(steps, schedule, sde):
    """The last two sigmas coincide to float32 precision: r = x / 0.  The reference's tensors turn the term into 0; so does the row."""
    solver = DPMSolver(steps, sigma_schedule=schedule, sde_variance=sde)
    for s in range(steps):
        row = solver.linear_step(s)
        assert all(v == v and abs(v) != float("inf") for v in row), (s, row)
    last = solver.linear_step(steps - 1)
    assert last[5] == 0.0, last
    a, _, lam = (t.tolist() for t in solver._tables64)
    f = 1.0 - torch.exp(torch.tensor((2.0 if sde else 1.0) * (lam[steps - 1] - lam[steps]), dtype=torch.float64)).item()
    assert last[4] == a[steps] * f  # kd without its 0.5 / r part


def _todays_row(solver, step):
    """DPMSolver.linear_step as it stood before `sigma_schedule=` / `sde_variance=` existed."""
    import numpy as np

    a, n, lam = (t.tolist() for t in solver._tables64)
    hx, he = 1.0 / a[step], -n[step] / a[step]
    f = 1.0 - float(np.exp(lam[step] - lam[step + 1]))
    kx = n[step + 1] / n[step]
    if solver._first_order(step):
        return (hx, he, kx, 0.0, f * a[step + 1], 0.0, 1.0)
    r = (lam[step] - lam[step - 1]) / (lam[step + 1] - lam[step])
    half = 0.5 * a[step + 1] * f / r
    return (hx, he, kx, 0.0, a[step + 1] * f + half, -half, 1.0)


@pytest.mark.parametrize("kw", [dict(), dict(first_inference_step=2, last_step_first_order=True), dict(timesteps_spacing="trailing")], ids=["plain", "late_first_order", "trailing"])
def test_defaults_reproduce_todays_rows_exactly(kw):
    for steps in (4, 6, 30):
        plain, explicit = DPMSolver(steps, **kw), DPMSolver(steps, sigma_schedule=None, sde_variance=0.0, **kw)
        assert not plain.stochastic and plain.sigma_schedule is None and not hasattr(DPMSolver, "needs_noise")
        for s in range(plain.first_inference_step, steps):
            assert plain.linear_step(s) == _todays_row(plain, s) == explicit.linear_step(s), (steps, s)


def test_only_the_two_variances_of_the_reference():
    with pytest.raises(NotImplementedError, match="sde_variance=0.0 or 1.0"):
        DPMSolver(6, sde_variance=0.5)
    with pytest.raises(AssertionError):
        DPMSolver(6, sigma_schedule="cosine")


def test_solver_tables_keeps_the_deterministic_mirror_and_refuses_the_sde_form():
    for kw in (dict(), dict(sigma_schedule="karras")):
        solver = DPMSolver(6, **kw)
        assert solver_tables(solver) is solver
    for kw in (dict(), dict(sigma_schedule="karras")):
        with pytest.raises(Unsupported, match="draws noise per step"):
            solver_tables(DPMSolver(6, sde_variance=1.0, **kw))


def test_solver_tables_restates_a_karras_solver_of_the_reference(meta):
    class NoiseSchedule(str, Enum):
        KARRAS = "karras"

    class DPMSolver_(object):  # the attributes solver_tables reads of refiners' own class
        pass

    DPMSolver_.__name__ = "DPMSolver"
    ref = DPMSolver_()
    ref.num_inference_steps, ref.first_inference_step, ref.last_step_first_order = 6, 0, False
    ref.params = SimpleNamespace(sde_variance=0.0, sigma_schedule=NoiseSchedule.KARRAS, timesteps_spacing=SimpleNamespace(value="custom"))
    ref.timesteps = torch.tensor(meta["tables"]["6.karras"]["timesteps"])
    mine = solver_tables(ref)
    assert isinstance(mine, DPMSolver) and mine.sigma_schedule == "karras" and torch.equal(mine.timesteps.long(), ref.timesteps.long())
    ref.params.sde_variance = 1.0
    with pytest.raises(Unsupported, match="draws noise per step"):
        solver_tables(ref)


def test_restart_timesteps_and_renoising(gold, meta):
    case = SC.CASES["restart"]
    ldm = SimpleNamespace(solver=DDIM(case["steps"]), device=torch.device("cpu"), dtype=torch.float32)
    restart = Restart(ldm, num_steps=case["num_steps"], num_iterations=case["num_iterations"])
    want = meta["restart"]
    assert (restart.start_step, restart.end_timestep) == (want["start_step"], want["end_timestep"])
    assert restart.timesteps.dtype == torch.int64 and restart.timesteps.tolist() == want["timesteps"]
    assert (Restart(ldm).num_steps, Restart(ldm).num_iterations, Restart(ldm).start_time, Restart(ldm).end_time) == (10, 2, 0.1, 2)
    ts = restart.timesteps
    start = gold[f"restart.x{case['steps'] - 1}"]
    for k in range(case["num_iterations"]):
        got = add_noise_interval(DDIM(case["steps"]), x=start, noise=gold[f"restart.r{k}.noise"], initial_timestep=ts[-1], target_timestep=ts[0])
        err = S.rel_err(got, gold[f"restart.r{k}.noised"])[0]
        print(f"restart iteration {k}: add_noise_interval l2 {err:.2e}")
        assert err < 1e-6, (k, err)
        start = gold[f"restart.r{k}.x{len(ts) - 2}"]
    with pytest.raises(AssertionError, match="only works with DDIM"):
        Restart(SimpleNamespace(solver=DPMSolver(10), device=torch.device("cpu"), dtype=torch.float32))


def test_restart_call_draws_from_the_given_generator(gold):
    """The mirror's loop over a stand-in denoiser that returns x unchanged: two draws, the recorded ones, and the caller's solver put back."""
    case = SC.CASES["restart"]

    class Ldm:
        device, dtype = torch.device("cpu"), torch.float32

        def __init__(self):
            self.solver, self.calls = DDIM(case["steps"]), []

        def __call__(self, x, step, **kw):
            self.calls.append((step, self.solver.timesteps.tolist()))
            return x

    ldm = Ldm()
    mine = ldm.solver
    restart = Restart(ldm, num_steps=case["num_steps"], num_iterations=1)
    x0 = gold[f"restart.x{case['steps'] - 1}"]
    got = restart(x0, clip_text_embedding=torch.zeros(2, 77, 768), generator=SC.generator("restart"))
    assert S.rel_err(got, gold["restart.r0.noised"])[0] < 1e-6
    assert ldm.solver is mine and [c[0] for c in ldm.calls] == [0, 1, 2] and ldm.calls[0][1] == restart.timesteps.tolist()


def test_the_binding_reads_the_new_header():
    for sym in ("mi355x_cfg_sde_step", "mi355x_sde_step"):  # (the header's names and exports: tests/test_abi_header_cpu.py)
        restype, argtypes = native.ABIS["sde_step"].functions[sym]
        assert len(argtypes) == 9
