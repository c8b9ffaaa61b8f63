"""pytest -m gpu: IP-Adapter on SD1.5 on the MI355X against what the reference's own SD1UNet + SD1IPAdapter computed on CPU (tests/golden/sd1_ip*,
tools/make_golden_sd1_ip.py).  Every cross-attention site is ONE mi355x_attention_streams launch (text + image keys).  float32 bar: the project's,
relative l2 and max <= 1e-3; bfloat16: at most 1.15 x the error of the mirror's unfused bfloat16 forward of the same tree on the same GPU."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import refiners_amd
from refiners_amd import synth
from refiners_amd.engine.compiled import CompiledSDXL, CompiledUNet
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from refiners_amd.latent_diffusion.solvers import DPMSolver
from tests import sd1_ip_cases as P
from tests import support as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F32_TOL = 1e-3


@pytest.fixture(scope="module")
def gold():
    return S.golden("sd1_ip")


def _within(got, ref, what, tol=F32_TOL):
    l2, mx = S.rel_err(got, ref)
    print(f"{what}: l2 {l2:.2e} max {mx:.2e}")
    assert l2 <= tol and mx <= tol, (what, l2, mx)


def _tree(case, dtype=torch.float32):
    unet = SD1UNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sd1", P.UNET["weight_seed"]), device="cuda", dtype=dtype)
    return unet, P.inject(unet, refiners_amd.namespace(), case, S.key_shapes("sd1"), device="cuda", dtype=dtype)


def _run(fast, unet, case, ts, dtype=torch.float32):
    inp = P.inputs(case)
    unet.set_clip_text_embedding(inp["text"].to("cuda", dtype))
    unet.set_timestep(torch.tensor([ts], device="cuda"))
    return fast(inp["x"].to("cuda", dtype).expand(2, -1, -1, -1).contiguous())


@pytest.mark.parametrize("case", list(P.CASES))
def test_unet_with_the_adapter_matches_the_reference(gpu_device, case, gold):
    unet, adapter = _tree(case)
    fast = CompiledUNet(unet)
    ts = P.CASES[case]["timesteps"]
    direct = _run(fast, unet, case, ts[0]).clone()
    _within(direct, gold[f"{case}.unet_out.t0"], f"{case} t0 direct")
    replayed = _run(fast, unet, case, ts[0])
    assert torch.equal(direct, replayed) and fast.graph is not None
    assert fast.stats["fallback_nodes"] == [] and fast.stats["ip_sites"] == 16 and fast.stats["attn_streams_sites"] == 16
    for i, t in enumerate(ts[1:], 1):
        _within(_run(fast, unet, case, t), gold[f"{case}.unet_out.t{i}"], f"{case} t{i} (graph replay)")
    if "rescale" in P.CASES[case]:  # a scale assigned after lowering reaches the launches
        adapter.scale = P.CASES[case]["rescale"]
        _within(_run(fast, unet, case, ts[0]), gold[f"{case}.unet_out.rescaled"], f"{case} rescaled")
        _within(_run(fast, unet, case, ts[0]), gold[f"{case}.unet_out.rescaled"], f"{case} rescaled (graph replay)")
        assert fast.stats["attn_streams_sites"] == 16


def test_one_solver_step_through_the_sampling_engine(gpu_device, gold):
    unet, _adapter = _tree("plain")
    inp = {k: v.cuda() for k, v in P.inputs("plain").items()}
    pipe = CompiledSDXL(unet, condition_scale=P.SOLVER["condition_scale"], solver=DPMSolver(P.SOLVER["num_steps"], device="cuda"))
    pipe.set_inputs(inp["x"], clip_text_embedding=inp["text"], clip_image_embedding=inp["tokens"])
    _within(pipe.step(P.SOLVER["step"]), gold["plain.x_next"], "DPM-Solver++ step")
    st = pipe.engine.stats
    assert st["fallback_nodes"] == [] and st["ip_sites"] == st["attn_streams_sites"]  # (16 per program: the CFG pair may run as two)


def test_eject_returns_to_the_bare_program(gpu_device, gold):
    unet, adapter = _tree("plain")
    fast = CompiledUNet(unet)
    _within(_run(fast, unet, "plain", 500.0), gold["plain.unet_out.t0"], "before eject")
    adapter.eject()
    unet.set_context("ip_adapter", {"clip_image_embedding": None})  # (the pair's image tokens: sd1_bare is one sample)
    cfg = S.CASES["sd1_bare"]
    unet.set_clip_text_embedding(torch.randn((1, 77, 768), generator=synth._gen("in.text", cfg["input_seed"])).cuda())
    unet.set_timestep(torch.tensor([cfg["timestep"]], device="cuda"))
    _within(fast(torch.randn((1, 4, *cfg["latent_hw"]), generator=synth._gen("in.x", cfg["input_seed"])).cuda()), S.golden("sd1_bare")["unet_out"], "ejected: sd1_bare")
    assert "attn_streams_sites" not in fast.stats and fast.stats["ip_sites"] == 0 and fast.stats["fallback_nodes"] == []


def test_bfloat16_step_against_the_unfused_chain(gpu_device, gold):
    unet, _adapter = _tree("plain", torch.bfloat16)
    fast = CompiledUNet(unet)
    y = _run(fast, unet, "plain", 500.0, torch.bfloat16)
    assert fast.stats["fallback_nodes"] == [] and fast.stats["attn_streams_sites"] == 16
    chain = P.run_chain(unet, "plain", 500.0, device="cuda", dtype=torch.bfloat16)
    mine, stock = S.rel_err(y, gold["plain.unet_out.t0"]), S.rel_err(chain, gold["plain.unet_out.t0"])
    print(f"bf16 against the float32 reference: lowered l2 {mine[0]:.3e} max {mine[1]:.3e} | unfused Chain l2 {stock[0]:.3e} max {stock[1]:.3e}")
    assert torch.isfinite(y.float()).all() and mine[0] <= 1.15 * stock[0]


_CHILD = """
import json, sys, torch
sys.path.insert(0, {root!r})
import refiners_amd
from refiners_amd.engine.compiled import CompiledUNet
from tests import test_sd1_ip_gpu as T
unet, _ = T._tree("plain")
fast = CompiledUNet(unet)
y = T._run(fast, unet, "plain", 500.0)
names = [e[2] for e in fast.low.step if e[0] is not None]
torch.save(y.cpu(), sys.argv[1])
print(json.dumps({{"launches": len(names), "streams": names.count("mi355x_attention_streams"), "sites": fast.stats.get("attn_streams_sites", 0)}}))
"""


def test_switch_keeps_the_three_launch_form(gpu_device, tmp_path):
    """REFINERS_AMD_ATTN_STREAMS is read once, so each form is lowered in a fresh process: 16 sites x (3 - 1) more launches, the same output."""
    got = {}
    for flag in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=str(ROOT)), str(tmp_path / f"y{flag}.pt")], env=dict(os.environ, REFINERS_AMD_ATTN_STREAMS=flag),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(ROOT), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[flag] = json.loads(r.stdout.strip().splitlines()[-1])
    assert (got["1"]["streams"], got["1"]["sites"], got["0"]["streams"], got["0"]["sites"]) == (16, 16, 0, 0)
    assert got["0"]["launches"] == got["1"]["launches"] + 32
    l2, _mx = S.rel_err(torch.load(tmp_path / "y0.pt"), torch.load(tmp_path / "y1.pt"))
    print(f"three-launch form against the fused form, float32: l2 {l2:.2e}")
    assert l2 <= 1e-5
