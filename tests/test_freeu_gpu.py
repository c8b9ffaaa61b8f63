"""pytest -m gpu: FreeU on the MI355X against what the reference's own UNets + SDFreeUAdapter computed on CPU (tests/golden/freeu*,
tools/make_golden_freeu.py), with REFINERS_AMD_FREEU=1: each FreeUResidualConcatenator is ONE mi355x_freeu_filter launch.  float32 bar: the project's,
relative l2 and max <= 1e-3; bfloat16: at most 1.15 x the error of the mirror's unfused bfloat16 forward of the same tree on the same GPU."""
import pytest
import torch

from refiners_amd.engine.compiled import CompiledSDXL, CompiledUNet
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from refiners_amd.latent_diffusion.sdxl import SDXLUNet
from refiners_amd.latent_diffusion.sampling import DDIM
from tests import freeu_cases as P
from tests import support as S

pytestmark = pytest.mark.gpu
F32_TOL = 1e-3


@pytest.fixture(scope="module")
def gold():
    return S.golden("freeu")


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    monkeypatch.setenv("REFINERS_AMD_FREEU", "1")


def _within(got, ref, what, tol=F32_TOL):
    l2, mx = S.rel_err(got, ref)
    print(f"{what}: l2 {l2:.2e} max {mx:.2e}")
    assert l2 <= tol and mx <= tol, (what, l2, mx)


def _tree(case, dtype=torch.float32):
    c = P.CASES[case]
    unet = (SDXLUNet if c["family"] == "sdxl" else SD1UNet)(4, device="meta")
    S.load_mirror_weights(unet, S.weights(c["family"], c["weight_seed"]), device="cuda", dtype=dtype)
    return unet, P.inject(unet, P.mirror_api(), case, S.key_shapes(c["family"]), device="cuda", dtype=dtype)


def _timesteps(case):
    c = P.CASES[case]
    return [float(DDIM(c["num_steps"]).timesteps[c["step"]])] if c["family"] == "sdxl" else c["timesteps"]


def _run(fast, unet, case, ts, dtype=torch.float32):
    P.set_context(unet, case, ts, "cuda", dtype)
    return fast(P.pair(case, "cuda", dtype))


@pytest.mark.parametrize("case", list(P.CASES))
def test_unet_with_the_adapter_matches_the_reference(gpu_device, case, gold):
    unet, _adapter = _tree(case)
    fast = CompiledUNet(unet)
    ts = _timesteps(case)
    direct = _run(fast, unet, case, ts[0]).clone()
    _within(direct, gold[f"{case}.unet_out.t0"], f"{case} t0 direct")
    replayed = _run(fast, unet, case, ts[0])
    assert torch.equal(direct, replayed) and fast.graph is not None
    assert fast.stats["fallback_nodes"] == [] and fast.stats["freeu_sites"] == 2 and not fast.stats.get("whole_fallback")
    for i, t in enumerate(ts[1:], 1):
        _within(_run(fast, unet, case, t), gold[f"{case}.unet_out.t{i}"], f"{case} t{i} (graph replay)")


def test_bfloat16_step_against_the_unfused_chain(gpu_device, gold):
    unet, _adapter = _tree("sd1", torch.bfloat16)
    fast = CompiledUNet(unet)
    y = _run(fast, unet, "sd1", 500.0, torch.bfloat16)
    assert fast.stats["fallback_nodes"] == [] and fast.stats["freeu_sites"] == 2
    chain = P.run_chain(unet, "sd1", 500.0, device="cuda", dtype=torch.bfloat16)
    mine, stock = S.rel_err(y, gold["sd1.unet_out.t0"]), S.rel_err(chain, gold["sd1.unet_out.t0"])
    print(f"bf16 against the float32 reference: lowered l2 {mine[0]:.3e} max {mine[1]:.3e} | unfused Chain l2 {stock[0]:.3e} max {stock[1]:.3e}")
    assert torch.isfinite(y.float()).all() and mine[0] <= 1.15 * stock[0]


def test_one_sdxl_step_injected_then_ejected(gpu_device, gold):
    c = P.CASES["sdxl"]
    unet, adapter = _tree("sdxl")
    inp = {k: v.cuda() for k, v in P.inputs("sdxl").items()}
    sd = CompiledSDXL(unet, num_inference_steps=c["num_steps"], condition_scale=c["condition_scale"])
    sd.set_inputs(inp["x"], clip_text_embedding=inp["text"], pooled_text_embedding=inp["pooled"], time_ids=inp["time_ids"])
    _within(sd.step(c["step"]), gold["sdxl.x_next"], "DDIM step with FreeU")
    assert sd.engine.stats["fallback_nodes"] == [] and sd.engine.stats["freeu_sites"] == 2
    adapter.eject()
    bare = S.CASES["sdxl_bare"]
    inp = {k: v.cuda() for k, v in S.synth.sdxl_inputs(bare["images"], bare["latent_hw"], bare["input_seed"]).items()}
    sd = CompiledSDXL(unet, num_inference_steps=bare["num_steps"], condition_scale=bare["condition_scale"])
    sd.set_inputs(inp["x"], clip_text_embedding=inp["text"], pooled_text_embedding=inp["pooled"], time_ids=inp["time_ids"])
    _within(sd.step(bare["step"]), S.golden("sdxl_bare")["x_next"], "ejected: sdxl_bare")
    assert "freeu_sites" not in sd.engine.stats and sd.engine.stats["fallback_nodes"] == []
