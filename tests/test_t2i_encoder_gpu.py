"""pytest -m gpu: CompiledT2IConditionEncoder against the reference's fixtures (tests/golden/t2i_encoder.safetensors): float32 within the project's
1e-3 bar on every feature map (both figures of support.rel_err), direct and replayed; bfloat16 no less accurate than the mirror's unfused bfloat16
torch forward of the same tree; the SD1UNet + SD1T2IAdapter step on stock and on compiled features; a tree of the reference's own classes."""
import os
import sys
import warnings
from pathlib import Path

import pytest
import torch

import refiners_amd
from refiners_amd.engine import CompiledT2IConditionEncoder
from refiners_amd.engine.compiled import CompiledUNet
from refiners_amd.latent_diffusion import t2i as M
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from tests import support as S
from tests import t2i_encoder_cases as TC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32_TOL = 1e-3
LAUNCHES = {"sd1": 1 + 16 + 2 + 3 + 4, "xl": 1 + 8 + 2 + 1 + 4}


@pytest.fixture(scope="module")
def gold():
    return S.golden("t2i_encoder")


def _worst(feats, gold, case):
    errs = [S.rel_err(f, gold[f"{case}.f{i}"]) for i, f in enumerate(feats)]
    return max(e[0] for e in errs), max(e[1] for e in errs)


@pytest.mark.parametrize("case", list(TC.ENCODER_CASES))
def test_float32_matches_the_reference(gpu_device, case, gold):
    fast = CompiledT2IConditionEncoder(TC.encoder(case, M, device=DEV))
    x = TC.picture(case).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # a fallback to the stock forward is a failure here
        feats = fast(x)
    assert fast.stats["fallback_nodes"] == [] and not fast.stats["whole_fallback"] and fast.stats["step_ops"] == LAUNCHES[case]
    assert all(f.is_contiguous() and tuple(f.shape) == tuple(gold[f"{case}.f{i}"].shape) for i, f in enumerate(feats))
    l2, mx = _worst(feats, gold, case)
    print(case, "float32", f"l2 {l2:.2e} max {mx:.2e}")
    assert l2 <= F32_TOL and mx <= F32_TOL
    again = fast(x)  # the graph replay equals the direct run bit for bit, and again on a second replay
    assert fast.program.graph is not None and all(torch.equal(a, b) for a, b in zip(feats, again)) and all(torch.equal(a, b) for a, b in zip(feats, fast(x)))


@pytest.mark.parametrize("case", list(TC.ENCODER_CASES))
def test_bfloat16_no_worse_than_unfused_torch(gpu_device, case, gold):
    enc = TC.encoder(case, M, device=DEV, dtype=torch.bfloat16)
    fast = CompiledT2IConditionEncoder(enc)
    x = TC.picture(case).to(DEV, torch.bfloat16)
    feats = fast(x)
    assert not fast.stats["whole_fallback"]
    with torch.no_grad():
        stock = enc(x)
    a, b = _worst(feats, gold, case)[0], _worst(stock, gold, case)[0]
    print(f"{case} bf16: engine l2 {a:.3e}; torch-bf16 unfused l2 {b:.3e}; ratio {a / b:.3f}")
    assert a <= 1.15 * b, (case, a, b)


def test_sd1_step_on_stock_and_on_compiled_features(gpu_device, gold):
    unet = SD1UNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sd1", TC.SD1_STEP["unet_seed"]), device=DEV)
    adapter = TC.sd1_adapter(unet, refiners_amd.namespace().SD1T2IAdapter, device=DEV)
    fast_unet = CompiledUNet(unet)
    stock = tuple(f.to(DEV) for f in (gold[f"sd1_step.f{i}"] for i in range(4)))
    y = TC.sd1_run(unet, stock, device=DEV, call=fast_unet).clone()
    assert fast_unet.stats.get("t2i_sites") == 4 and fast_unet.stats["fallback_nodes"] == []
    assert max(S.rel_err(y, gold["sd1_step.out"])) <= F32_TOL
    fast = CompiledT2IConditionEncoder(adapter.condition_encoder)
    feats = fast(TC.sd1_inputs()["picture"].to(DEV))
    assert not fast.stats["whole_fallback"] and max(max(S.rel_err(f, s)) for f, s in zip(feats, stock)) <= F32_TOL
    adapter.set_condition_features(feats)  # end to end: the compiled encoder's tuple goes in unchanged
    y2 = TC.sd1_run(unet, feats, device=DEV, call=fast_unet)
    assert max(S.rel_err(y2, gold["sd1_step.out"])) <= F32_TOL


REF = Path(os.environ.get("REFINERS_SRC") or Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "src")


@pytest.mark.skipif(not (REF / "refiners").exists(), reason="no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
def test_refiners_own_encoder_runs_natively(gpu_device, gold):
    sys.path[:0] = [str(Path(__file__).resolve().parent.parent / "oracle" / "shim"), str(REF)]
    import refiners.foundationals.latent_diffusion.t2i_adapter as ref_t2i

    fast = CompiledT2IConditionEncoder(TC.encoder("xl", ref_t2i, device=DEV))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        feats = fast(TC.picture("xl").to(DEV))
    l2, mx = _worst(feats, gold, "xl")
    assert fast.stats["fallback_nodes"] == [] and fast.stats["step_ops"] == LAUNCHES["xl"] and l2 <= F32_TOL and mx <= F32_TOL, (l2, mx)
