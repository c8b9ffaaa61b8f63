"""pytest -m gpu: CompiledTiledVAE against the real reference's tiled_inference (tests/golden/tiled_vae.*, cases of tests/tiled_vae_cases.py).

Bounds: float32 at the bar the VAE tests of tests/test_engine_gpu.py use (F32_TOL on both figures of tests/support.rel_err), for the frozen statistics as
for the images and latents; bf16 decode at the 3e-2 l2 of test_vae_decoder_matches_reference, against the float32 golden."""
import json

import pytest
import torch

import refiners_amd.fluxion.layers as fl
import tests.support as S
from refiners_amd import CompiledTiledVAE
from refiners_amd.latent_diffusion.vae import FixedGroupNorm, SDXLAutoencoder
from tests.tiled_vae_cases import TILE, TILED_VAE_CASES, WEIGHT_SEED, image_tensor

pytestmark = pytest.mark.gpu
F32_TOL = 1e-3
BF16_TOL = 3e-2


@pytest.fixture(scope="module")
def gold(gpu_device):
    return S.golden("tiled_vae")


def _vae(dtype=torch.float32):
    shapes = {k: tuple(v) for k, v in json.loads((S.GOLD / "vae_keys.json").read_text()).items()}
    m = SDXLAutoencoder(device="meta")
    m.load_state_dict({k: v.to("cuda", dtype) for k, v in S.synth.synth_state_dict(shapes, WEIGHT_SEED).items()}, assign=True)
    return m


@pytest.fixture(scope="module")
def vae(gpu_device):
    return _vae()


def _close(got, ref, what, tol=F32_TOL, both=True):
    l2, mx = S.rel_err(got.float(), ref)
    print(f"tiled vae {what}: l2 {l2:.2e} max {mx:.2e}")
    assert l2 < tol and (mx < tol or not both), (what, l2, mx)


def _check_case(eng, name, gold, what):
    case = TILED_VAE_CASES[name]
    dec = eng.decode(gold[f"{name}.latents"].cuda())
    assert eng.stats["fallback_nodes"] == [] and eng.stats["tiles"] == case["grid"][0] * case["grid"][1] and not eng.stats["graph_replayed"]
    assert eng.stats["gn_launches_per_program"] == 30
    _close(dec, gold[f"{name}.decoded"], f"{what} {name} decode")
    again = eng.decode(gold[f"{name}.latents"].cuda())
    assert eng.stats["graph_replayed"] and torch.equal(dec, again)
    enc = eng.encode(image_tensor(gold[f"{name}.image_u8"]).cuda())
    assert eng.stats["fallback_nodes"] == [] and eng.stats["gn_launches_per_program"] == 22
    _close(enc, gold[f"{name}.encoded"], f"{what} {name} encode")
    assert torch.equal(enc, eng.encode(image_tensor(gold[f"{name}.image_u8"]).cuda())) and eng.stats["graph_replayed"]
    return dec, enc


@pytest.mark.parametrize("name", list(TILED_VAE_CASES))
def test_calibrate_encode_decode_match_the_reference(name, gold, vae):
    """calibrate() on the recorded tensor reproduces the reference's FixedGroupNorm statistics; decode and encode reproduce its tiled results; the second
    call of a shape replays the captured graph with the same bits; tile_batch 1 and 4 give the same bits."""
    case = TILED_VAE_CASES[name]
    eng = CompiledTiledVAE(vae, tile_size=TILE, blending=case["blending"], tile_batch=4)
    with pytest.raises(ValueError):
        eng.decode(gold[f"{name}.latents"].cuda())
    eng.calibrate(gold[f"{name}.calibration"].cuda())
    mean, var = eng.statistics()
    _close(mean, gold[f"{name}.gn_mean"], f"{name} gn mean")
    _close(var, gold[f"{name}.gn_var"], f"{name} gn var")
    dec, enc = _check_case(eng, name, gold, "calibrated")
    one = CompiledTiledVAE(vae, tile_size=TILE, blending=case["blending"], tile_batch=1)
    one.calibrate(gold[f"{name}.calibration"].cuda())
    assert torch.equal(one.decode(gold[f"{name}.latents"].cuda()), dec) and torch.equal(one.encode(image_tensor(gold[f"{name}.image_u8"]).cuda()), enc)
    if case["grid"] != (1, 1):
        assert len(one.stats["tile_groups"]) == case["grid"][0] * case["grid"][1] and all(n == 1 for _s, n in one.stats["tile_groups"])


@pytest.mark.parametrize("name", list(TILED_VAE_CASES))
def test_adopted_statistics_match_the_reference(name, gold, vae):
    """adopt() on a mirror tree whose FixedGroupNorms hold the GOLDEN statistics: apply and blend without the engine's own calibration."""
    case = TILED_VAE_CASES[name]
    fixed = [FixedGroupNorm(gn).inject(parent) for gn, parent in list(vae.walk(fl.GroupNorm))]
    try:
        assert len(fixed) == gold[f"{name}.gn_mean"].shape[0]
        for f, m, v in zip([f for f, _ in vae.walk(FixedGroupNorm)], gold[f"{name}.gn_mean"], gold[f"{name}.gn_var"]):
            f.mean, f.var = m.cuda(), v.cuda()
        eng = CompiledTiledVAE(vae, tile_size=TILE, blending=case["blending"])
        eng.adopt()
        _check_case(eng, name, gold, "adopted")
        assert len(list(vae.walk(FixedGroupNorm))) == len(fixed)  # the lowering put the adapters back
    finally:
        vae._remove_fixed_group_norm()


def test_bf16_decode_of_case_a(gold):
    """bf16 weights, activations and canvas against the float32 golden (the l2 figure is printed before it is asserted)."""
    m = _vae(torch.bfloat16)
    eng = CompiledTiledVAE(m, tile_size=TILE, blending=TILED_VAE_CASES["a"]["blending"])
    eng.calibrate(gold["a.calibration"].cuda().to(torch.bfloat16))
    dec = eng.decode(gold["a.latents"].cuda().to(torch.bfloat16))
    assert eng.stats["fallback_nodes"] == [] and dec.dtype == torch.bfloat16
    _close(dec, gold["a.decoded"], "bf16 a decode", tol=BF16_TOL, both=False)
