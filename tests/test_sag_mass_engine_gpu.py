"""pytest -m gpu: the Self-Attention Guidance tap as one mi355x_attention_key_mass call (LoweredBlocks.sag_attention_mass).  SD1.5's middle block
has 8 heads of 160, which the GEMM -> softmax -> column-sum chain cannot take in bfloat16: that tree lowers only through the fused call.  On SDXL
in float32 both forms evaluate the same q and k, so the chain is the yardstick for the fused call's `mass`."""
import pytest
import torch

from refiners_amd.engine import lowering_blocks
from refiners_amd.engine.compiled import CompiledSDXL
from refiners_amd.latent_diffusion.sag import SD1SAGAdapter, SDXLSAGAdapter
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from refiners_amd.latent_diffusion.sdxl import SDXLUNet
from tests import support as S

pytestmark = pytest.mark.gpu


def _names(low):
    return [e[2] for e in low.step if e[0] is not None]


def test_sd1_self_attention_guidance_lowers_in_bfloat16(gpu_device):
    bf = torch.bfloat16
    unet = SD1UNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sd1", 0), device="cuda", dtype=bf)
    SD1SAGAdapter(target=unet, scale=0.75).inject()
    x = torch.randn((1, 4, 32, 32), generator=S.synth._gen("in.x", 3)).to("cuda", bf)
    text = torch.randn((2, 77, 768), generator=S.synth._gen("in.text", 3)).to("cuda", bf)
    for use_graph in (False, True):
        sd = CompiledSDXL(unet, num_inference_steps=30, condition_scale=5.0, use_graph=use_graph)
        sd.set_inputs(x, clip_text_embedding=text)
        out = sd.step(11)
        names, low = _names(sd.engine.low), sd.engine.low
        assert sd.engine.stats["fallback_nodes"] == [] and sd.engine2.stats["fallback_nodes"] == [] and sd.engine.stats["sag_mass_fused"] is True
        assert names.count("mi355x_attention_key_mass") == 1 and "mi355x_softmax_rows" not in names and "mi355x_colsum_rows" not in names
        assert bool(torch.isfinite(out.float()).all())
        mass, L = low.sag["mass"], low.sag["tokens"]
        print(f"SD1.5 SAG bf16 graph={use_graph}: L {L}, mass rows sum to {mass.sum(1).tolist()}")
        assert tuple(mass.shape) == (1, L) and bool(((mass.sum(1) - L).abs() <= 1e-3 * L).all())  # every softmax row sums to 1


def test_sdxl_fused_tap_against_the_chain(gpu_device, monkeypatch):
    from tests.golden_cases import SAG_CASE as CFG

    unet = SDXLUNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sdxl", CFG["weight_seed"]), device="cuda", dtype=torch.float32)
    SDXLSAGAdapter(target=unet, scale=CFG["sag_scale"]).inject()
    inp = {k: v.cuda() for k, v in S.synth.sdxl_inputs(1, CFG["latent_hw"], CFG["input_seed"]).items()}
    mass, names = {}, {}
    for on in (True, False):  # (a program keeps the form it was lowered with)
        monkeypatch.setattr(lowering_blocks, "SAG_MASS", on)
        sd = CompiledSDXL(unet, num_inference_steps=CFG["num_steps"], condition_scale=CFG["condition_scale"], use_graph=False)
        sd.set_inputs(inp["x"], clip_text_embedding=inp["text"], pooled_text_embedding=inp["pooled"], time_ids=inp["time_ids"])
        sd.step(CFG["step"])
        assert sd.engine.stats["fallback_nodes"] == [] and sd.engine.stats.get("sag_mass_fused", False) is on
        mass[on], names[on] = sd.engine.low.sag["mass"].clone(), _names(sd.engine.low)
    n, heads = mass[True].shape[0], 20
    err = float((mass[True] - mass[False]).abs().max() / mass[False].abs().max())
    print(f"SDXL SAG f32: fused mass against the chain's {err:.2e}; tap launches {3 * n * heads} -> 1")
    assert err <= 1e-4
    assert names[True].count("mi355x_attention_key_mass") == 1 and "mi355x_colsum_rows" not in names[True]
    assert names[False].count("mi355x_softmax_rows") == names[False].count("mi355x_colsum_rows") == n * heads
    assert len(names[False]) - len(names[True]) == 3 * n * heads - 1
