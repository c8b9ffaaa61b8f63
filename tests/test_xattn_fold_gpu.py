"""pytest -m gpu: the golden trees stepped with the cross-attention fold (REFINERS_AMD_XATTN_FOLD) on and off.  The fused launch computes what the two
launches compute with the same arithmetic and the same rounding points (tests/test_gemm_xattn_kernels_gpu.py: bit-equal), so the two programs' outputs
are expected to be identical, and each passes the bar the golden has in tests/test_engine_gpu.py."""
import pytest
import torch

from refiners_amd.engine.compiled import CompiledUNet
from tests import support as S
from tests.test_engine_gpu import BF16_TOL, build, set_context

pytestmark = pytest.mark.gpu
# folded sites per tree at the golden's latent size: token counts that are a multiple of 64 (a 24 x 16 latent has 96 and 24 tokens: nothing folds)
CASES = {"sdxl_bare": 70, "sdxl_lora_ip": 70, "sdxl_control": None, "sdxl_control2": 0, "sdxl_conv_lora": None}


@pytest.mark.parametrize("case", list(CASES))
def test_step_with_and_without_the_fold(case, monkeypatch, gpu_device):
    cfg, unet, _specs, _handles, inp = build(case, torch.bfloat16)
    x = torch.cat((inp["x"], inp["x"])).to(torch.bfloat16)
    gold = S.golden(case)["unet_out"]
    outs, sites, ops = {}, {}, {}
    for lever in ("0", "1"):
        monkeypatch.setenv("REFINERS_AMD_XATTN_FOLD", lever)
        fast = CompiledUNet(unet)
        set_context(unet, cfg, inp, torch.bfloat16)
        outs[lever] = fast(x).clone()
        sites[lever], ops[lever] = fast.stats.get("xattn_fold_sites", 0), fast.stats["step_ops"]
        assert fast.stats["fallback_nodes"] == []
        l2, mx = S.rel_err(outs[lever].float(), gold)
        print(f"{case} bf16 fold {lever}: l2 {l2:.3e} max {mx:.3e}, {ops[lever]} launches, {sites[lever]} folded sites")
        assert l2 < BF16_TOL, (case, lever, l2, mx)
        del fast
    assert sites["0"] == 0 and ops["1"] == ops["0"] - sites["1"]
    if CASES[case] is not None:
        assert sites["1"] == CASES[case]
    else:
        assert sites["1"] > 0
    differ = (outs["0"] != outs["1"]).float().mean().item()
    print(f"{case}: {differ:.2%} of the elements differ between the two programs")
    assert torch.equal(outs["0"], outs["1"])
