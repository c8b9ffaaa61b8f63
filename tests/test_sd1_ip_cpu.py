"""IP-Adapter on SD1.5 without a GPU: the mirror's SD1IPAdapter against what the reference's own class recorded (tests/golden/sd1_ip*, written by
tools/make_golden_sd1_ip.py), and the dry lowering of its cross-attention sites."""
import json

import pytest
import torch

import refiners_amd
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from tests import sd1_ip_cases as P
from tests import support as S


@pytest.mark.parametrize("case", ["plain", "plus"])
def test_repr_and_state_dict_keys_are_the_references(case):
    want = json.loads((S.GOLD / "sd1_ip_keys.json").read_text())[case]
    adapter = P.inject(SD1UNet(4, device="meta"), refiners_amd.namespace(), case, S.key_shapes("sd1"), device="meta")
    assert P.repr_digest(adapter) == want["repr_sha256"]
    assert list(adapter.state_dict()) == want["state_dict"] and list(adapter.image_proj.state_dict()) == want["image_proj"]
    assert adapter.image_proj.state_dict()[want["image_proj"][-1]].shape[-1] == 768 and len(adapter.sub_adapters) == 16


def test_mirror_forward_matches_the_reference():
    unet = SD1UNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sd1", P.UNET["weight_seed"]))
    P.inject(unet, refiners_amd.namespace(), "plain", S.key_shapes("sd1"))
    l2, mx = S.rel_err(P.run_chain(unet, "plain", P.CASES["plain"]["timesteps"][0]), S.golden("sd1_ip")["plain.unet_out.t0"])
    print(f"mirror Chain forward, CPU float32: l2 {l2:.2e} max {mx:.2e}")
    assert l2 <= 1e-5 and mx <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dry_lowering_has_one_streams_launch_per_cross_attention(dtype):
    from refiners_amd.engine.unet_lowering import UNetIO, UNetLowering

    dev, B = torch.device("meta"), P.UNET["batch"]
    unet = SD1UNet(4, device="meta", dtype=dtype)
    P.inject(unet, refiners_amd.namespace(), "plain", S.key_shapes("sd1"), device=dev, dtype=dtype)
    io = UNetIO(x=torch.empty(B, 4, 32, 32, device=dev, dtype=dtype), timestep=torch.empty(B, device=dev), out=torch.empty(B, 4, 32, 32, device=dev, dtype=dtype))
    io.tokens[("cross_attention_block", "clip_text_embedding")] = (torch.zeros(B * 128, 768, device=dev, dtype=dtype), 77)
    io.tokens[("ip_adapter", "clip_image_embedding")] = (torch.zeros(B * 64, 768, device=dev, dtype=dtype), 4)
    low = UNetLowering(dev, dtype)
    low.lower(unet, io)
    names = [what for fn, _args, what, _keep in low.step if fn is not None]
    bare = json.loads((S.GOLD / "ella_bare_programs.json").read_text())[f"sd1_{str(dtype).split('.')[1]}"]["step"]
    assert low.stats["fallback_nodes"] == [] and low.stats["ip_sites"] == 16 and low.stats["attn_streams_sites"] == 16
    assert names.count("mi355x_attention_streams") == 16 and names.count("mi355x_attention_general") == 16  # (the self-attentions keep theirs)
    assert names.count("mi355x_axpby") == bare["counts"].get("mi355x_axpby", 0) and len(names) == bare["launches"]  # a fused site costs what a bare one does
