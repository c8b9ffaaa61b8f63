"""The T2I-Adapter condition encoder on the CPU: the mirror against the reference's fixtures (tests/golden/t2i_encoder.safetensors, t2i_keys.json),
SD1T2IAdapter's inject / eject / duplicate-name assertion and its lowering, dry-run lowerings of the encoder on the meta device, the fallback."""
import json
import warnings
from collections import Counter

import pytest
import torch

import refiners_amd
from refiners_amd.engine import CompiledT2IConditionEncoder
from refiners_amd.engine import t2i as ET
from refiners_amd.engine.unet_lowering import UNetIO, UNetLowering
from refiners_amd.latent_diffusion import t2i as M
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from tests import support as S
from tests import t2i_encoder_cases as TC

F32_TOL = 1e-3


@pytest.fixture(scope="module")
def gold():
    return S.golden("t2i_encoder")


@pytest.mark.parametrize("case", list(TC.ENCODER_CASES))
def test_mirror_encoder_matches_the_reference(case, gold):
    with torch.no_grad():
        feats = TC.encoder(case, M)(TC.picture(case))
    assert len(feats) == 4
    for i, f in enumerate(feats):
        l2, mx = S.rel_err(f, gold[f"{case}.f{i}"])
        assert tuple(f.shape) == tuple(gold[f"{case}.f{i}"].shape) and l2 <= F32_TOL and mx <= F32_TOL, (case, i, l2, mx)


def test_state_dict_keys_equal_the_reference():
    want = {k: tuple(v) for k, v in json.loads((S.GOLD / "t2i_keys.json").read_text()).items()}
    assert {k: tuple(v.shape) for k, v in M.ConditionEncoderXL(device="meta").state_dict().items()} == want
    sd1 = {k: tuple(v.shape) for k, v in M.ConditionEncoder(device="meta").state_dict().items()}
    assert list(sd1) == list(want) and sd1["Conv2d.weight"] == (320, 192, 3, 3)


def test_sd1_adapter_injects_ejects_and_lowers():
    unet = SD1UNet(4, device="meta", dtype=torch.bfloat16)
    bare = repr(unet)
    adapter = refiners_amd.namespace().SD1T2IAdapter(unet, name="depth", scale=0.5).inject()
    taps = list(unet.layers(M.T2IFeatures))
    assert [t.index for t in taps] == [0, 1, 2, 3] and adapter.residual_indices == (2, 5, 8, 11)
    with pytest.raises(AssertionError, match="already injected"):
        M.SD1T2IAdapter(unet, name="depth").inject()
    dev, dt = torch.device("meta"), torch.bfloat16
    e = lambda *shape, dtype=dt: torch.empty(*shape, device=dev, dtype=dtype)  # noqa: E731
    io = UNetIO(x=e(2, 4, 32, 32), timestep=e(2, dtype=torch.float32), out=e(2, 4, 32, 32))
    io.tokens[("cross_attention_block", "clip_text_embedding")] = (e(256, 768), 77)
    io.t2i["depth"] = [e(1, 320, 32, 32), e(1, 640, 16, 16), e(1, 1280, 8, 8), e(1, 1280, 4, 4)]
    low = UNetLowering(dev, dt, None, "merged")
    low.lower(unet, io)
    assert low.stats.get("t2i_sites") == 4 and low.stats["fallback_nodes"] == []
    adapter.eject()
    assert repr(unet) == bare and list(unet.layers(M.T2IFeatures)) == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", list(TC.ENCODER_CASES))
def test_dry_lowering_has_the_expected_launches(case, dtype):
    c = TC.ENCODER_CASES[case]
    enc = getattr(M, c["cls"])(**c["kw"], device="meta", dtype=dtype)
    B, _cin, Hp, Wp = c["shape"]
    outs = [torch.empty(s, device="meta", dtype=dtype) for s in ET.feature_shapes(enc, B, Hp, Wp)]
    low = ET.lower(enc, torch.empty(c["shape"], device="meta", dtype=dtype), outs)
    blocks = 4 * c["kw"]["num_residual_blocks"]
    shortcuts, pools = (2, 3) if case == "sd1" else (2, 1)
    # 1 stem + 2 per block (3x3 convolution, 1x1 GEMM with the residual) + shortcuts + pools + 4 output transposes
    assert Counter(e[2] for e in low.step) == {"mi355x_t2i_stem": 1, "mi355x_gemm(conv)": blocks, "mi355x_gemm": blocks + shortcuts, "mi355x_t2i_pool": pools, "mi355x_nhwc_to_nchw": 4}
    assert low.stats["fallback_nodes"] == [] and low.prologue == []
    convs = [e[1][0]._obj for e in low.step if e[2] == "mi355x_gemm(conv)"]
    assert all(g.geglu == 4 and g.seg[0].ksize == 3 for g in convs)  # the ReLU rides in the convolution's epilogue
    assert [o.shape[1] for o in outs] == list(TC.CHANNELS)


def test_an_indivisible_picture_falls_back_before_any_launch():
    enc = TC.encoder("sd1", M)
    fast = CompiledT2IConditionEncoder(enc)
    x = torch.rand(1, 3, 64, 72 + 4)
    with pytest.warns(RuntimeWarning, match="not a multiple of the downscale factor 8"):
        with pytest.raises(RuntimeError):  # the stock forward: PixelUnshuffle's own error
            fast(x)
    assert fast.stats["whole_fallback"] and fast.lowerings == 0 and fast.program is None
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # the refusal is remembered
        with pytest.raises(RuntimeError):
            fast(x)
