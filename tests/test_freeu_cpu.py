"""FreeU without a GPU: the host tables of mi355x_freeu_filter and the mirror's fourier_filter against torch.fft, the dry lowering of the
adapter's two sites behind REFINERS_AMD_FREEU, and the mirror adapter against what the reference's own class recorded (tests/golden/freeu_keys.json)."""
import json
import math

import pytest
import torch

from refiners_amd.engine import freeu as T
from refiners_amd.engine.packing import Unsupported
from refiners_amd.engine.unet_lowering import UNetIO, UNetLowering
from refiners_amd.latent_diffusion.freeu import fourier_filter
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from tests import freeu_cases as P
from tests import support as S


@pytest.mark.parametrize("scale", [0.9, 0.2])
@pytest.mark.parametrize("hw", [(32, 32), (4, 4), (5, 7), (38, 26), (2, 3), (8, 16)])
def test_tables_are_the_fourier_filter(hw, scale):
    H, W = hw
    x = torch.randn((2, 3, H, W), dtype=torch.float64, generator=torch.Generator().manual_seed(H * 100 + W))
    pl, wt = T.planes(H, W)
    rows = x.reshape(6, H * W)
    got = rows + (scale - 1.0) * (rows @ pl.T) * wt @ pl
    assert (got.reshape(x.shape) - fourier_filter(x, scale)).abs().max() <= 1e-10
    A, S_, R = T.tables(H, W, scale)
    assert R == pl.shape[0] == (7 if min(H, W) >= 3 else 6) and A.shape == S_.shape == (16, -(-H * W // 128) * 128)
    assert not A[R:].any() and not A[:, H * W:].any() and not S_[R:].any() and not S_[:, H * W:].any()
    f32 = rows + (rows @ A[:, : H * W].double().T) @ S_[:, : H * W].double()  # the tables as the kernel gets them, rounded to float32
    assert (f32.reshape(x.shape) - fourier_filter(x, scale)).abs().max() <= 1e-5


def test_tables_refuse_what_does_not_fit():
    for args in [(1, 8, 0.5), (8, 1, 0.5), (16, 16, 0.5, 2)]:  # a 1-wide plane; rank 23 at threshold 2
        with pytest.raises(Unsupported):
            T.tables(*args)


def test_mirror_filter_at_threshold_two():
    """out = Re(ifft2(mask * fft2(x))), the mask = scale on the frequencies {-2 .. 1} of both axes, written out as a sum over them."""
    H, W, scale = 8, 16, 0.3
    x = torch.randn((1, 2, H, W), dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    i, j = torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64)
    want = x.clone()
    for u in range(-2, 2):
        for v in range(-2, 2):
            e = torch.exp(2j * math.pi * (u * i[:, None] / H + v * j[None, :] / W))
            coeff = (x * e.conj()).sum(dim=(-2, -1), keepdim=True) / (H * W)
            want += (scale - 1.0) * (coeff * e).real
    assert (fourier_filter(x, scale, threshold=2) - want).abs().max() <= 1e-10


def _dry(unet, dtype=torch.float32):
    dev, (h, w) = torch.device("meta"), P.CASES["sd1"]["latent_hw"]
    io = UNetIO(x=torch.empty(2, 4, h, w, device=dev, dtype=dtype), timestep=torch.empty(2, device=dev), out=torch.empty(2, 4, h, w, device=dev, dtype=dtype))
    io.tokens[("cross_attention_block", "clip_text_embedding")] = (torch.zeros(2 * 128, 768, device=dev, dtype=dtype), 77)
    low = UNetLowering(dev, dtype)
    low.lower(unet, io)
    return low, [what for fn, _args, what, _keep in low.step if fn is not None]


def test_dry_lowering_behind_the_switch(monkeypatch):
    monkeypatch.delenv("REFINERS_AMD_FREEU", raising=False)
    _low, bare = _dry(SD1UNet(4, device="meta"))
    unet = SD1UNet(4, device="meta")
    adapter = P.inject(unet, P.mirror_api(), "sd1", S.key_shapes("sd1"), device="meta")
    with pytest.raises(Unsupported, match="FreeUResidualConcatenator"):
        _dry(unet)
    monkeypatch.setenv("REFINERS_AMD_FREEU", "1")
    low, names = _dry(unet)
    assert low.stats["freeu_sites"] == 2 and low.stats["fallback_nodes"] == [] and "whole_fallback" not in low.stats
    assert names.count("mi355x_freeu_filter") == 2 and len(names) == len(bare) + 2  # one launch per site; the concatenation is still never written
    adapter.eject()
    low, names = _dry(unet)
    assert names == bare and "freeu_sites" not in low.stats


@pytest.mark.parametrize("family", ["sd1", "sdxl"])
def test_repr_and_state_dict_keys_are_the_references(family):
    from refiners_amd.latent_diffusion.sdxl import SDXLUNet

    want = json.loads((S.GOLD / "freeu_keys.json").read_text())[family]
    unet = (SD1UNet if family == "sd1" else SDXLUNet)(4, device="meta")
    adapter = P.inject(unet, P.mirror_api(), family, S.key_shapes(family), device="meta")
    assert P.repr_digest(adapter) == want["repr_sha256"] and list(adapter.state_dict()) == want["state_dict"]
    adapter.eject()
    assert P.repr_digest(unet) == P.repr_digest((SD1UNet if family == "sd1" else SDXLUNet)(4, device="meta"))
