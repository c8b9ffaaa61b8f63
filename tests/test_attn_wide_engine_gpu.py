"""The autoencoder's mid-block attention (Residual(GroupNorm, SelfAttention2d), one head of 512 channels) through the VAE lowering and the tiled VAE
lowering: one fused mi355x_attention_general launch, no score matrix and no row softmax, within the VAE tests' float32 bar of torch's own forward."""
import pytest
import torch

import tests.support as S
from refiners_amd import native
from refiners_amd.engine.packing import Act, PackCache
from refiners_amd.engine.tiled_vae import NodeStats, TiledVAELowering
from refiners_amd.engine.vae import VAEDecoderLowering
from refiners_amd.latent_diffusion.vae import _attention

pytestmark = pytest.mark.gpu
C = 512


@pytest.fixture(scope="module")
def block(gpu_device):
    torch.manual_seed(0)
    node = _attention(C, dict(device="cuda", dtype=torch.float32))
    gn = node[0]
    with torch.no_grad():
        gn.weight.copy_(1 + 0.2 * torch.randn(C))
        gn.bias.copy_(0.2 * torch.randn(C))
    return node


@pytest.mark.parametrize("hw", [(16, 16), (8, 7)], ids=["16x16", "8x7"])
@pytest.mark.parametrize("tiled", [False, True], ids=["plain", "tiled"])
@torch.no_grad()
def test_mid_block_attention_is_one_fused_launch(block, tiled, hw):
    gn, att = block[0], block[1]
    x = torch.randn(2, C, *hw, device="cuda")
    if tiled:  # frozen statistics (FixedGroupNorm): every group normalised with mean 0.1, variance 1.5
        mean, var = 0.1, 1.5
        gain = gn.weight / (var + gn.eps) ** 0.5
        tab = torch.stack((torch.full_like(gain, mean), gain), dim=1).contiguous()
        low = TiledVAELowering(x.device, x.dtype, PackCache(), {id(gn): NodeStats(gn, tab, torch.tensor([[mean, var]] * gn.num_groups, device="cuda"))}, "fixed")
        ref = x + att((x - mean) * gain.view(1, -1, 1, 1) + gn.bias.view(1, -1, 1, 1))
    else:
        low = VAEDecoderLowering(x.device, x.dtype, PackCache())
        ref = block(x)
    with low.in_step():
        out = low.attention_2d(block, Act(x.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), 2, *hw))
    native.replay(low.step)
    got = out.t.view(2, *hw, C).permute(0, 3, 1, 2)
    l2, mx = S.rel_err(got, ref)
    print(f"mid-block attention tiled={tiled} {hw}: l2 {l2:.2e} max {mx:.2e}")
    assert l2 < 1e-3 and mx < 1e-3, (l2, mx)
    names = [e[2] for e in low.step]
    wide = [e[1][0]._obj for e in low.step if e[2] == "mi355x_attention_general"]
    assert [(a.Dqk, a.Dv, a.B) for a in wide] == [(C, C, 2)] and "mi355x_softmax_rows" not in names and low.stats["fallback_nodes"] == []
