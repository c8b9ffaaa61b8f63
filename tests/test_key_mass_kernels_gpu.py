"""mi355x_attention_key_mass (csrc/attn_key_mass.hip) against float64 torch on the GPU: mass[b, j] = mean over heads, sum over queries of
softmax_j(q k^T / sqrt(D)).  The inputs are unit normals rounded to the storage dtype before the reference is formed and the output is float32, so
the project's float32 bar, max-abs error <= 1e-3 max|reference|, holds for bfloat16 storage too."""
import pytest
import torch

from refiners_amd import native
from tests.glue_cases import SENT, _fill
from tests.kernel_cases import _rand

pytestmark = pytest.mark.gpu
PAD = 5  # sentinel columns behind every mass row
#: (H, D, L, B, layout)
CASES = [
    (2, 64, 64, 1, "contiguous"),   # one tile in both passes
    (3, 160, 65, 1, "contiguous"),  # one query and one key in a second tile; heads no multiple of the waves; SD1.5's width
    (8, 40, 144, 2, "sliced"),      # q | k as column slices of one [B * L, 2 C] buffer; D padded to the MMA step; L no multiple of 16
    (5, 64, 320, 1, "contiguous"),  # five tiles in both loops: the rings are reused
    (2, 64, 96, 1, "q x 8"),        # scores far beyond what an exponential without the row maximum survives
]


def _inputs(H, D, L, B, layout, dtype):
    C = H * D
    if layout == "sliced":
        qk = _rand(B * L, 2 * C, dtype=dtype, seed=L)
        return qk[:, :C].view(B, L, C), qk[:, C:].view(B, L, C)
    return _rand(B, L, C, dtype=dtype, seed=L, scale=8.0 if layout == "q x 8" else 1.0), _rand(B, L, C, dtype=dtype, seed=L + 1)


def _launch(q, k, H):
    B, L, _ = q.shape
    mass = _fill(B, L + PAD, dtype=torch.float32, value=SENT)
    lse = _fill(B, H, L, dtype=torch.float32, value=SENT)
    native.attention_key_mass(q, k, H, None, lse, mass)
    return mass


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H, D, L, B, layout", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_key_mass_matches_float64(gpu_device, H, D, L, B, layout, dtype):
    q, k = _inputs(H, D, L, B, layout, dtype)
    qh, kh = (t.double().reshape(B, L, H, D).transpose(1, 2) for t in (q, k))
    ref = torch.softmax(qh @ kh.transpose(2, 3) * D ** -0.5, -1).mean(1).sum(1)  # [B, L]
    got = _launch(q, k, H)
    err = float((got[:, :L].double() - ref).abs().max() / ref.abs().max())
    print(f"H {H} D {D} L {L} B {B} {layout} {dtype}: {err:.2e}")
    assert err <= 1e-3
    assert bool((got[:, L:] == SENT).all()), "columns at or beyond L were written"
    assert torch.equal(got, _launch(q, k, H)), "a repeat launch differs"


@pytest.mark.parametrize("what", ["D = 168", "q misaligned"])
def test_refusals_launch_nothing(gpu_device, what):
    H, D, L = (1, 168, 64) if what == "D = 168" else (2, 64, 64)
    q, k = _rand(L * H * D + 1, dtype=torch.float32, seed=1), _rand(1, L, H * D, dtype=torch.float32, seed=2)
    q = (q[1:] if what == "q misaligned" else q[:-1]).view(1, L, H * D)
    mass, lse = _fill(1, L, dtype=torch.float32, value=SENT), _fill(1, H, L, dtype=torch.float32, value=SENT)
    with pytest.raises(native.NativeError, match="ESHAPE"):
        native.attention_key_mass(q, k, H, None, lse, mass)
    torch.cuda.synchronize()
    assert bool((mass == SENT).all()) and bool((lse == SENT).all())
