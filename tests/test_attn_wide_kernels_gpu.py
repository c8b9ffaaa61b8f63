"""mi355x_attention_general on head widths above (160, 160): the wide-head kernel (csrc/attn_wide_kernel.cuh) against softmax(scale * Q K^T [causal]) V
computed in float64 from the same (already rounded) inputs, at the bars of tests/kernel_cases._tol.

Measured on an MI355X (max-abs error relative to the reference's max-abs; docs/MEASUREMENTS_attn_wide.md has every case): float32 at most 2e-6,
bfloat16 at most 4e-3."""
import math

import pytest
import torch

from refiners_amd import native
from tests.kernel_cases import _cmp

pytestmark = pytest.mark.gpu

B, H = 2, 2
WIDTHS = [(512, 512), (320, 320), (168, 488)]
LENGTHS = [(40, 150), (130, 56), (64, 64)]
#: (Dqk, Dv, Lq, Lk, causal, spike)
CASES = [(dqk, dv, lq, lk, False, False) for dqk, dv in WIDTHS for lq, lk in LENGTHS] + [(512, 512, 40, 150, False, True), (512, 512, 150, 150, True, False)]


def _strided(rows, width, dtype, seed, scale=1.0):
    """[B, rows, width] as a view of a wider, longer buffer: batch, row and head offsets all differ from the dense ones."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = (torch.randn(B, rows + 3, width + 24, generator=g) * scale).to(device="cuda", dtype=dtype)
    return buf[:, 1 : rows + 1, 8 : width + 8]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dqk,dv,lq,lk,causal,spike", CASES)
def test_wide_attention_matches_float64(gpu_device, dqk, dv, lq, lk, causal, spike, dtype):
    q, k, v = _strided(lq, H * dqk, dtype, 1), _strided(lk, H * dqk, dtype, 2), _strided(lk, H * dv, dtype, 3)
    if spike:  # (kernel_cases.attention_general_case: two keys whose scores stand ~30 above the rest, one of them in the last tile)
        k[:, lk - 3] *= 6.0
        k[:, lk // 2] *= 4.0
    lkp = (lk + 63) // 64 * 64
    vt = torch.zeros(H * dv, B, lkp + 64, dtype=dtype, device="cuda")[:, :, :lkp]  # (rows longer than the padded length: ldvt != B * Lkp)
    vt[:, :, :lk] = v.permute(2, 0, 1)
    out = torch.full((B, lq + 2, H * dv + 8), float("nan"), dtype=dtype, device="cuda")[:, 1 : lq + 1, 4 : H * dv + 4]
    native.attention_general(q, k, vt, out, H, lk, causal=causal)

    qh, kh, vh = (t.double().reshape(B, -1, H, d).transpose(1, 2) for t, d in ((q, dqk), (k, dqk), (v, dv)))
    logits = qh @ kh.transpose(-1, -2) / math.sqrt(dqk)
    if causal:
        logits = logits.masked_fill(~torch.ones(lq, lk, dtype=torch.bool, device="cuda").tril(), float("-inf"))
    ref = (torch.softmax(logits, dim=-1) @ vh).transpose(1, 2).reshape(B, lq, H * dv)
    err, scale, tol = _cmp(out, ref, dtype)
    print(f"attn_wide {dtype} ({dqk},{dv}) L ({lq},{lk}) causal {causal} spike {spike}: rel {err / scale:.2e}")
    assert err <= tol * scale, (err, scale)
    assert torch.isnan(out._base[:, 0]).all() and torch.isnan(out._base[:, lq + 1]).all() and torch.isnan(out._base[:, :, :4]).all() and torch.isnan(out._base[:, :, H * dv + 4 :]).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_boundary_of_the_wide_kernel(gpu_device, dtype):
    """Above 512 nothing serves the request; (160, 160) still runs on the instance it always ran on (bit-stable against itself)."""
    q, k = _strided(64, 520, dtype, 4), _strided(64, 520, dtype, 5)
    vt = torch.zeros(64, B, 64, dtype=dtype, device="cuda")
    with pytest.raises(native.NativeError, match="ESHAPE|-2"):
        native.attention_general(q, k, vt, torch.empty(B, 64, 64, dtype=dtype, device="cuda"), 1, 64)
    q, k = _strided(130, 160, dtype, 6), _strided(150, 160, dtype, 7)
    vt = torch.randn(160, B, 192, device="cuda").to(dtype)
    a, b = (native.attention_general(q, k, vt, torch.empty(B, 130, 160, dtype=dtype, device="cuda"), 1, 150) for _ in range(2))
    assert torch.equal(a, b) and torch.isfinite(a.float()).all()
