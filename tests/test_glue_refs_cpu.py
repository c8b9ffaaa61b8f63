"""The references of tests/glue_cases.py that need no GPU, checked on their own.

  * nearest_cells_f32 -- the float32 cell formula sag_degrade_kernel uses, min(floor(dst * (float(n_in) / float(n_out))), n_in - 1) -- is what
    F.interpolate(mode="nearest") does for every 1 <= n_in <= n_out <= 512; the integer formula dst * n_in / n_out it replaced is not (rows
    61 of 122 from 16 cells and 99 of 198 from 50, the sizes the GPU cases use).
  * sag_reference equals a direct transcription of SAGAdapter.compute_degraded_latents' steps with the package's own gaussian_blur.
  * relpos_gather_ref gives the decomposed relative-position bias when its output multiplies K' = [ k | onehot(a') | onehot(b') ].
"""
import numpy as np
import torch
import torch.nn.functional as F

from refiners_amd.latent_diffusion.sag import gaussian_blur
from tests import glue_cases as GC


def _torch_nearest(n_out: int, n_in: int) -> np.ndarray:
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    return F.interpolate(src, size=(n_out, 1), mode="nearest").view(n_out).long().numpy()


def test_float32_cell_formula_is_torch_nearest():
    bad = [(n_out, n_in) for n_out in range(1, 513) for n_in in range(1, n_out + 1) if not np.array_equal(GC.nearest_cells_f32(n_out, n_in), _torch_nearest(n_out, n_in))]
    assert not bad, bad[:10]


def test_integer_cell_formula_is_not():
    for n_out, n_in, row in ((122, 16, 61), (198, 50, 99)):
        assert (n_out, n_in) in GC.SAG_NEAREST
        integer = np.arange(n_out) * n_in // n_out
        differ = np.nonzero(integer != _torch_nearest(n_out, n_in))[0].tolist()
        assert differ == [row], (n_out, n_in, differ)
        assert np.array_equal(GC.nearest_cells_f32(n_out, n_in), _torch_nearest(n_out, n_in))


def test_sag_reference_matches_compute_degraded_latents():
    g = torch.Generator().manual_seed(3)
    n, C, h, w, ah, aw, ks, sigma = 2, 4, 12, 9, 3, 3, 9, 1.0
    x, noise = torch.randn(n, C, h, w, generator=g, dtype=torch.float64), torch.randn(n, C, h, w, generator=g, dtype=torch.float64)
    mass = torch.tensor([[0.5, 1.5, 1.0, 1.5, 0.5, 1.0, 1.5, 1.5, 0.5], [1.5, 0.5, 1.5, 1.0, 1.5, 0.5, 1.0, 0.5, 1.5]])
    a, sd = 0.83, 0.55
    # compute_sag_mask: threshold, one plane per channel, nearest interpolate to the latent size
    mask = (mass > 1.0).reshape(n, ah, aw).unsqueeze(1).repeat(1, C, 1, 1).type(torch.float64)
    mask = F.interpolate(mask, size=(h, w), mode="nearest")
    # compute_degraded_latents: remove_noise, gaussian_blur, blend, add_noise
    original = (x - sd * noise) / a
    degraded = gaussian_blur(original, kernel_size=ks, sigma=sigma)
    degraded = degraded * mask + original * (1 - mask)
    want = a * degraded + sd * noise
    got = GC.sag_reference(x, noise, mass, ah, aw, a, sd, GC.gaussian_w1(ks, sigma).double())
    assert (got - want).abs().max().item() < 1e-6  # (the separable weights are float32 values, gaussian_blur's float64: 1e-7 of an O(1) latent)
    assert mask.min() == 0 and mask.max() == 1  # both branches of the blend are exercised
    assert not torch.equal(mask[0], mask[1])  # the samples' masks differ


def test_relpos_gather_is_the_decomposed_bias():
    S1, S2, H, d, Lp, Dq = 3, 5, 2, 4, 20, 12
    L, M = S1 * S2, 2 * S1 * S2
    g = torch.Generator().manual_seed(5)
    q = torch.randn(M, H, d, generator=g, dtype=torch.float64)
    E1, E2 = torch.randn(2 * S1 - 1, d, generator=g, dtype=torch.float64), torch.randn(2 * S2 - 1, d, generator=g, dtype=torch.float64)
    src = torch.randn(M, H, Lp, generator=g, dtype=torch.float64)
    src[..., :d] = q
    src[..., d : d + 2 * S1 - 1] = q @ E1.flip(0).t()
    src[..., d + 2 * S1 - 1 : d + 2 * S1 + 2 * S2 - 2] = q @ E2.flip(0).t()
    out = GC.relpos_gather_ref(src.reshape(M, H * Lp), H, d, S1, S2, Lp, Dq).view(M, H, Dq)
    assert torch.equal(out[..., :d], q) and (out[..., d + S1 + S2 :] == 0).all()
    for row in range(M):
        a, b = (row % L) // S2, (row % L) % S2
        for a2 in range(S1):
            torch.testing.assert_close(out[row, :, d + a2], q[row] @ E1[a - a2 + S1 - 1], rtol=0, atol=1e-12)
        for b2 in range(S2):
            torch.testing.assert_close(out[row, :, d + S1 + b2], q[row] @ E2[b - b2 + S2 - 1], rtol=0, atol=1e-12)
