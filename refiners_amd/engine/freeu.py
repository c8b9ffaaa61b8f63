"""Host tables of FreeU's Fourier filter (reference latent_diffusion/freeu.py, fourier_filter) for mi355x_freeu_filter.

fourier_filter(x, scale, threshold=t) multiplies the slice `center - t : center + t` of the shifted spectrum, i.e. the frequencies
F = {-t .. t-1} of each axis (odd sizes included: the shifted index n // 2 is frequency 0), by `scale` and keeps the real part.  Per plane

    out = x + (scale - 1) P x,      P = Re( sum over (u, v) in F x F of  e_uv e_uv^H ) / (H W),    e_uv[i, j] = exp(2 pi i (u i / H + v j / W))

and Re(e e^H) = Re(e) Re(e)^T + Im(e) Im(e)^T: every frequency pair contributes its cosine and its sine plane.  A pair whose conjugate
(-u, -v) lies in the box as well shares both planes with it (weight 2, listed once); a self-conjugate pair (u = 0 or 2 u = H, and the same
for v) has no sine plane.  At threshold 1 that leaves 1 + 3 * 2 = 7 planes for every H, W >= 3 and fewer on 2-wide planes -- the rank of P.

The kernel takes the factors as two float32 tables of 16 rows, columns padded with zeros to a multiple of 128:
    analysis  A[r][p] = plane r at pixel p = i * W + j                      (entries in [-1, 1])
    synthesis S[r][p] = (scale - 1) * weight_r / (H W) * plane r at pixel p
built in float64 and rounded once."""
from __future__ import annotations

import math
from typing import Callable

import torch
from torch import Tensor

from .packing import PackCache, Unsupported

ROWS = 16  # table rows of mi355x_freeu_filter
COLS = 128  # its column granularity


def planes(H: int, W: int, threshold: int = 1) -> tuple[Tensor, Tensor]:
    """(planes [R, H*W] float64, weights [R] float64) with P = planes^T diag(weights) planes."""
    if H < 2 or W < 2:
        raise Unsupported(f"the Fourier filter of a {H} x {W} plane is not lowered")
    if threshold < 1 or 2 * threshold > min(H, W):
        raise Unsupported(f"threshold {threshold} does not select a box of a {H} x {W} spectrum")
    box = {(u % H, v % W) for u in range(-threshold, threshold) for v in range(-threshold, threshold)}
    i = torch.arange(H, dtype=torch.float64).repeat_interleave(W)
    j = torch.arange(W, dtype=torch.float64).repeat(H)
    rows, weights = [], []
    for u, v in sorted(box):
        conj = ((-u) % H, (-v) % W)
        if conj in box and conj < (u, v):
            continue  # listed with its conjugate
        phase = 2 * math.pi * (u * i / H + v * j / W)
        if conj == (u, v):
            rows.append(torch.cos(phase))  # (+-1: a self-conjugate pair has no sine plane)
            weights.append(1.0)
        else:
            w = 2.0 if conj in box else 1.0
            rows += [torch.cos(phase), torch.sin(phase)]
            weights += [w, w]
    return torch.stack(rows), torch.tensor(weights, dtype=torch.float64) / (H * W)


def probe_skip_scale(func: Callable[[Tensor], Tensor]) -> float:
    """The skip scale of a FreeUSkipFeatures' Lambda, which keeps it in a closure: on a 2 x 2 plane the box covers the whole spectrum, so the
    filter of ones returns the scale.  The function is then held to the threshold-1 filter at that scale on a 5 x 6 plane; anything else is not
    the lowered pattern."""
    with torch.no_grad():
        scale = float(func(torch.ones(1, 1, 2, 2, dtype=torch.float64))[0, 0, 0, 0])
        x = torch.sin(torch.arange(30, dtype=torch.float64) * 1.7).reshape(1, 1, 5, 6)
        pl, wt = planes(5, 6)
        want = x.reshape(30) + (scale - 1.0) * (pl.T * wt) @ (pl @ x.reshape(30))
        got = func(x)
    if tuple(got.shape) != (1, 1, 5, 6) or not torch.allclose(got.reshape(30).double(), want, rtol=0.0, atol=1e-6):
        raise Unsupported("FreeUSkipFeatures' Lambda is not the threshold-1 Fourier filter")
    return scale


def tables(H: int, W: int, scale: float, threshold: int = 1, cache: PackCache | None = None, device: torch.device | str = "cpu") -> tuple[Tensor, Tensor, int]:
    """(analysis, synthesis, rank): float32 [16, HWpad] on `device`, cached per (H, W, scale, threshold); Unsupported when the rank exceeds 16 rows."""

    def make() -> tuple[Tensor, Tensor, int]:
        pl, wt = planes(H, W, threshold)
        R = pl.shape[0]
        if R > ROWS:
            raise Unsupported(f"the Fourier filter at threshold {threshold} on a {H} x {W} plane has rank {R}, the kernel's tables hold {ROWS} rows")
        pad = (H * W + COLS - 1) // COLS * COLS
        A = torch.zeros(ROWS, pad, dtype=torch.float64)
        S = torch.zeros(ROWS, pad, dtype=torch.float64)
        A[:R, : H * W] = pl
        S[:R, : H * W] = pl * (wt * (float(scale) - 1.0)).unsqueeze(1)
        return A.to(device=device, dtype=torch.float32), S.to(device=device, dtype=torch.float32), R

    if cache is None:
        return make()
    return cache.get(("freeu_tables", H, W, float(scale), threshold, str(device)), make)
