"""The three streaming kernels of csrc/dinov2.hip against float64 torch on the GPU, float32 and bfloat16: the position resampling (its host tap
tables applied to the channels-last table), the token assembly and GLU(SiLU()).

Inputs are rounded to the tested dtype first and the reference is computed from the rounded values.  The bound is the one the kernels of this
project are held to (tests/kernel_cases._tol): max-abs error <= 1e-3 max|ref| for float32, 1.6e-2 max|ref| for bfloat16.  Outputs sit inside
NaN-filled buffers with guard rows and a wider leading dimension: whatever the kernel has no business writing must stay NaN."""
import pytest
import torch
import torch.nn.functional as F

from refiners_amd import native
from refiners_amd.engine import dinov2 as ED
from tests.kernel_cases import _tol

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
GUARD = 3  # rows in front of and behind every output


def _guarded(rows, cols, dtype, pad=16):
    """(buffer [GUARD + rows + GUARD, cols + pad] of NaN, the [rows, cols] view inside it)."""
    buf = torch.full((rows + 2 * GUARD, cols + pad), NAN, device=DEV, dtype=dtype)
    return buf, buf[GUARD : GUARD + rows, :cols]


def _only_view_written(buf, rows, cols):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[GUARD : GUARD + rows, :cols] = False
    return bool(torch.isnan(buf[mask]).all()) and bool(torch.isfinite(buf[~mask]).all())


def _err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ pos_resample
#: (source side, rows, columns, D, mode, antialias)
RESAMPLE = [
    (5, 3, 7, 64, "bicubic", True),
    (5, 1, 9, 200, "bicubic", True),    # one output row: the antialiased taps span the whole axis
    (37, 16, 16, 384, "bicubic", True),
    (37, 16, 16, 384, "bicubic", False),
    (5, 8, 4, 64, "bilinear", False),
]


def _table(m, D, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    full = (0.5 * torch.randn(1 + m * m, D, device=DEV, generator=g)).to(dtype)  # row 0: the class position, as in the model's table
    return full


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,h,w,D,mode,aa", RESAMPLE)
def test_pos_resample(m, h, w, D, mode, aa, dtype):
    full = _table(m, D, dtype, seed=m * 100 + h)
    src = full[1:]
    ty, tx = ED.axis_table(m, h, mode, aa, DEV), ED.axis_table(m, w, mode, aa, DEV)
    buf, out = _guarded(h * w, D, torch.float32)
    native.dinov2_pos_resample(src, ty, tx, out)
    torch.cuda.synchronize()
    grid = src.double().view(m, m, D).permute(2, 0, 1).unsqueeze(0)
    ref = F.interpolate(grid, size=(h, w), mode=mode, antialias=aa).squeeze(0).permute(1, 2, 0).reshape(h * w, D)
    err = _err(out, ref)
    print(f"pos_resample {mode} aa={aa} {m}x{m} -> {h}x{w} D={D} {dtype}: {err:.3e}")
    assert _only_view_written(buf, h * w, D)
    assert err <= _tol(dtype), err
    if aa and h == 1:
        assert int(ty.host[1][0]) == m  # the whole axis in one output cell


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,aa", [("bicubic", False), ("bicubic", True), ("bilinear", False)])
def test_pos_resample_at_the_native_grid_is_the_identity(mode, aa, dtype):
    m, D = 5, 64
    src = _table(m, D, dtype, seed=3)[1:]
    ty, tx = ED.axis_table(m, m, mode, aa, DEV), ED.axis_table(m, m, mode, aa, DEV)
    buf, out = _guarded(m * m, D, torch.float32)
    native.dinov2_pos_resample(src, ty, tx, out)
    torch.cuda.synchronize()
    assert torch.equal(out, src.float()) and _only_view_written(buf, m * m, D)


# ------------------------------------------------------------------------------------------------ tokens
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,R,n,D,rows", [(1, 0, 25, 64, 26), (3, 4, 21, 200, 26), (2, 4, 21, 64, 64)])
def test_tokens(B, R, n, D, rows, dtype):
    g = torch.Generator(device=DEV).manual_seed(B * 10 + R)
    patch = torch.randn(B * n, D + 8, device=DEV, generator=g).to(dtype)[:, :D]  # a wider leading dimension
    pos = 0.5 * torch.randn(n, D, device=DEV, generator=g)
    cls, pos0 = (0.5 * torch.randn(D, device=DEV, generator=g)).to(dtype), (0.5 * torch.randn(D, device=DEV, generator=g)).to(dtype)
    reg = (0.5 * torch.randn(R, D, device=DEV, generator=g)).to(dtype) if R else None
    buf, out = _guarded(B * rows, D, dtype)
    native.dinov2_tokens(patch, pos, cls, pos0, reg, out, B, rows=rows)
    torch.cuda.synchronize()
    T = 1 + R + n
    ref = torch.zeros(B, rows, D, device=DEV, dtype=torch.float64)
    ref[:, 0] = cls.double() + pos0.double()
    if R:
        ref[:, 1 : 1 + R] = reg.double()
    ref[:, 1 + R : T] = patch.double().reshape(B, n, D) + pos.double()
    err = _err(out, ref.view(B * rows, D))
    print(f"tokens B={B} R={R} n={n} D={D} rows={rows} {dtype}: {err:.3e}")
    assert _only_view_written(buf, B * rows, D)  # the guard rows and the padding columns are untouched
    assert err <= _tol(dtype), err
    got = out.view(B, rows, D)
    assert bool((got[:, T:] == 0).all())  # padding rows are exact zeros
    if R:
        assert torch.equal(got[:, 1 : 1 + R], reg.expand(B, R, D))  # registers get no position: copied bit for bit
    if dtype == torch.float32:  # every sum is one float32 addition
        assert torch.equal(got[:, 1 + R : T], patch.reshape(B, n, D) + pos) and torch.equal(got[:, 0], (cls + pos0).expand(B, D))


# ------------------------------------------------------------------------------------------------ glu_silu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Fd", [(25, 256), (3, 4096)])
def test_glu_silu(M, Fd, dtype):
    g = torch.Generator(device=DEV).manual_seed(M)
    x = (2.0 * torch.randn(M, 2 * Fd, device=DEV, generator=g)).to(dtype)
    x[0, Fd : Fd + 4] = torch.tensor([100.0, -100.0, 88.5, -88.5], device=DEV).to(dtype)  # gates where exp over- and underflows
    x[0, :4] = 1.5
    buf, out = _guarded(M, Fd, dtype)
    native.glu_silu(x, out)
    torch.cuda.synchronize()
    xd = x.double()
    ref = xd[:, :Fd] * F.silu(xd[:, Fd:])
    err = _err(out[1:], ref[1:])  # (row 0 holds the +-100 gates, checked on their own below: its 150 would hide everything else)
    print(f"glu_silu M={M} F={Fd} {dtype}: {err:.3e}")
    assert _only_view_written(buf, M, Fd)
    assert err <= _tol(dtype), err
    edge, want = out[0, :4].double(), ref[0, :4]
    assert torch.isfinite(edge).all() and float((edge - want).abs().max()) <= _tol(dtype) * 150.0, (edge, want)  # 150 = |1.5 * silu(100)|
