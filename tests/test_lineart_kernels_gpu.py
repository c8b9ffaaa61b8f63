"""The entry points of csrc/lineart.hip against float64 torch on the GPU, float32 and bfloat16: the reflect-padded 7x7 stem, the InstanceNorm2d
statistics and apply over the three activation layouts (rows, the interior of a padded image, quadrants), the head, and the transposed
convolution end to end (phase weights through native.conv_gemm, statistics, apply with the un-shuffle).

Inputs are rounded to the tested dtype first and the reference is computed from the rounded values.  The bound is the one the kernels of this
project are held to (tests/kernel_cases._tol): max-abs error <= 1e-3 max|ref| for float32, 1.6e-2 max|ref| for bfloat16.  Outputs sit inside
NaN-filled buffers with guard rows and a wider leading dimension: whatever the kernel has no business writing must stay NaN.  The ring of a
padded INPUT is NaN as well: a reader of the interior that touched it would show."""
import pytest
import torch
import torch.nn.functional as F

from refiners_amd import native
from refiners_amd.engine import lineart as EL
from tests.kernel_cases import _tol

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
GUARD = 3  # rows in front of and behind every output
ROWS, PADDED, QUAD = native.LINEART_ROWS, native.LINEART_PADDED, native.LINEART_QUAD


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


def _activation(B, H, W, C_, dtype, seed, mean=0.0):
    """A logical [B, H, W, C_] activation rounded to dtype, with per-channel offsets and scales so that the statistics differ by channel."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    scale = 0.5 + torch.rand(C_, device=DEV, generator=g)
    shift = mean + torch.randn(C_, device=DEV, generator=g)
    return ((torch.randn(B, H, W, C_, device=DEV, generator=g) + shift) * scale).to(dtype)


def _in_layout(x, layout, pad=0, extra=8):
    """The buffer that holds the logical [B, H, W, C] activation x in `layout`: a [rows, columns] view of a wider buffer; a padded image's ring is NaN."""
    B, H, W, C_ = x.shape
    if layout == QUAD:
        body = x.view(B, H // 2, 2, W // 2, 2, C_).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // 2) * (W // 2), 4 * C_)
    elif layout == PADDED:
        img = torch.full((B, H + 2 * pad, W + 2 * pad, C_), NAN, device=DEV, dtype=x.dtype)
        img[:, pad : pad + H, pad : pad + W] = x
        body = img.view(-1, C_)
    else:
        body = x.reshape(B * H * W, C_)
    buf = torch.zeros(body.shape[0], body.shape[1] + extra, device=DEV, dtype=x.dtype)
    buf[:, : body.shape[1]] = body
    return buf[:, : body.shape[1]]


def _table(x, eps):
    """float64 (mean, rstd) [B, C, 2] of a logical [B, H, W, C] activation."""
    xd = x.double()
    mean, var = xd.mean(dim=(1, 2)), xd.var(dim=(1, 2), unbiased=False)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], dim=-1)


# ------------------------------------------------------------------------------------------------ stem
#: (B, Cin, H, W, bias): the smallest input; batch 2, odd sizes; four channels, larger than the 16 x 16 tile in both axes by a non-multiple
STEM = [(1, 3, 5, 5, False), (2, 3, 37, 50, True), (1, 4, 23, 41, False)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Cin,H,W,bias", STEM)
def test_stem(B, Cin, H, W, bias, dtype):
    g = torch.Generator(device=DEV).manual_seed(H * 100 + W)
    image = torch.rand(B, Cin, H, W + 3, device=DEV, generator=g).to(dtype)[..., :W]  # rows of a wider image
    w = torch.randn(64, Cin, 7, 7, device=DEV, generator=g) / (49 * Cin) ** 0.5
    b = 0.5 * torch.randn(64, device=DEV, generator=g) if bias else None
    buf, out = _guarded(B * H * W, 64, dtype)
    native.lineart_stem(image, native.lineart_pack_stem(w), b, out)
    torch.cuda.synchronize()
    ref = F.conv2d(F.pad(image.double(), (3, 3, 3, 3), mode="reflect"), w.double(), None if b is None else b.double())
    err = _err(out, ref.permute(0, 2, 3, 1).reshape(B * H * W, 64))
    print(f"stem {B}x{Cin}x{H}x{W} bias={bias} {dtype}: {err:.3e}")
    assert _only_view_written(buf, B * H * W, 64)
    assert err <= _tol(dtype), err


def test_stem_refuses_what_the_reflection_cannot_serve():
    image, w = torch.rand(1, 3, 3, 8, device=DEV), torch.zeros(3 * 49, 64, device=DEV)
    buf, out = _guarded(24, 64, torch.float32)
    with pytest.raises(native.NativeError, match="ESHAPE"):
        native.lineart_stem(image, w, None, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())  # a refused call launches nothing


# ------------------------------------------------------------------------------------------------ statistics
#: (B, H, W, C, layout, pad, mean): 6 pixels; batch 2 with H W no multiple of 32; the interior of a padded image, one of them a 2 x 3 one;
#: quadrants; 24 slabs of a mean of 50 standard deviations; four slabs with a ragged last one
STATS = [
    (1, 2, 3, 64, ROWS, 0, 0.0),
    (2, 10, 13, 128, ROWS, 0, 0.0),
    (2, 10, 13, 256, PADDED, 1, 0.0),
    (1, 2, 3, 256, PADDED, 1, 0.0),
    (1, 19, 25, 256, PADDED, 1, 0.0),
    (2, 10, 14, 64, QUAD, 0, 0.0),
    (1, 20, 26, 128, QUAD, 0, 0.0),
    (1, 64, 48, 64, ROWS, 0, 50.0),
    (1, 19, 25, 128, ROWS, 0, 50.0),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C_,layout,pad,mean", STATS)
def test_in_stats(B, H, W, C_, layout, pad, mean, dtype):
    eps = 1e-5
    x = _activation(B, H, W, C_, dtype, seed=H * W + C_, mean=mean)
    if mean:  # every channel about `mean` standard deviations off zero
        x = ((x.float() - x.float().mean(dim=(1, 2), keepdim=True)) / x.float().std(dim=(1, 2), keepdim=True) + mean).to(dtype)
    src = _in_layout(x, layout, pad)
    buf = torch.full((B + 2, C_, 2), NAN, device=DEV)
    tab = buf[1 : B + 1]
    native.lineart_in_stats(src, B, H, W, C_, eps, tab, layout=layout, pad=pad)
    torch.cuda.synchronize()
    ref = _table(x, eps)
    e_mean, e_rstd = _err(tab[..., 0], ref[..., 0]), _err(tab[..., 1], ref[..., 1])
    print(f"in_stats {B}x{H}x{W}x{C_} layout {layout} mean {mean} {dtype}: mean {e_mean:.3e} rstd {e_rstd:.3e}")
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()) and bool(torch.isfinite(tab).all())
    # the table is float32 whatever the storage type: the float32 bound holds for both
    assert e_mean <= _tol(torch.float32) and e_rstd <= _tol(torch.float32), (e_mean, e_rstd)
    again = torch.empty_like(tab)
    native.lineart_in_stats(src, B, H, W, C_, eps, again, layout=layout, pad=pad)
    assert torch.equal(again, tab)  # a fixed order of summation


# ------------------------------------------------------------------------------------------------ apply
#: source map -> (C, logical size for ROWS / PADDED; QUAD doubles it)
APPLY_SIZES = {(2, 3): 256, (10, 13): 128, (19, 25): 64}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ring", [0, 1, 3])
@pytest.mark.parametrize("layout", [ROWS, PADDED, QUAD])
@pytest.mark.parametrize("hw", list(APPLY_SIZES))
def test_in_apply(hw, layout, ring, dtype):
    C_ = APPLY_SIZES[hw]
    B = 2
    H, W = (2 * hw[0], 2 * hw[1]) if layout == QUAD else hw  # (a quadrant source of h x w rows is a logical 2h x 2w image)
    pad = 1 if layout == PADDED else 0
    x = _activation(B, H, W, C_, dtype, seed=H + 7 * W + ring)
    src = _in_layout(x, layout, pad)
    g = torch.Generator(device=DEV).manual_seed(ring + 3)
    tab = torch.stack([torch.randn(B, C_, device=DEV, generator=g), 0.5 + torch.rand(B, C_, device=DEV, generator=g)], dim=-1).contiguous()
    resid = _activation(B, H, W, C_, dtype, seed=H + 11 * W)
    res_pad = 1 if layout != ROWS else 0
    res_buf = _in_layout(resid, PADDED if res_pad else ROWS, res_pad)
    rows = B * (H + 2 * ring) * (W + 2 * ring)
    if ring >= min(H, W):  # ReflectionPad2d refuses it: so does the entry point, and nothing is launched
        buf, out = _guarded(rows, C_, dtype)
        with pytest.raises(native.NativeError, match="ESHAPE"):
            native.lineart_in_apply(src, B, H, W, C_, tab, out, layout=layout, pad=pad, relu=True, ring=ring)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all())
        return
    for relu, with_res in [(False, False), (True, False), (False, True), (True, True)]:
        buf, out = _guarded(rows, C_, dtype)
        native.lineart_in_apply(src, B, H, W, C_, tab, out, layout=layout, pad=pad, relu=relu, res=res_buf if with_res else None, res_pad=res_pad, ring=ring)
        torch.cuda.synchronize()
        ref = (x.double() - tab[..., 0].double()[:, None, None]) * tab[..., 1].double()[:, None, None]
        ref = F.relu(ref) if relu else ref
        ref = ref + resid.double() if with_res else ref
        ref = F.pad(ref.permute(0, 3, 1, 2), (ring,) * 4, mode="reflect").permute(0, 2, 3, 1) if ring else ref
        err = _err(out, ref.reshape(rows, C_))
        print(f"in_apply {B}x{H}x{W}x{C_} layout {layout} ring {ring} relu={relu} res={with_res} {dtype}: {err:.3e}")
        assert _only_view_written(buf, rows, C_)
        assert err <= _tol(dtype), err
        if ring:  # the ring is a COPY of interior pixels: bit for bit
            img = out.reshape(B, H + 2 * ring, W + 2 * ring, C_)
            iy, ix = EL.reflect_index(H, ring).to(DEV) + ring, EL.reflect_index(W, ring).to(DEV) + ring
            assert torch.equal(img, img[:, iy][:, :, ix])


# ------------------------------------------------------------------------------------------------ head
#: (B, H, W, layout, pad): the smallest; batch 2, odd, read from the interior of a padded image; quadrants, larger than the 16 x 8 tile in
#: both axes by a non-multiple
HEAD = [(1, 5, 5, ROWS, 0), (2, 37, 50, PADDED, 1), (1, 42, 22, QUAD, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,layout,pad", HEAD)
def test_head(B, H, W, layout, pad, dtype):
    eps = 1e-5
    x = _activation(B, H, W, 64, dtype, seed=H * 3 + W)
    src = _in_layout(x, layout, pad)
    g = torch.Generator(device=DEV).manual_seed(H)
    w = torch.randn(1, 64, 7, 7, device=DEV, generator=g) / 28.0
    bias = 0.3
    ref_tab = _table(x, eps)
    tab = ref_tab.float().contiguous()
    stride = H * W + 16
    buf = torch.full((GUARD + B * stride + GUARD,), NAN, device=DEV, dtype=dtype)
    out = buf.as_strided((B, 1, H, W), (stride, stride, W, 1), GUARD)
    native.lineart_head(src, B, H, W, tab, native.lineart_pack_head(w), bias, out, layout=layout, pad=pad)
    torch.cuda.synchronize()
    z = F.relu((x.double() - ref_tab[..., 0][:, None, None]) * ref_tab[..., 1][:, None, None]).permute(0, 3, 1, 2)
    ref = torch.sigmoid(F.conv2d(F.pad(z, (3, 3, 3, 3), mode="reflect"), w.double()) + bias)
    err = _err(out, ref)
    print(f"head {B}x{H}x{W} layout {layout} {dtype}: {err:.3e}")
    mask = torch.ones_like(buf, dtype=torch.bool)
    for b in range(B):
        mask[GUARD + b * stride : GUARD + b * stride + H * W] = False
    assert bool(torch.isnan(buf[mask]).all()) and bool(torch.isfinite(buf[~mask]).all())
    assert err <= _tol(dtype), err


# ------------------------------------------------------------------------------------------------ transposed convolution, end to end
@pytest.mark.parametrize("dtype", DTYPES)
def test_transposed_convolution_end_to_end(dtype):
    """ConvTranspose2d(256 -> 128, 3, stride 2, padding 1, output_padding 1) + InstanceNorm2d + ReLU at 10 x 13, the order the model applies
    them in: packed phase weights through native.conv_gemm, statistics over the quadrant layout, apply with the un-shuffle."""
    B, h, w, C_, Cp, eps = 1, 10, 13, 256, 128, 1e-5
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(B, h, w, C_, device=DEV, generator=g).to(dtype)
    wt = (torch.randn(C_, Cp, 3, 3, device=DEV, generator=g) / (4 * C_) ** 0.5).to(dtype)
    packed = native.pack_conv_weight(EL.pack_convt_phases(wt))
    quad = torch.empty(B * h * w, 4 * Cp, device=DEV, dtype=dtype)
    native.conv_gemm([(x, packed, 3, 1, 1)], quad, B, h, w)
    tab = torch.empty(B, Cp, 2, device=DEV)
    native.lineart_in_stats(quad, B, 2 * h, 2 * w, Cp, eps, tab, layout=QUAD)
    buf, out = _guarded(B * 4 * h * w, Cp, dtype)
    native.lineart_in_apply(quad, B, 2 * h, 2 * w, Cp, tab, out, layout=QUAD, relu=True)
    torch.cuda.synchronize()
    y = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), wt.double(), stride=2, padding=1, output_padding=1)
    ref = F.relu(F.instance_norm(y, eps=eps)).permute(0, 2, 3, 1).reshape(B * 4 * h * w, Cp)
    err = _err(out, ref)
    print(f"conv_transpose + instance norm + relu {dtype}: {err:.3e}")
    assert _only_view_written(buf, B * 4 * h * w, Cp)
    assert err <= _tol(dtype), err
