"""pytest -m gpu: mi355x_t2i_stem against float64 F.conv2d(F.pixel_unshuffle(x, r), w, b, padding=1) of the upcast inputs, mi355x_t2i_pool against
float64 F.avg_pool2d.  Bounds: the project's kernel bounds (docs/MEASUREMENTS_dinov2.md): max-abs error over max |reference| <= 1e-3 for float32
and <= 1.6e-2 for bfloat16 storage."""
import pytest
import torch
import torch.nn.functional as F

from refiners_amd import native

pytestmark = pytest.mark.gpu
BOUND = {torch.float32: 1e-3, torch.bfloat16: 1.6e-2}
#: (B, cin, r, h, w, C0): one pixel (every tap but the centre is padding); one row; a strip tail, two strips per row; two images, three strips;
#: one picture channel; SDXL's width (five column chunks); a column-chunk tail behind a whole chunk
STEM = [(1, 3, 8, 1, 1, 16), (1, 3, 16, 1, 3, 16), (1, 3, 16, 3, 33, 64), (2, 3, 8, 5, 70, 32), (1, 1, 8, 2, 5, 48), (1, 1, 16, 2, 2, 16),
        (1, 3, 8, 2, 3, 320), (1, 3, 8, 3, 33, 176)]
#: (picture dtype, output = compute dtype)
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)]
GUARD = 3


def _stem_case(shape, pic_dtype, dtype):
    B, cin, r, h, w, C0 = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((B, cin, r * h, r * w), generator=g).to(pic_dtype)
    wt = (torch.randn((C0, cin * r * r, 3, 3), generator=g) / (3 * r * cin ** 0.5)).to(dtype)
    b = torch.randn((C0,), generator=g).to(dtype)
    want = F.conv2d(F.pixel_unshuffle(x.double(), r), wt.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(B * h * w, C0)
    return x.cuda(), native.t2i_pack_stem(wt, r, dtype).cuda(), b.cuda(), want


def _run_stem(shape, pic_dtype, dtype):
    """The output is a view of a wider, longer buffer.  Returns (error, buffer, the buffer before the launch, the launch)."""
    B, cin, r, h, w, C0 = shape
    rows = B * h * w
    x, wp, b, want = _stem_case(shape, pic_dtype, dtype)
    buf = torch.full((rows + GUARD, C0 + 8), 7.0, dtype=dtype, device="cuda")
    buf0 = buf.clone()
    launch = lambda t: (native.t2i_stem(x, wp, b, t[:rows, :C0], r), torch.cuda.synchronize())  # noqa: E731
    launch(buf)
    err = float((buf[:rows, :C0].double().cpu() - want).abs().max() / want.abs().max())
    return err, buf, buf0, launch


@pytest.mark.parametrize("pic_dtype,dtype", DTYPES)
@pytest.mark.parametrize("shape", STEM)
def test_stem_against_float64(gpu_device, shape, pic_dtype, dtype):
    rows, C0 = shape[0] * shape[3] * shape[4], shape[5]
    err, buf, buf0, launch = _run_stem(shape, pic_dtype, dtype)
    print(f"{shape} {pic_dtype} -> {dtype}: {err:.2e}")
    assert err <= BOUND[dtype]
    assert torch.equal(buf[rows:], buf0[rows:]) and torch.equal(buf[:, C0:], buf0[:, C0:])  # guard rows, the columns behind the row
    again = buf0.clone()
    launch(again)
    assert torch.equal(again, buf)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("strip,chunk", [(32, 64), (32, 128), (64, 64), (64, 128)])
def test_every_strip_and_chunk(gpu_device, strip, chunk, dtype):
    shape = (1, 3, 8, 3, 70, 176)  # 70 pixels: a strip tail at 32 and at 64; 176 channels: a chunk tail at 64 and at 128
    native.load().mi355x_t2i_set_strip(strip, chunk)
    try:
        err, buf, buf0, _ = _run_stem(shape, dtype, dtype)
    finally:
        native.load().mi355x_t2i_set_strip(0, 0)
    assert err <= BOUND[dtype]
    assert torch.equal(buf[3 * 70:], buf0[3 * 70:]) and torch.equal(buf[:, 176:], buf0[:, 176:])


@pytest.mark.parametrize("r,C0", [(4, 16), (8, 24)])
def test_refused_stem_leaves_the_output_alone(gpu_device, r, C0):
    x = torch.randn(1, 3, 2 * r, 2 * r, device="cuda")
    wp = native.t2i_pack_stem(torch.randn(C0, 3 * r * r, 3, 3), r, torch.float32).cuda()
    buf = torch.full((4 + GUARD, C0 + 8), 7.0, device="cuda")
    with pytest.raises(native.NativeError, match="ESHAPE"):
        native.t2i_stem(x, wp, None, buf[:4, :C0], r)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 5, 4, 16), (2, 6, 7, 1280), (1, 3, 3, 16)])
def test_pool_against_float64(gpu_device, shape, dtype):
    B, H, W, C = shape
    rows, orows = B * H * W, B * (H // 2) * (W // 2)
    x = torch.randn((rows + GUARD, C + 8), generator=torch.Generator().manual_seed(H * W + C)).to(dtype).cuda()
    buf = torch.full((orows + GUARD, C + 16), 7.0, dtype=dtype, device="cuda")
    buf0 = buf.clone()
    native.t2i_pool(x[:rows, :C], B, H, W, buf[:orows, :C])
    torch.cuda.synchronize()
    want = F.avg_pool2d(x[:rows, :C].double().cpu().reshape(B, H, W, C).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).reshape(orows, C)
    err = float((buf[:orows, :C].double().cpu() - want).abs().max() / want.abs().max())
    assert err <= BOUND[dtype]
    assert torch.equal(buf[orows:], buf0[orows:]) and torch.equal(buf[:, C:], buf0[:, C:])
