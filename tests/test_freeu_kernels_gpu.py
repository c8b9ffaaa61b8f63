"""pytest -m gpu: mi355x_freeu_filter against the float64 torch.fft filter of the upcast input.  Bounds: the project's kernel bounds
(docs/MEASUREMENTS_dinov2.md): max-abs error over max |reference| <= 1e-3 for float32 and <= 1.6e-2 for bfloat16 storage."""
import pytest
import torch

from refiners_amd import native
from refiners_amd.engine import freeu as T
from refiners_amd.latent_diffusion.freeu import fourier_filter

pytestmark = pytest.mark.gpu
BOUND = {torch.float32: 1e-3, torch.bfloat16: 1.6e-2}
#: (B, H, W, C_skip, C_b): one slab; odd plane, tail slab, half = 24; SDXL's plane, several slabs, several rounds per wave; 988 pixels (K tail); rank below 7
SHAPES = [(1, 4, 4, 64, 64), (2, 5, 7, 80, 48), (2, 32, 32, 128, 128), (1, 38, 26, 64, 32), (1, 2, 3, 32, 16)]
GUARD, SKIP_SCALE, BACKBONE_SCALE = 3, 0.2, 1.3


def _buffers(dtype, B, H, W, cs, cb):
    """skip, skip_out and backbone as views of wider, longer buffers: a row stride above the width and guard rows behind."""
    g = torch.Generator().manual_seed(B * 1000 + H * W + cs)
    rows = B * H * W
    skip = torch.randn((rows + GUARD, cs + 8), generator=g).to(dtype).cuda()
    out = torch.full((rows + GUARD, cs + 16), 7.0, dtype=dtype, device="cuda")
    bb = torch.randn((rows + GUARD, cb + 8), generator=g).to(dtype).cuda()
    return skip, out, bb


def _launch(skip, out, bb, B, H, W, cs, cb):
    rows = B * H * W
    A, S, R = T.tables(H, W, SKIP_SCALE, device="cuda")
    native.freeu_filter(skip[:rows, :cs], out[:rows, :cs], bb[:rows, :cb], B, A, S, R, BACKBONE_SCALE)
    torch.cuda.synchronize()


def _errors(skip, out, bb0, bb, B, H, W, cs, cb):
    rows = B * H * W
    x = skip[:rows, :cs].double().cpu().reshape(B, H, W, cs).permute(0, 3, 1, 2)
    want = fourier_filter(x, SKIP_SCALE).permute(0, 2, 3, 1).reshape(rows, cs)
    e_skip = float((out[:rows, :cs].double().cpu() - want).abs().max() / want.abs().max())
    want_b = bb0[:rows, : cb // 2].double().cpu() * BACKBONE_SCALE
    return e_skip, float((bb[:rows, : cb // 2].double().cpu() - want_b).abs().max() / want_b.abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_filter_against_float64_fft(gpu_device, shape, dtype):
    B, H, W, cs, cb = shape
    rows = B * H * W
    skip, out, bb = _buffers(dtype, *shape)
    skip0, out0, bb0 = skip.clone(), out.clone(), bb.clone()
    _launch(skip, out, bb, *shape)
    e_skip, e_bb = _errors(skip, out, bb0, bb, *shape)
    print(f"{shape} {dtype}: skip {e_skip:.2e} backbone {e_bb:.2e}")
    assert e_skip <= BOUND[dtype] and e_bb <= BOUND[dtype]
    assert torch.equal(skip, skip0)
    assert torch.equal(out[rows:], out0[rows:]) and torch.equal(out[:, cs:], out0[:, cs:])  # guard rows, the columns behind the row
    assert torch.equal(bb[rows:], bb0[rows:]) and torch.equal(bb[:, cb // 2:], bb0[:, cb // 2:])  # ... and the backbone's other half, bit for bit
    out2, bb2 = out0.clone(), bb0.clone()
    _launch(skip, out2, bb2, *shape)
    assert torch.equal(out2, out) and torch.equal(bb2, bb)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("slab", [16, 32, 64])
def test_every_slab_width(gpu_device, slab, dtype):
    shape = (2, 5, 7, 80, 48)  # 80 channels: a tail slab at 32 and at 64
    skip, out, bb = _buffers(dtype, *shape)
    bb0 = bb.clone()
    native.load().mi355x_freeu_set_slab(slab)
    try:
        _launch(skip, out, bb, *shape)
    finally:
        native.load().mi355x_freeu_set_slab(0)
    e_skip, e_bb = _errors(skip, out, bb0, bb, *shape)
    assert e_skip <= BOUND[dtype] and e_bb <= BOUND[dtype]


@pytest.mark.parametrize("cs,cb", [(12, 48), (80, 40)])
def test_refused_shapes_leave_the_outputs_alone(gpu_device, cs, cb):
    shape = (1, 4, 4, cs, cb)
    skip, out, bb = _buffers(torch.float32, *shape)
    out0, bb0 = out.clone(), bb.clone()
    with pytest.raises(native.NativeError, match="ESHAPE"):
        _launch(skip, out, bb, *shape)
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(bb, bb0)
