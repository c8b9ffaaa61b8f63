"""pytest -m gpu: the kernels of the tiled VAE (mi355x_groupnorm_table, mi355x_groupnorm_fixed, mi355x_vae_tile_gather, mi355x_vae_tile_blend)
against torch -- no autoencoder, milliseconds each.

Bounds.
  groupnorm_table   against torch.var_mean(correction=0) in float64 on the stored values.  The kernel sums pivoted float32 differences per thread
                    (chains of at most a few dozen terms) and everything across threads in double: the raw mean within 4 float32 ulps of the largest
                    |x|; the table's mean, which the existing finalize pass averages over the group's cg channels in float32, within cg + 2
                    half-ulps of it (cg - 1 additions, the division, the channel mean's own rounding); the variance and the table's rstd *
                    gamma within 1e-4 relative (a group of mean 100 and deviation 0.1 included: the pivot
                    removes the mean before anything is squared, so nothing cancels).
  groupnorm_fixed   against F.batch_norm(training=False) * weight + bias in float64 on the stored values.  The kernel computes
                    (x - mean) * a + beta with a = gamma / sqrt(var + eps) rounded to float32: each of the three terms carries a few float32
                    roundings, so |err| <= K eps32 (|x - mean| |a| + |beta| + |y|), K = 8; with SiLU K = 32 (the hardware exponential and
                    reciprocal add a few ulps of their own, and SiLU's slope is below 1.1).  bf16 adds the one rounding of the store, 2^-8 |y|.
  gather            a copy: the bits of the canvas, zeros in the pad channels.
  blend             single-rounding products, sums and a correctly rounded division in the reference's order: float32 must give the BITS of the
                    torch loop below; bf16 accumulates in float32 and rounds once, so it lies within one bf16 ulp of the float32 loop's result."""
import pytest
import torch
import torch.nn.functional as F

from refiners_amd import native
from refiners_amd.engine import tiled_vae as T
from refiners_amd.latent_diffusion.vae import _create_blending_mask, _ImageSize
from tests.tiled_vae_cases import GEOMETRY_C, TILE, TILED_VAE_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
EPS32 = 2.0**-23
GEOMETRIES = {"a": TILED_VAE_CASES["a"], "b": TILED_VAE_CASES["b"], "c": GEOMETRY_C}


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- GroupNorm with frozen statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C", [(1, 30, 128), (2, 64, 128), (1, 64, 512)])
def test_groupnorm_table_matches_var_mean(dtype, B, HW, C):
    G, eps = 32, 1e-6
    g = _gen(B * 1000 + HW + C)
    x = torch.randn(B, HW, C, generator=g)
    cg = C // G
    x[:, :, cg : 2 * cg] = 100.0 + 0.1 * torch.randn(B, HW, cg, generator=g)  # group 1: mean 100, deviation 0.1
    x[:, :, 5 * cg] += 100.0  # one channel of group 5 far from its group's other channels
    x = x.to(dtype)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dtype)
    tab = torch.full((B, C, 2), float("nan"), device=DEV)
    raw = torch.full((B, G, 2), float("nan"), device=DEV)
    native.groupnorm_table(x.to(DEV), gamma.to(DEV), G, eps, tab, raw)
    var, mean = torch.var_mean(x.double().reshape(B, HW, G, cg), dim=(1, 3), correction=0)
    raw, tab = raw.cpu().double(), tab.cpu().double()
    top = float(x.double().abs().max())
    print(f"table {dtype} B{B} HW{HW} C{C}: mean err {float((raw[..., 0] - mean).abs().max()):.2e} var rel {float(((raw[..., 1] - var) / var).abs().max()):.2e}")
    assert float((raw[..., 0] - mean).abs().max()) <= 4 * EPS32 * top
    assert float(((raw[..., 1] - var) / var).abs().max()) <= 1e-4
    assert float((tab[..., 0] - mean.repeat_interleave(cg, dim=1)).abs().max()) <= (cg + 2) * 0.5 * EPS32 * top
    a_ref = gamma.double() / torch.sqrt(var + eps).repeat_interleave(cg, dim=1)
    assert float(((tab[..., 1] - a_ref) / a_ref).abs().max()) <= 1e-4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("B,HW,C", [(1, 30, 128), (3, 64, 128), (3, 30, 512), (1, 64, 512)])
def test_groupnorm_fixed_matches_batch_norm(dtype, silu, B, HW, C):
    G, eps = 32, 1e-6
    g = _gen(B * 1000 + HW + C)
    cg = C // G
    x = (torch.randn(B, HW, C, generator=g) * 1.5 + 0.3).to(dtype)
    mean, var = torch.randn(G, generator=g) * 0.5, torch.rand(G, generator=g) * 2 + 0.05
    mean[1], var[1] = 100.0, 0.01
    x[:, :, cg : 2 * cg] = (100.0 + 0.1 * torch.randn(B, HW, cg, generator=g)).to(dtype)
    if B == 3:
        x[2] = x[0]  # the first and the last sample are the same data: under ONE table they must come out the same bits
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(dtype), (0.1 * torch.randn(C, generator=g)).to(dtype)
    a = gamma.float() / torch.sqrt(var + eps).repeat_interleave(cg)
    tab = torch.stack((mean.repeat_interleave(cg), a), dim=1).contiguous()
    out = torch.full((B, HW, C), float("nan"), device=DEV, dtype=dtype)
    native.groupnorm_fixed(x.to(DEV), tab.to(DEV), beta.to(DEV), silu, out)
    # FixedGroupNorm.compute_group_norm (auto_encoder.py:226-251) on the NCHW view of the same values, in float64
    xn = x.double().permute(0, 2, 1).reshape(B, C, HW, 1)
    grouped = xn.reshape(1, B * G, cg, HW, 1)
    y = F.batch_norm(grouped, mean.double().repeat(B), var.double().repeat(B), None, None, False, 0.0, eps).reshape(B, C, HW, 1)
    y = y * gamma.double().reshape(1, -1, 1, 1) + beta.double().reshape(1, -1, 1, 1)
    scale = (xn - mean.double().repeat_interleave(cg).reshape(1, -1, 1, 1)).abs() * a.double().abs().reshape(1, -1, 1, 1) + beta.double().abs().reshape(1, -1, 1, 1) + y.abs()
    if silu:
        y = F.silu(y)
    bound = (32 if silu else 8) * EPS32 * scale + (2.0**-8 * y.abs() if dtype == torch.bfloat16 else 0.0)
    got = out.cpu().double().permute(0, 2, 1).reshape(B, C, HW, 1)
    assert torch.isfinite(got).all()
    err = (got - y).abs()
    print(f"fixed {dtype} silu{int(silu)} B{B} HW{HW} C{C}: worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    if B == 3:
        assert torch.equal(out[0], out[2]) and not torch.equal(out[0], out[1])


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", [8, 6, 16])
def test_gather_nchw(dtype, w):
    """Odd lefts on an odd canvas width into the decoder's NCHW batch: w = 8 is the 16-byte path in float32 and the element path in bf16, 16 the vector
    path in both, 6 the element path."""
    C, H, W, h = 4, 21, 37, 5
    canvas = torch.randn(1, C, H, W, generator=_gen(w)).to(dtype)
    rows = [(0, 0), (3, 1), (H - h, W - w), (7, 11)]
    host = native.vae_pos_rows(rows)
    dst = torch.full((len(rows), C, h, w), 7.0, device=DEV, dtype=dtype)
    native.vae_tile_gather(canvas.to(DEV), host.to(DEV), host, dst, len(rows), (h, w), (C * h * w, h * w, w, 1))
    ref = torch.stack([canvas[0, :, t : t + h, l : l + w] for t, l in rows])
    assert torch.equal(dst.cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_token_major_padded(dtype):
    """The encoder's first activation: [T * h * w, cpad] rows, 3 image channels and zeros up to one K block."""
    C, H, W, h, w = 3, 19, 37, 6, 7
    cpad = 32 if dtype == torch.float32 else 64
    canvas = torch.randn(1, C, H, W, generator=_gen(5)).to(dtype)
    rows = [(0, 0), (13, 29), (5, 3)]
    host = native.vae_pos_rows(rows)
    dst = torch.full((len(rows) * h * w, cpad), 7.0, device=DEV, dtype=dtype)
    native.vae_tile_gather(canvas.to(DEV), host.to(DEV), host, dst, len(rows), (h, w), (h * w * cpad, 1, w * cpad, cpad), cpad=cpad)
    got = dst.cpu().view(len(rows), h, w, cpad)
    ref = torch.stack([canvas[0, :, t : t + h, l : l + w].permute(1, 2, 0) for t, l in rows])
    assert torch.equal(got[..., :C], ref) and bool((got[..., C:] == 0).all())


# ---- blend -------------------------------------------------------------------------------------------------------------------------------
def _grid(name, scale):
    c = GEOMETRIES[name]
    lat = T.latent_grid(c["latent_wh"], TILE, c["blending"])
    return lat if scale == 1 else lat.scaled(8, c["blending"])


def _reference_blend(grid, tiles, C):
    """_tiled_encode / _tiled_decode's accumulation (auto_encoder.py:480-526, 543-591) stated directly: tiles[i] is tile i's [C, h, w] result."""
    W, H = grid.size
    result = torch.zeros((1, C, H, W), device=DEV, dtype=torch.float32)
    weights = torch.zeros_like(result)
    for (top, left, bottom, right), tile in zip(grid.tiles, tiles):
        edge = (top == 0, bottom == H, left == 0, right == W)
        mask = _create_blending_mask(_ImageSize(bottom - top, right - left), grid.blending, C, device=DEV, dtype=torch.float32, is_edge=edge)
        result[:, :, top:bottom, left:right] += tile[None] * mask
        weights[:, :, top:bottom, left:right] += mask
    assert bool((weights > 0).all())
    return result / weights


def _run_blend(grid, tiles, C, dtype, layout):
    """The tiles laid out as the engine leaves them: "nchw" = [C, h, w] blocks back to back, "tokens" = [h * w, ld] rows with ld = C + 1."""
    placement, parts, off = {}, [], 0
    for i, tile in enumerate(tiles):
        _, h, w = tile.shape
        if layout == "nchw":
            parts.append(tile.reshape(-1))
            placement[i] = (off, h * w, w, 1)
        else:
            ld = C + 1
            rows = torch.full((h * w, ld), 3.0, device=DEV, dtype=tile.dtype)
            rows[:, :C] = tile.permute(1, 2, 0).reshape(h * w, C)
            parts.append(rows.reshape(-1))
            placement[i] = (off, 1, w * ld, ld)
        off += parts[-1].numel()
    arena = torch.cat(parts).to(dtype)
    ramps, offs = T.ramp_tables(grid)
    axis_host = native.vae_axis_rows(grid.xs, grid.ys)
    tiles_host = native.vae_blend_rows(T.blend_rows(grid, placement, offs))
    canvas = torch.full((1, C, grid.size[1], grid.size[0]), 7.0, device=DEV, dtype=dtype)
    args = (arena, ramps.to(DEV), axis_host.to(DEV), axis_host, tiles_host.to(DEV), tiles_host, (len(grid.xs), len(grid.ys)), grid.stride, grid.tile)
    native.vae_tile_blend(canvas, *args)
    return canvas, args


@pytest.mark.parametrize("name,scale,layout", [("a", 1, "nchw"), ("a", 8, "tokens"), ("b", 1, "nchw"), ("b", 8, "tokens"), ("c", 1, "nchw"), ("c", 1, "tokens"), ("c", 8, "tokens"),
                                               ("b", 8, "nchw")])
def test_blend_matches_reference_loop(name, scale, layout):
    grid = _grid(name, scale)
    C = 4 if scale == 1 else 3
    g = torch.Generator(device=DEV).manual_seed(len(grid.tiles) + scale)
    tiles = [torch.randn((C, b - t, r - l), generator=g, device=DEV) for t, l, b, r in grid.tiles]
    assert name != "c" or len(tiles) > 64
    ref = _reference_blend(grid, tiles, C)
    got, args = _run_blend(grid, tiles, C, torch.float32, layout)
    assert torch.equal(got, ref), float((got - ref).abs().max())
    again = torch.full_like(got, -1.0)
    native.vae_tile_blend(again, *args)
    assert torch.equal(again, got)  # two replays are bit-equal
    # bf16: the same rounded inputs through the float32 loop, one rounding at the store
    tiles16 = [t.to(torch.bfloat16) for t in tiles]
    ref16 = _reference_blend(grid, [t.float() for t in tiles16], C)
    got16, _ = _run_blend(grid, tiles16, C, torch.bfloat16, layout)
    ulp = torch.ldexp(torch.ones_like(ref16), torch.frexp(ref16).exponent - 8)  # |ref| = m 2^e with m in [0.5, 1): 8 significant bits
    assert bool(((got16.float() - ref16).abs() <= ulp).all()), float(((got16.float() - ref16).abs() / ulp).max())


# ---- validation --------------------------------------------------------------------------------------------------------------------------
def test_validation_errors_leave_the_destination_untouched():
    grid = _grid("b", 1)
    C = 4
    tiles = [torch.ones((C, b - t, r - l), device=DEV) for t, l, b, r in grid.tiles]
    _, good = _run_blend(grid, tiles, C, torch.float32, "nchw")
    arena, ramps, axis, axis_host, trows, trows_host, nxy, stride, tile = good
    canvas = torch.full((1, C, grid.size[1], grid.size[0]), 7.0, device=DEV)

    def refused(code, *args, **kw):
        with pytest.raises(native.NativeError, match=code):
            native.vae_tile_blend(canvas, *args, **kw)
        torch.cuda.synchronize()
        assert bool((canvas == 7.0).all())

    bad_axis = native.vae_axis_rows([(s + 1, e) for s, e in grid.xs], grid.ys)  # starts that are not index * stride
    refused("ESHAPE", arena, ramps, axis, bad_axis, trows, trows_host, nxy, stride, tile)
    outside = native.vae_axis_rows(grid.xs[:-1] + [(grid.xs[-1][0], grid.xs[-1][1] + 1)], grid.ys)  # the last column ends past the canvas
    refused("ESHAPE", arena, ramps, axis, outside, trows, trows_host, nxy, stride, tile)
    _, offs = T.ramp_tables(grid)
    place = {i: (0, 1, 1, 1) for i in range(len(tiles))}
    long_ramp = native.vae_blend_rows([(0, 1, 1, 1, 0, 5)] * len(tiles))  # 2 * 5 > the 8 of a tile
    refused("ESHAPE", arena, ramps, axis, axis_host, trows, long_ramp, nxy, stride, tile)
    far = native.vae_blend_rows([(arena.numel(), *r[1:]) for r in T.blend_rows(grid, place, offs)])  # a tile that starts where the source ends
    refused("EARG", arena, ramps, axis, axis_host, trows, far, nxy, stride, tile)
    refused("ESHAPE", arena, ramps, axis, axis_host, trows, trows_host, nxy, (0, stride[1]), tile)
    with pytest.raises(native.NativeError, match="EARG"):  # the source overlaps the canvas
        native.vae_tile_blend(canvas, canvas.view(-1), ramps, axis, axis_host, trows, trows_host, nxy, stride, tile)
    assert bool((canvas == 7.0).all())

    src = torch.randn(1, 3, 16, 20, device=DEV)
    dst = torch.full((2, 3, 4, 8), 7.0, device=DEV)
    for rows, strides, code in (([(0, 0), (13, 0)], (96, 32, 8, 1), "ESHAPE"),      # a tile below the canvas
                                ([(0, 0), (0, 13)], (96, 32, 8, 1), "ESHAPE"),      # ... right of it
                                ([(0, 0), (1, 1)], (97, 32, 8, 1), "ESHAPE")):      # the last tile ends past dst
        host = native.vae_pos_rows(rows)
        with pytest.raises(native.NativeError, match=code):
            native.vae_tile_gather(src, host.to(DEV), host, dst, 2, (4, 8), strides)
        assert bool((dst == 7.0).all())
    host = native.vae_pos_rows([(0, 0)])
    before = src.clone()
    with pytest.raises(native.NativeError, match="EARG"):  # the destination lies inside the canvas
        native.vae_tile_gather(src, host.to(DEV), host, src.view(-1)[8:], 1, (4, 8), (96, 32, 8, 1))
    assert torch.equal(src, before)

    x = torch.randn(1, 30, 128, device=DEV)
    out = torch.full_like(x, 7.0)
    tab, beta = torch.zeros(128, 2, device=DEV), torch.zeros(128, device=DEV)
    with pytest.raises(native.NativeError, match="ESHAPE"):  # channels that are no multiple of 16 bytes
        native.groupnorm_fixed(x[:, :, :126], tab[:126].contiguous(), beta[:126], False, out[:, :, :126])
    with pytest.raises(native.NativeError, match="ESHAPE"):  # more channels per group than the finalize pass holds
        native.groupnorm_table(torch.randn(1, 8, 1024, device=DEV), torch.ones(1024, device=DEV), 2, 1e-6, torch.zeros(1, 1024, 2, device=DEV))
    assert bool((out == 7.0).all())
