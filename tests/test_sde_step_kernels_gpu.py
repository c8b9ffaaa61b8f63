"""pytest -m gpu: the stochastic solver updates (csrc/solver_step.hip: mi355x_cfg_sde_step, mi355x_sde_step).

* The guidance-free form is bit-equal to the guided one on cat(out, out) at any guidance scale: u + s (c - u) with c == u is u, and the rest
  is ONE device function (csrc/solver_update.cuh: sde_update) called from both instantiations.
* With kn = 0 the results compare equal to mi355x_linear_step / mi355x_cfg_linear_step on the same operands (x, hist, model input): the update is
  their device function followed by one fused multiply-add, and fma(0, noise, v) == v.
* Against a float64 torch model of the five-term update, with the coefficients as the kernel reads them (float32): the bounds of
  tests/test_solver_step_kernels_gpu.py, by the same argument -- float32 within 1e-6 (relative l2 and relative maximum: a handful of float32
  roundings, 6e-8 each, on terms the size of the result; a plain float32 evaluation of the five terms reads 1.6e-7 at most on these shapes);
  bfloat16 within ONE bfloat16 rounding of the float64 result, |got - ref| <= 2^-8 |ref|, plus the float32 bound for a value on a rounding tie.
Shapes: that file's -- 1x4x16x16, 1x4x12x20, 3x4x6x10, 1x4x5x7 (140 elements: in bfloat16 a 4-element tail behind 17 vectors; guided, the second
half starts off a 16-byte boundary) and 1x3x3x7 (63: a tail in both types) -- and views that start one element off a 16-byte boundary."""
import pytest
import torch

from refiners_amd import native
from refiners_amd.latent_diffusion.solvers import DPMSolver

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 4, 16, 16), (1, 4, 12, 20), (3, 4, 6, 10), (1, 4, 5, 7), (1, 3, 3, 7)]
DTYPES = [torch.float32, torch.bfloat16]
SDE_ROWS = {
    "first_order": lambda: DPMSolver(4, sde_variance=1.0).linear_step(0),
    "second_order": lambda: DPMSolver(4, sde_variance=1.0).linear_step(2),
    "last_step": lambda: DPMSolver(4, sde_variance=1.0).linear_step(3),
}


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


def _data(shape, dtype, seed, parts=4):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(shape, device=DEV, generator=g).to(dtype) for _ in range(parts)]


def _close(got, ref, dtype, what):
    g, r = got.double(), ref
    scale = float(r.abs().max())
    if dtype == torch.float32:
        l2, mx = float((g - r).norm() / r.norm()), float((g - r).abs().max() / scale)
        print(f"{what} float32: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < 1e-6 and mx < 1e-6, (what, l2, mx)
    else:
        over = ((g - r).abs() - (2.0**-8 * r.abs() + 1e-6 * scale)).max()
        print(f"{what} bfloat16: worst excess over one rounding {float(over):.2e}")
        assert float(over) <= 0.0, (what, float(over))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("row", list(SDE_ROWS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sde_step(shape, row, dtype):
    x0, out, h0, nz = _data(shape, dtype, 21)
    n = x0.numel()
    coefs = SDE_ROWS[row]()
    assert len(coefs) == 8 and coefs[7] > 0.0
    got = None
    for cfg in (1.0, 7.5):
        coef = torch.tensor([cfg, *coefs], dtype=torch.float32, device=DEV)
        xg, hg, mg, zg = x0.clone(), h0.clone(), torch.zeros((2 * shape[0],) + shape[1:], device=DEV, dtype=dtype), nz.clone()
        native.cfg_sde_step(xg, torch.cat((out, out)).contiguous(), hg, zg, mg, coef)
        xf, hf, mf, zf = x0.clone(), h0.clone(), torch.zeros_like(x0), nz.clone()
        native.sde_step(xf, out, hf, zf, mf, coef)
        assert torch.equal(xf, xg) and torch.equal(hf, hg), f"{row}, guidance scale {cfg}: not bit-equal to mi355x_cfg_sde_step"
        assert torch.equal(mf, mg[: shape[0]]) and torch.equal(mf, mg[shape[0] :]), f"{row}: model input differs from the guided kernel's"
        assert torch.equal(zg, nz) and torch.equal(zf, nz), "the draw is read only"
        xn, hn = x0.clone(), h0.clone()
        native.sde_step(xn, out, hn, nz, None, coef)  # no model-input buffer
        assert torch.equal(xn, xf) and torch.equal(hn, hf)
        xn, hn = x0.clone(), h0.clone()
        native.cfg_sde_step(xn, torch.cat((out, out)).contiguous(), hn, nz, None, coef)
        assert torch.equal(xn, xf) and torch.equal(hn, hf)
        got = (xf, hf, mf)
    c = torch.tensor([0.0, *coefs], dtype=torch.float32).double()
    x, e, h, z = x0.double(), out.double(), h0.double(), nz.double()
    d = c[1] * x + c[2] * e
    ref = c[3] * x + c[4] * e + c[5] * d + c[6] * h + c[8] * z
    _close(got[0], ref, dtype, f"{row} x' {n}")
    _close(got[1], d, dtype, f"{row} hist {n}")
    _close(got[2], c[7] * got[0].double(), dtype, f"{row} model input {n}")  # the STORED x' is what the next step scales


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_guided_pair_against_a_float64_model(shape, dtype):
    """Two DIFFERENT halves: eps = u + cfg (c - u) in front of the update."""
    x0, u, c_, h0, nz = _data(shape, dtype, 22, parts=5)
    coefs = SDE_ROWS["second_order"]()
    coef = torch.tensor([7.5, *coefs], dtype=torch.float32, device=DEV)
    x, h, m = x0.clone(), h0.clone(), torch.zeros((2 * shape[0],) + shape[1:], device=DEV, dtype=dtype)
    native.cfg_sde_step(x, torch.cat((u, c_)).contiguous(), h, nz, m, coef)
    c = coef.double()
    eps = u.double() + c[0] * (c_.double() - u.double())
    d = c[1] * x0.double() + c[2] * eps
    ref = c[3] * x0.double() + c[4] * eps + c[5] * d + c[6] * h0.double() + c[8] * nz.double()
    _close(x, ref, dtype, f"guided pair x' {x0.numel()}")
    _close(h, d, dtype, f"guided pair hist {x0.numel()}")
    assert torch.equal(m[: shape[0]], m[shape[0] :])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("row", ["dpm_first_order", "dpm_second_order"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_without_a_noise_coefficient_it_is_the_existing_kernel(shape, row, dtype):
    x0, u, c_, h0, nz = _data(shape, dtype, 23, parts=5)
    coefs = DPMSolver(4).linear_step(0 if row == "dpm_first_order" else 2)  # the deterministic row, kn = 0 behind it
    coef = torch.tensor([7.5, *coefs, 0.0], dtype=torch.float32, device=DEV)
    pair = torch.cat((u, c_)).contiguous()
    xa, ha, ma = x0.clone(), h0.clone(), torch.zeros_like(pair)
    native.cfg_linear_step(xa, pair, ha, ma, coef)
    xb, hb, mb = x0.clone(), h0.clone(), torch.zeros_like(pair)
    native.cfg_sde_step(xb, pair, hb, nz, mb, coef)
    assert torch.equal(xb, xa) and torch.equal(hb, ha) and torch.equal(mb, ma), f"{row}: kn = 0 differs from mi355x_cfg_linear_step"
    xa, ha, ma = x0.clone(), h0.clone(), torch.zeros_like(x0)
    native.linear_step(xa, u, ha, ma, coef)
    xb, hb, mb = x0.clone(), h0.clone(), torch.zeros_like(x0)
    native.sde_step(xb, u, hb, nz, mb, coef)
    assert torch.equal(xb, xa) and torch.equal(hb, ha) and torch.equal(mb, ma), f"{row}: kn = 0 differs from mi355x_linear_step"


@pytest.mark.parametrize("guided", [False, True], ids=["free", "guided"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_views_off_a_16_byte_boundary_take_the_single_element_loop(dtype, guided):
    n = 4 * 8 * 8  # whole vectors in both types: the aligned call takes the vector loop throughout
    rows = 2 if guided else 1
    bufs = _data((rows * n + 1,), dtype, 24, parts=5)  # x, out, hist, noise, model input
    sizes = (n, rows * n, n, n, rows * n)
    aligned = [b[:k].clone() for b, k in zip(bufs, sizes)]
    off = [torch.cat((b[:1], b[:k]))[1:] for b, k in zip(bufs, sizes)]  # the same values, one element off the boundary
    coef = torch.tensor([7.5, *SDE_ROWS["second_order"]()], dtype=torch.float32, device=DEV)
    step = native.cfg_sde_step if guided else native.sde_step
    x_a, out_a, h_a, z_a, m_a = (t.clone() for t in aligned)
    step(x_a, out_a, h_a, z_a, m_a, coef)
    x_u, out_u, h_u, z_u, m_u = off
    assert all(t.data_ptr() % 16 != 0 for t in off) and torch.equal(x_u, aligned[0])
    step(x_u, out_u, h_u, z_u, m_u, coef)
    assert torch.equal(x_u, x_a) and torch.equal(h_u, h_a) and torch.equal(m_u, m_a) and torch.equal(z_u, z_a)
    # ONE operand off the boundary (the draw) is enough for the single-element loop
    x_b, out_b, h_b, m_b = (aligned[j].clone() for j in (0, 1, 2, 4))
    z_b = torch.cat((bufs[3][:1], bufs[3][:n]))[1:]
    step(x_b, out_b, h_b, z_b, m_b, coef)
    assert torch.equal(x_b, x_a) and torch.equal(h_b, h_a) and torch.equal(m_b, m_a)


def test_refusals_launch_nothing():
    x = torch.ones(8, device=DEV)
    pair = torch.ones(16, device=DEV)
    coef = torch.tensor([1.0, *SDE_ROWS["second_order"]()], dtype=torch.float32, device=DEV)
    lib = native.load()
    p, q, k = x.data_ptr(), pair.data_ptr(), coef.data_ptr()
    for fn, uo in ((lib.mi355x_sde_step, p), (lib.mi355x_cfg_sde_step, q)):
        assert fn(native.MI355X_F32, None, uo, p, p, None, k, 8, None) == -4  # EARG: no latents
        assert fn(native.MI355X_F32, p, None, p, p, None, k, 8, None) == -4  # no UNet output
        assert fn(native.MI355X_F32, p, uo, None, p, None, k, 8, None) == -4  # no history
        assert fn(native.MI355X_F32, p, uo, p, None, None, k, 8, None) == -4  # no draw
        assert fn(native.MI355X_F32, p, uo, p, p, None, None, 8, None) == -4  # no coefficients
        assert fn(native.MI355X_F32, p, uo, p, p, None, k, 0, None) == -4  # n = 0
        assert fn(native.MI355X_F32, p, uo, p, p, None, k, -8, None) == -4
        assert fn(7, p, uo, p, p, None, k, 8, None) == -1  # EDTYPE
    torch.cuda.synchronize()
    assert bool((x == 1).all()) and bool((pair == 1).all())
