"""pytest -m gpu: the guidance-free solver updates (csrc/solver_step.hip: mi355x_ddim_step, mi355x_linear_step), and the recorded bits of all six
entry points of that file's one kernel.

* Bit-equal to the guided entry points on cat(out, out) at any guidance scale: u + s (c - u) with c == u is u, and the rest is ONE device function
  (csrc/solver_update.cuh) called from both instantiations.  A difference of one bit means the two instantiations do not share the arithmetic.
* Bit-equal to what the guided one-element-per-lane kernels and the earlier vector kernels wrote (tests/golden/solver_step_bits.safetensors): the
  test above compares the kernel with itself, this one pins it.
* Against a float64 torch model of the formulas, with the coefficients as the kernel reads them (float32): float32 within 1e-6 (relative l2 and
  relative maximum: a handful of float32 roundings, 6e-8 each, on terms the size of the result); bfloat16 within ONE bfloat16 rounding of the float64
  result, |got - ref| <= 2^-8 |ref|, plus the float32 bound for a float32 value that sits on a rounding tie.
Shapes: the latents of the few-step goldens (1x4x16x16, 1x4x12x20, 3x4x6x10), 1x4x5x7 (140 elements: in bfloat16 a 4-element tail behind 17
vectors) and 1x3x3x7 (63: a tail in both types); and views that start off a 16-byte boundary (the single-element loop throughout)."""
import pytest
import torch

from refiners_amd import native
from refiners_amd.latent_diffusion.sampling import DDIM
from refiners_amd.latent_diffusion.solvers import DPMSolver, Euler, LCMSolver

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 4, 16, 16), (1, 4, 12, 20), (3, 4, 6, 10), (1, 4, 5, 7), (1, 3, 3, 7)]
DTYPES = [torch.float32, torch.bfloat16]
LINEAR_ROWS = {
    "euler_noise": lambda: Euler(4, timesteps_spacing="trailing").linear_step(1),
    "euler_sample": lambda: Euler(4, timesteps_spacing="trailing", model_prediction_type="sample").linear_step(1),
    "dpm_first_order": lambda: DPMSolver(4).linear_step(0),
    "dpm_second_order": lambda: DPMSolver(4).linear_step(2),
    "lcm_noise_in_hist": lambda: LCMSolver(4).linear_step(1),
}


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


def _data(shape, dtype, seed, parts=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(shape, device=DEV, generator=g).to(dtype) for _ in range(parts)]


def _ddim_row(cfg):
    cur, sig, prev, nf = DDIM(4).coefficients(1)
    return torch.tensor([cfg, cur, sig, prev, nf, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)


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
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ddim_step(shape, dtype):
    x0, out = _data(shape, dtype, 11, parts=2)
    n = x0.numel()
    got = None
    for cfg in (1.0, 7.5):
        coef = _ddim_row(cfg)
        xg = x0.clone()
        native.cfg_ddim_step(xg, torch.cat((out, out)).contiguous(), coef)
        xf, mi = x0.clone(), torch.zeros_like(x0)
        native.ddim_step(xf, out, mi, coef)
        assert torch.equal(xf, xg) and torch.equal(mi, xf), f"guidance scale {cfg}: not bit-equal to mi355x_cfg_ddim_step"
        xn = x0.clone()
        native.ddim_step(xn, out, None, coef)  # no model-input buffer
        assert torch.equal(xn, xf)
        got = xf
    c = _ddim_row(1.0).double()
    x, e = x0.double(), out.double()
    ref = c[3] * ((x - c[2] * e) / c[1]) + c[4] * e
    _close(got, ref, dtype, f"ddim {n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("row", list(LINEAR_ROWS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_step(shape, row, dtype):
    x0, out, h0 = _data(shape, dtype, 12)
    n = x0.numel()
    coefs = LINEAR_ROWS[row]()
    got = None
    for cfg in (1.0, 7.5):
        coef = torch.tensor([cfg, *coefs], dtype=torch.float32, device=DEV)
        xg, hg, mg = x0.clone(), h0.clone(), torch.zeros((2 * shape[0],) + shape[1:], device=DEV, dtype=dtype)
        native.cfg_linear_step(xg, torch.cat((out, out)).contiguous(), hg, mg, coef)
        xf, hf, mf = x0.clone(), h0.clone(), torch.zeros_like(x0)
        native.linear_step(xf, out, hf, mf, coef)
        assert torch.equal(xf, xg) and torch.equal(hf, hg), f"{row}, guidance scale {cfg}: not bit-equal to mi355x_cfg_linear_step"
        assert torch.equal(mf, mg[: shape[0]]) and torch.equal(mf, mg[shape[0] :]), f"{row}: model input differs from the guided kernel's"
        xn, hn = x0.clone(), h0.clone()
        native.linear_step(xn, out, hn, None, coef)
        assert torch.equal(xn, xf) and torch.equal(hn, hf)
        got = (xf, hf, mf)
    c = torch.tensor([0.0, *coefs], dtype=torch.float32).double()
    x, e, h = x0.double(), out.double(), h0.double()
    d = c[1] * x + c[2] * e
    ref = c[3] * x + c[4] * e + c[5] * d + c[6] * h
    _close(got[0], ref, dtype, f"{row} x' {n}")
    if float(d.abs().max()) > 0:  # (Euler and LCM keep nothing: d = 0 exactly)
        _close(got[1], d, dtype, f"{row} hist {n}")
    else:
        assert not got[1].any()
    _close(got[2], c[7] * got[0].double(), dtype, f"{row} model input {n}")  # the STORED x' is what the next step scales


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_views_off_a_16_byte_boundary_take_the_single_element_loop(dtype):
    n = 4 * 5 * 7
    bufs = _data((n + 1,), dtype, 13, parts=4)
    x_a, out_a, h_a = (b[:n].clone() for b in bufs[:3])  # aligned copies of the same values
    x_u, out_u, h_u, m_u = (b[1:] for b in (torch.cat((b[:1], b[:n])) for b in bufs))  # the same values, one element off the boundary
    m_a = torch.zeros(n, device=DEV, dtype=dtype)
    coef = torch.tensor([1.0, *LINEAR_ROWS["dpm_second_order"]()], dtype=torch.float32, device=DEV)
    assert x_u.data_ptr() % 16 != 0 and torch.equal(x_u, x_a)
    native.linear_step(x_a, out_a, h_a, m_a, coef)
    native.linear_step(x_u, out_u, h_u, m_u, coef)
    assert torch.equal(x_u, x_a) and torch.equal(h_u, h_a) and torch.equal(m_u, m_a)
    x_a, out_a = (b[:n].clone() for b in bufs[:2])
    x_u, out_u = (b[1:] for b in (torch.cat((b[:1], b[:n])) for b in bufs[:2]))
    native.ddim_step(x_a, out_a, None, _ddim_row(1.0))
    native.ddim_step(x_u, out_u, None, _ddim_row(1.0))
    assert torch.equal(x_u, x_a)


def test_bits_are_the_parent_commits():
    """Every entry point, on the inputs stored in tests/golden/solver_step_bits.safetensors (tests/solver_step_cases.py), writes the bits that the
    library before the move onto one kernel wrote: the guided scalar kernels, whose fused operations the compiler chose, were the anchor of every
    bit-equality test above and in the neighbouring files, and this record is what is left of them.  No tolerance, nothing skipped."""
    from safetensors.torch import load_file

    from tests import solver_step_cases as SC

    gold = load_file(str(SC.GOLD))
    coefs = {k: gold[k] for k in ("coef.linear", "coef.ddim")}
    assert all(torch.equal(v, coefs[k]) for k, v in SC.coefficient_rows().items())  # the rows the issue names are the rows recorded
    visited = 0
    for tname, dtype in SC.DTYPES.items():
        for layout in SC.LAYOUTS:
            inp = {k: gold[f"{tname}.{layout}.in.{k}"] for k in ("x", "unet_out", "hist", "noise")}
            assert all(v.dtype == dtype for v in inp.values())
            for entry, (_, _, has_hist, _, has_model_in) in SC.ENTRIES.items():
                got = SC.run(native, entry, layout, inp, coefs)
                assert set(got) == {"x"} | ({"hist"} if has_hist else set()) | ({"model_in"} if has_model_in else set())
                for k, v in got.items():
                    want = gold[f"{tname}.{layout}.{entry}.{k}"]
                    assert torch.equal(v, want), f"{tname} {layout} {entry}: {k} differs in {int((v != want).sum())} of {v.numel()} elements"
                visited += 1
    assert visited == 48


def test_refusals_launch_nothing():
    x = torch.ones(8, device=DEV)
    coef = _ddim_row(1.0)
    lib = native.load()
    assert lib.mi355x_ddim_step(native.MI355X_F32, x.data_ptr(), None, None, coef.data_ptr(), 8, None) < 0  # EARG: no UNet output
    assert lib.mi355x_linear_step(native.MI355X_F32, x.data_ptr(), x.data_ptr(), None, None, coef.data_ptr(), 8, None) < 0  # EARG: no history
    assert lib.mi355x_linear_step(7, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, coef.data_ptr(), 8, None) < 0  # EDTYPE
    assert lib.mi355x_ddim_step(native.MI355X_F32, x.data_ptr(), x.data_ptr(), None, coef.data_ptr(), 0, None) < 0  # EARG: n = 0
    torch.cuda.synchronize()
    assert bool((x == 1).all())
