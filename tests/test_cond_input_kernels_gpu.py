"""pytest -m gpu: the kernels of step-constant UNet input channels (csrc/cond_input.hip: mi355x_cond_step, mi355x_cond_fill,
mi355x_inpaint_conditions).

The comparisons of cond_step / cond_fill are EXACT (torch.equal), so there is no tolerance:
* x and hist are bit-equal to the existing step kernel on the same operands (cfg_ddim_step, cfg_linear_step, ddim_step, linear_step: one set of
  device functions, csrc/solver_update.cuh);
* the latent channels of model_in are the existing kernel's model_in, re-strided into the C + E channel images (guided DDIM has none: the stored x');
* the constant channels are (cond.float() * s).to(dtype), one float32 product and one rounding; with cond = None they keep a sentinel.
Shapes: hw = 35 (5 x 7: single elements, a channel row ends off every 16-byte boundary) and 64 (8 x 8: 16-byte vectors); n in {1, 3}; C = 4;
E in {0, 4, 5}; the constants of batch 1 or n; both storage types, both forms, guided and not.
inpaint_conditions: the mask latents are exactly torch's nearest interpolation; the masked image is within 4 float32 ulp at 1 (5e-7: two roundings
of a value in [-1, 1] and a division whose last bit may differ) of the torch expression in float32, within one bfloat16 ulp at 1 (2^-8) in
bfloat16, and exactly 0 under the mask."""
import itertools

import pytest
import torch

from refiners_amd import native
from refiners_amd.latent_diffusion.sampling import DDIM

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
C = 4
GEOMETRIES = [(h, w, n, E, nc) for (h, w), n, E in itertools.product([(5, 7), (8, 8)], [1, 3], [0, 4, 5]) for nc in sorted({1, n})]
LINEAR_ROW = [7.5, 0.7, -0.3, 1.1, -0.4, 0.25, 0.15, 0.83]  # (cfg, hx, he, kx, ke, kd, kp, s_next): every term live, an input scale that is not 1
SENTINEL = 123.0
EARG = -4


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


def _coef(linear):
    if linear:
        return torch.tensor(LINEAR_ROW, dtype=torch.float32, device=DEV)
    cur, sig, prev, nf = DDIM(4).coefficients(1)
    return torch.tensor([7.5, cur, sig, prev, nf, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)


def _randn(shape, dtype, g, misalign=False):
    """Seeded values; misalign: the same values in a view that starts one element behind a 16-byte boundary."""
    t = torch.randn(shape, device=DEV, generator=g).to(dtype)
    if not misalign:
        return t
    n = t.numel()
    buf = torch.empty(n + 1, device=DEV, dtype=dtype)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _existing(x, uo, hist, coef, linear, guided):
    """The existing kernel on clones: (x', hist', latent part of the model input [B, C, h, w])."""
    n = x.shape[0]
    xr, hr = x.clone(), hist.clone()
    mr = torch.zeros((2 * n if guided else n,) + tuple(x.shape[1:]), device=DEV, dtype=x.dtype)
    if linear:
        (native.cfg_linear_step if guided else native.linear_step)(xr, uo.clone(), hr, mr, coef)
    elif guided:
        native.cfg_ddim_step(xr, uo.clone(), coef)
        mr = torch.cat((xr, xr))
    else:
        native.ddim_step(xr, uo.clone(), mr, coef)
    return xr, hr, mr


def _step_case(dtype, linear, guided, h, w, n, E, nc, with_cond, misalign=False):
    g = torch.Generator(device=DEV).manual_seed(17 + h * w + 7 * n + E)
    B = 2 * n if guided else n
    x, hist, uo = _randn((n, C, h, w), dtype, g, misalign), _randn((n, C, h, w), dtype, g), _randn((B, C, h, w), dtype, g)
    cond = _randn((nc, E, h, w), dtype, g) if (with_cond and E > 0) else None
    coef = _coef(linear)
    xr, hr, mr = _existing(x, uo, hist, coef, linear, guided)
    model_in = torch.full((B, C + E, h, w), SENTINEL, device=DEV, dtype=dtype)
    hist_before = hist.clone()
    native.cond_step(x, uo, hist, model_in, cond, coef, linear, guided)
    what = (str(dtype), linear, guided, h, w, n, E, nc, with_cond)
    assert torch.equal(x, xr), ("x", what)
    assert torch.equal(hist, hr if linear else hist_before), ("hist", what)
    assert torch.equal(model_in[:, :C], mr), ("latent channels of model_in", what)
    if E:
        if cond is None:
            assert bool((model_in[:, C:] == SENTINEL).all()), ("NULL cond must leave the constant channels alone", what)
        else:
            s = LINEAR_ROW[7] if linear else 1.0
            want = (cond.float() * torch.tensor(s, dtype=torch.float32, device=DEV)).to(dtype)
            want = want.expand(n, E, h, w).repeat(B // n, 1, 1, 1)
            assert torch.equal(model_in[:, C:], want), ("constant channels of model_in", what)


@pytest.mark.parametrize("guided", [True, False], ids=["guided", "free"])
@pytest.mark.parametrize("linear", [False, True], ids=["ddim", "linear"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_cond_step_is_the_existing_update_plus_the_extended_model_input(dtype, linear, guided):
    for h, w, n, E, nc in GEOMETRIES:
        for with_cond in ((True, False) if E else (False,)):
            _step_case(dtype, linear, guided, h, w, n, E, nc, with_cond)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_cond_step_behind_a_misaligned_pointer_takes_single_elements(dtype):
    for linear, guided in itertools.product((False, True), (False, True)):
        _step_case(dtype, linear, guided, 8, 8, 3, 5, 3, True, misalign=True)  # hw = 64 would be the vector path


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_cond_fill(dtype):
    s_dev = torch.tensor([0.83], dtype=torch.float32, device=DEV)
    for (h, w, n, E, nc), double, s, with_x in itertools.product(GEOMETRIES, (False, True), (None, s_dev), (True, False)):
        if not with_x and E == 0:
            continue  # nothing to write: refused, see test_refusals_launch_nothing
        g = torch.Generator(device=DEV).manual_seed(29 + h * w + 7 * n + E)
        B = 2 * n if double else n
        x = _randn((n, C, h, w), dtype, g)
        cond = _randn((nc, E, h, w), dtype, g) if E else None
        model_in = torch.full((B, C + E, h, w), SENTINEL, device=DEV, dtype=dtype)
        native.cond_fill(x if with_x else None, cond, model_in, s, n, C)
        sv = s_dev[0] if s is not None else torch.tensor(1.0, device=DEV)
        what = (str(dtype), h, w, n, E, nc, double, s is not None, with_x)
        if with_x:
            assert torch.equal(model_in[:, :C], (x.float() * sv).to(dtype).repeat(B // n, 1, 1, 1)), ("latent channels", what)
        else:
            assert bool((model_in[:, :C] == SENTINEL).all()), ("NULL x must leave the latent channels alone", what)
        if E:
            assert torch.equal(model_in[:, C:], (cond.float() * sv).to(dtype).expand(n, E, h, w).repeat(B // n, 1, 1, 1)), ("constant channels", what)
    # a view one element off a 16-byte boundary: single elements, the same values
    g = torch.Generator(device=DEV).manual_seed(31)
    x, cond = _randn((3, C, 8, 8), dtype, g, misalign=True), _randn((3, 5, 8, 8), dtype, g)
    model_in = torch.full((6, C + 5, 8, 8), SENTINEL, device=DEV, dtype=dtype)
    native.cond_fill(x, cond, model_in, s_dev, 3, C)
    assert torch.equal(model_in[:, :C], (x.float() * s_dev[0]).to(dtype).repeat(2, 1, 1, 1))
    assert torch.equal(model_in[:, C:], (cond.float() * s_dev[0]).to(dtype).repeat(2, 1, 1, 1))


def test_refusals_launch_nothing():
    lib = native.load()
    n, E, hw = 3, 4, 64
    F32, LIN = native.MI355X_F32, 1
    x = torch.ones(n * C * hw, device=DEV)
    hist, uo, cond = torch.ones_like(x), torch.ones(2 * n * C * hw, device=DEV), torch.ones(n * E * hw, device=DEV)
    mi = torch.ones(2 * n * (C + E) * hw, device=DEV)
    coef = _coef(True)
    p = lambda t: t.data_ptr()  # noqa: E731

    def step(x_=p(x), uo_=p(uo), hist_=p(hist), mi_=p(mi), cond_=p(cond), coef_=p(coef), n_=n, C_=C, E_=E, nc_=n, hw_=hw, dtype=F32, form=LIN, guided=1):
        return lib.mi355x_cond_step(dtype, form, guided, x_, uo_, hist_, mi_, cond_, coef_, n_, C_, E_, nc_, hw_, None)

    for name, kw in {"x NULL": dict(x_=None), "unet_out NULL": dict(uo_=None), "model_in NULL": dict(mi_=None), "coef NULL": dict(coef_=None),
                     "hist NULL with LINEAR": dict(hist_=None), "n = 0": dict(n_=0), "C = 0": dict(C_=0), "hw = 0": dict(hw_=0), "E < 0": dict(E_=-1),
                     "nc outside {1, n}": dict(nc_=2), "form": dict(form=2), "guided": dict(guided=2),
                     "model_in over x": dict(mi_=p(x)), "model_in over hist": dict(mi_=p(hist)), "model_in over unet_out": dict(mi_=p(uo)),
                     "model_in over cond": dict(mi_=p(cond)), "model_in ends inside x": dict(x_=p(mi) + 4 * (mi.numel() - 8))}.items():
        assert step(**kw) == EARG, name
    assert step(dtype=7) == -1  # EDTYPE

    def fill(x_=p(x), cond_=p(cond), mi_=p(mi), n_=n, B_=2 * n, C_=C, E_=E, nc_=n, hw_=hw):
        return lib.mi355x_cond_fill(F32, x_, cond_, mi_, None, n_, B_, C_, E_, nc_, hw_, None)

    for name, kw in {"model_in NULL": dict(mi_=None), "x and cond NULL": dict(x_=None, cond_=None), "n = 0": dict(n_=0, B_=0), "C = 0": dict(C_=0),
                     "hw = 0": dict(hw_=0), "E < 0": dict(E_=-1), "B outside {n, 2n}": dict(B_=n + 1), "nc outside {1, n}": dict(nc_=2),
                     "cond with E = 0": dict(E_=0), "model_in over x": dict(mi_=p(x)), "model_in over cond": dict(mi_=p(cond))}.items():
        assert fill(**kw) == EARG, name

    img, msk = torch.ones(2 * 8 * 8 * 3, dtype=torch.uint8, device=DEV), torch.ones(2 * 8 * 8, dtype=torch.uint8, device=DEV)

    def inpaint(img_=p(img), msk_=p(msk), out_=p(mi), ml_=p(x), n_=2, nm_=2, H=8, W=8, h=2, w=2):
        return lib.mi355x_inpaint_conditions(F32, img_, msk_, out_, ml_, n_, nm_, H, W, h, w, None)

    for name, kw in {"image NULL": dict(img_=None), "mask NULL": dict(msk_=None), "out NULL": dict(out_=None), "mask latents NULL": dict(ml_=None),
                     "n = 0": dict(n_=0), "nm outside {1, n}": dict(nm_=3), "H = 0": dict(H=0), "w = 0": dict(w=0)}.items():
        assert inpaint(**kw) == EARG, name
    torch.cuda.synchronize()
    for t in (x, hist, uo, cond, mi):
        assert bool((t == 1).all())


@pytest.fixture(scope="module")
def picture():
    """A seeded 40 x 56 uint8 picture pair and masks whose values include 0, 127, 128 and 255 (the threshold sits between the middle two)."""
    g = torch.Generator().manual_seed(5)
    image = torch.randint(0, 256, (2, 40, 56, 3), generator=g, dtype=torch.uint8)
    mask = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)[torch.randint(0, 4, (2, 40, 56), generator=g)]
    return image.to(DEV), mask.to(DEV)


@pytest.mark.parametrize("size", [(5, 7), (7, 9)], ids=["5x7", "7x9"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_inpaint_conditions(picture, dtype, size):
    for n, nm in ((1, 1), (2, 1), (2, 2)):
        image, mask = picture[0][:n].contiguous(), picture[1][:nm].contiguous()
        masked = torch.full((n, 3, 40, 56), SENTINEL, device=DEV, dtype=dtype)
        ml = torch.full((nm, 1) + size, SENTINEL, device=DEV, dtype=dtype)
        native.inpaint_conditions(image, mask, masked, ml)
        m = (mask.float() / 255.0 > 0.5).unsqueeze(1).float()
        assert set(m.unique().tolist()) == {0.0, 1.0}
        assert torch.equal(ml.float(), torch.nn.functional.interpolate(m, size=size, mode="nearest")), (n, nm, size)
        ref = ((image.permute(0, 3, 1, 2).float() / 255.0) * 2 - 1) * (1 - m)
        err = float((masked.float() - ref).abs().max())
        bound = 5e-7 if dtype == torch.float32 else 2.0**-8
        print(f"inpaint_conditions {dtype} n {n} nm {nm} -> {size}: max |masked - ref| = {err:.3e} (bound {bound:.1e})")
        assert err <= bound, (n, nm, size, err)
        assert bool((masked.float()[(m == 1).expand(n, 3, 40, 56)] == 0).all())
