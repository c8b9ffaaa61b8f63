"""mi355x_ella_adaln (include/mi355x_refiners_ella.h, csrc/ella.hip) and the squared-ReLU epilogue of mi355x_gemm (code 5) against float64 torch,
float32 and bfloat16, at the smallest shapes that reach each branch.

Inputs are rounded to the tested dtype first and the reference is computed in float64 from the rounded values (tests/ella_cases.adaln_model).
Bars of the AdaLayerNorm pass: float32 within 1e-5 of the row's largest magnitude (two-pass statistics over at most 768 float32 values and a
handful of roundings; measured values are printed); bfloat16 adds the output's one rounding, 2^-8 |y|.  The GEMM is held to
tests/kernel_cases._tol, the bar of the library's other activation epilogues (tests/kernel_cases.gemm_gelu_case)."""
import pytest
import torch

from refiners_amd import native
from tests.ella_cases import adaln_model
from tests.kernel_cases import _tol

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
OK, ESHAPE, EARG = 0, -2, -4


def _randn(*shape, dtype, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(device=DEV, dtype=dtype)


def _pad64(n):
    return (n + 63) // 64 * 64


def _check(out, ref, dtype, what):
    """out, ref: [B, Lp, C].  |err| <= 1e-5 max_row |ref| (+ 2^-8 |ref| in bfloat16)."""
    got, ref = out.double(), ref.double()
    assert torch.isfinite(got).all(), what
    bound = 1e-5 * ref.abs().amax(-1, keepdim=True) + (ref.abs() * 2.0**-8 if dtype == torch.bfloat16 else 0)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    print(f"{what}: max |err| = {float(err.max()):.3e}, max err / bound = {float(ratio.max()):.3f}")
    assert bool((err <= bound).all()), (what, float(ratio.max()))


def _table(B, C, dtype, seed, extra=24):
    """A time table [B, 4 C + extra] (leading dimension larger than any slice): shift_l | scale_l | shift_x | scale_x, scale rows of order 0.5,
    different per batch row."""
    t = _randn(B, 4 * C + extra, dtype=dtype, seed=seed, scale=0.5)
    return t, [t[:, i * C:(i + 1) * C] for i in range(4)]


def _run(lat, x, mods, Lp, dtype, eps=1e-6):
    """Launch into a NaN-filled [B, Lp + 1, C] buffer (a batch stride of its own): (out[:, :Lp], the guard row)."""
    B, Nl, C = lat.shape
    buf = torch.full((B, Lp + 1, C), NAN, device=DEV, dtype=dtype)
    if x is None:
        native.ella_adaln(lat, mods[0], mods[1], buf[:, :Lp], eps=eps)
    else:
        native.ella_adaln(lat, mods[0], mods[1], buf[:, :Lp], x=x, shift_x=mods[2], scale_x=mods[3], eps=eps)
    torch.cuda.synchronize()
    return buf[:, :Lp], buf[:, Lp]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [0, 1, 5, 77, 128])
@pytest.mark.parametrize("C,Nl", [(64, 16), (64, 64), (768, 16), (768, 64)])
def test_adaln_rows_against_float64(C, Nl, T, dtype):
    B = 2
    lat = _randn(B, Nl, C, dtype=dtype, seed=C + Nl + T, scale=3.0)
    x = _randn(B, T, C + 8, dtype=dtype, seed=C + Nl + T + 1)[:, :, :C] if T else None  # text rows with a leading dimension of their own
    _tab, mods = _table(B, C, dtype, seed=7 * C + T)
    for Lp in ([_pad64(Nl + T)] if T else sorted({Nl, _pad64(Nl)})):
        out, guard = _run(lat, x, mods, Lp, dtype)
        ref = adaln_model(lat, mods[0], mods[1], Lp, x, mods[2], mods[3])
        _check(out, ref, dtype, f"adaln C {C} Nl {Nl} T {T} Lp {Lp} {dtype}")
        assert bool((out[:, Nl + T:] == 0).all()), "padding rows are exact zeros although the buffer held NaN"
        assert torch.isnan(guard.float()).all(), "nothing past the Lp rows of a batch row is written"
    assert not torch.equal(out[0, :Nl], out[1, :Nl])  # per-row modulation


@pytest.mark.parametrize("dtype", DTYPES)
def test_adaln_statistics_hold_where_a_one_pass_variance_fails(dtype):
    """A row whose mean is 50 x its standard deviation (E[x^2] - E[x]^2 would lose the variance in float32), and a constant row: its variance
    is 0, eps decides, and the result is exactly the shift row."""
    B, Nl, T, C = 2, 16, 5, 768
    lat = _randn(B, Nl, C, dtype=torch.float32, seed=1) + 50.0
    lat[1, 3] = 7.25  # constant row
    lat = lat.to(dtype)
    x = (_randn(B, T, C, dtype=torch.float32, seed=2) * 0.01 + 0.5).to(dtype)
    x[0, 2] = -3.0
    _tab, mods = _table(B, C, dtype, seed=3)
    Lp = _pad64(Nl + T)
    out, _guard = _run(lat, x, mods, Lp, dtype)
    _check(out, adaln_model(lat, mods[0], mods[1], Lp, x, mods[2], mods[3]), dtype, f"adaln offset and constant rows {dtype}")
    assert torch.equal(out[1, 3], mods[0][1]) and torch.equal(out[0, Nl + 2], mods[2][0]), "a constant row gives the shift row, bit for bit"


def _recorded(call):
    ops = []
    with native.recording(ops):
        call()
    fn, args, _what, _keep = ops[0]
    return fn, args


def test_adaln_refuses_what_it_cannot_run():
    B, Nl, T, C = 2, 16, 5, 64
    dtype = torch.float32
    lat, x = _randn(B, Nl, C, dtype=dtype, seed=1), _randn(B, T, C, dtype=dtype, seed=2)
    _tab, mods = _table(B, C, dtype, seed=3)
    out = torch.full((B, 64, C), NAN, device=DEV, dtype=dtype)
    call = lambda: native.ella_adaln(lat, mods[0], mods[1], out, x=x, shift_x=mods[2], scale_x=mods[3])  # noqa: E731
    changes = [
        ("C whose rows are no multiple of 16 bytes", {"C": 6}, ESHAPE),
        ("C above 4096", {"C": 4100}, ESHAPE),
        ("fewer rows than Nl + T", {"Lp": Nl + T - 1}, ESHAPE),
        ("a row stride below C", {"ldo": C - 4}, ESHAPE),
        ("a misaligned row stride", {"ldx": C + 2}, ESHAPE),
        ("a misaligned pointer", {"latents": lat.data_ptr() + 4}, ESHAPE),
        ("a misaligned time-table stride", {"mod_batch_stride": 4 * C + 22}, ESHAPE),
        ("batch rows that overlap", {"out_batch_stride": C}, ESHAPE),
        ("no text rows", {"x": None}, EARG),
        ("in place", {"out": lat.data_ptr()}, EARG),
        ("a dtype the library does not know", {"dtype": 7}, -1),
    ]
    for what, change, status in changes:
        fn, args = _recorded(call)
        for k, v in change.items():
            setattr(args[0]._obj, k, v)
        assert fn(*args, native.stream_ptr()) == status, what
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote"
    fn, args = _recorded(call)
    assert fn(*args, native.stream_ptr()) == OK
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------------------ squared ReLU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("M,N", [(1, 64), (1, 3072), (128, 64), (128, 3072)])
def test_gemm_squared_relu_epilogue(M, N, res, dtype):
    """geglu == 5: out = max(x W^T + b, 0)^2 (+ res).  A library without the code applies no activation: negative pre-activations then stay negative."""
    K = 768
    x, w = _randn(M, K, dtype=dtype, seed=M + N), _randn(N, K, dtype=dtype, seed=M + N + 1, scale=K**-0.5)
    b = _randn(N, dtype=dtype, seed=M + N + 2)
    r = _randn(M, N, dtype=dtype, seed=M + N + 3) if res else None
    out = torch.empty(M, N, device=DEV, dtype=dtype)
    native.gemm([(x, w)], out, bias=b, res=r, squared_relu=True)
    torch.cuda.synchronize()
    pre = x.double() @ w.double().t() + b.double()
    assert bool((pre < -0.1).any()) and bool((pre > 0.1).any())
    ref = torch.relu(pre) ** 2 + (r.double() if res else 0)
    err, scale = float((out.double() - ref).abs().max()), float(ref.abs().max())
    print(f"squared ReLU {M}x{N}x{K} res {res} {dtype}: max |err| / max |ref| = {err / scale:.3e} (bar {_tol(dtype):.1e})")
    assert torch.isfinite(out.float()).all() and err <= _tol(dtype) * scale
    if not res:
        assert bool((out.float() >= 0).all())
