"""The HQ-SAM kernels (csrc/sam_hq.hip) against float32 torch on the GPU: the folded 3x3 mask head at shapes where every pixel touches a
border, where tiles meet in both directions and at 2 x 2; the mask head that also stores the upscaled embedding; LayerNorm2d + GELU + 2x
scatter at 128 and 256 channels; and the refusals of the three entry points.

Inputs are rounded to the tested dtype first and the reference is computed from the rounded values, so what separates the kernels from it
is float32 arithmetic and, for bfloat16, one rounding of the output: the bounds are KTOL of tests/test_sam_decoder_gpu.py (relative l2
1e-5 float32, 2^-8 bfloat16), for the same reason."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from refiners_amd import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.bfloat16]
KTOL = {torch.float32: 1e-5, torch.bfloat16: 2.0**-8}
NAN = float("nan")
OK, EDTYPE, ESHAPE, EARG = 0, -1, -2, -4
EPS = 1e-6


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _untouched(t, what=""):
    assert torch.isnan(t.float()).all(), f"{what}: {int((~torch.isnan(t.float())).sum())} elements written"


def _quadrants(f):
    """[H, W, 32] -> the quadrant layout [(H/2) (W/2), 128]: pixel (y, x) = row (y >> 1) (W/2) + (x >> 1), columns ((y & 1) 2 + (x & 1)) 32 + c."""
    H, W, C = f.shape
    return f.view(H // 2, 2, W // 2, 2, C).permute(0, 2, 1, 3, 4).reshape((H // 2) * (W // 2), 4 * C)


def _hq_inputs(P, H, W, dtype, seed, constant_y=False):
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    y = (torch.full((P, H, W, 64), 0.37, device=DEV) if constant_y else r(P, H, W, 64) * 2 + r(P, H, W, 1)).to(dtype)
    gamma, beta = 1 + 0.1 * r(64), 0.5 * r(64)
    w2, b2 = r(32, 64, 3, 3) / 24, 0.1 * r(32)
    h = r(P, 32).to(dtype)
    f = r(H, W, 32).to(dtype)
    return y, gamma, beta, w2, b2, h, f


def _hq_ref(y, gamma, beta, w2, b2, h, f):
    z = F.gelu(F.layer_norm(y.float(), (64,), gamma, beta, EPS)).permute(0, 3, 1, 2)
    feat = F.conv2d(z, w2, b2, padding=1) + f.float().permute(2, 0, 1)
    return torch.einsum("pc,pchw->phw", h.float(), feat).unsqueeze(1)


def _hq_run(y, gamma, beta, w2, b2, h, f):
    """The engine's operand shapes: y rows with ldy = 72 (NaN pad columns), h a strided view of [P, 3, 48], an output plane more than asked."""
    P, H, W, _ = y.shape
    ybuf = torch.full((P * H * W, 72), NAN, device=DEV, dtype=y.dtype)
    ybuf[:, :64] = y.reshape(-1, 64)
    hbuf = torch.full((P, 3, 48), NAN, device=DEV, dtype=y.dtype)
    hbuf[:, 1, 8:40] = h
    obuf = torch.full((P + 1, 1, H, W), NAN, device=DEV, dtype=y.dtype)
    args = (ybuf[:, :64], P, H, W, gamma, beta, EPS, w2.permute(0, 2, 3, 1).reshape(32, 9, 64).contiguous(), b2, hbuf[:, 1, 8:40], _quadrants(f).contiguous(), obuf[:P])
    native.sam_hq_mask_head(*args)
    first = obuf.clone()
    native.sam_hq_mask_head(*args)
    assert torch.equal(obuf[:P], first[:P]), "two calls differ"
    _untouched(obuf[P:], "the plane after the last prompt")
    return obuf[:P]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,H,W", [(3, 6, 10), (2, 34, 18), (1, 2, 2)])
def test_sam_hq_mask_head(dtype, P, H, W):
    """6 x 10: every pixel is at or next to a border; 34 x 18: tiles of 16 x 8 meet in both directions (halos between tiles); 2 x 2."""
    inputs = _hq_inputs(P, H, W, dtype, 400 + H)
    out = _hq_run(*inputs)
    assert torch.isfinite(out.float()).all()
    err = _rel(out.float(), _hq_ref(*inputs))
    print(f"sam_hq_mask_head {dtype} P={P} {H}x{W}: rel l2 {err:.3e}")
    assert err < KTOL[dtype], err


@pytest.mark.parametrize("dtype", DTYPES)
def test_sam_hq_mask_head_zero_pads_the_activated_tensor(dtype):
    """A constant y makes z = GELU(beta) at every pixel: a halo of GELU(LayerNorm2d(0)) would be that same constant instead of 0, and every
    border pixel would be wrong by whole taps."""
    inputs = _hq_inputs(2, 10, 20, dtype, 410, constant_y=True)
    out, ref = _hq_run(*inputs), _hq_ref(*inputs)
    assert float((ref[..., 0, :] - ref[..., 4, :]).abs().max()) > 0.05 * float(ref.abs().max())  # (the border is visible in the reference)
    err = _rel(out.float(), ref)
    print(f"sam_hq_mask_head constant y {dtype}: rel l2 {err:.3e}")
    assert err < KTOL[dtype], err
    edge = torch.cat([(out.float() - ref)[..., 0, :].flatten(), (out.float() - ref)[..., -1, :].flatten(), (out.float() - ref)[..., :, 0].flatten(), (out.float() - ref)[..., :, -1].flatten()])
    assert float(edge.abs().max()) <= 4 * KTOL[dtype] * float(ref.abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_sam_mask_head_up(dtype):
    g = _gen(420)
    P, Hin, Win, nk = 2, 5, 7, 1
    x = torch.randn(P, Hin, Win, 64, device=DEV, generator=g).to(dtype)
    weight = torch.randn(64, 32, 2, 2, device=DEV, generator=g) / 8
    bias = torch.randn(32, device=DEV, generator=g)
    hyper = torch.randn(P, 4, 32, device=DEV, generator=g).to(dtype)
    rows = x.reshape(-1, 64).contiguous()
    w = weight.permute(0, 2, 3, 1).reshape(64, 128).contiguous()
    base = torch.full((P, nk, 2 * Hin, 2 * Win), NAN, device=DEV, dtype=dtype)
    native.sam_mask_head(rows, P, Hin, Win, w, bias, hyper[:, :nk], base)
    out = torch.full((P, nk, 2 * Hin, 2 * Win), NAN, device=DEV, dtype=dtype)
    ubuf = torch.full((4 * P * Hin * Win, 64), NAN, device=DEV, dtype=dtype)
    native.sam_mask_head_up(rows, P, Hin, Win, w, bias, hyper[:, :nk], out, ubuf)
    assert torch.isfinite(base.float()).all() and torch.equal(out, base)
    up = F.gelu(F.conv_transpose2d(x.float().permute(0, 3, 1, 2), weight, bias, stride=2)).permute(0, 2, 3, 1).reshape(-1, 32)
    assert _rel(ubuf[:, :32].float(), up) < KTOL[dtype]
    _untouched(ubuf[:, 32:], "columns 32.. of u")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [128, 256])
def test_ln2d_gelu_wide(dtype, C):
    g = _gen(430 + C)
    P, Hs, Ws = 2, 4, 6
    M = P * Hs * Ws
    x = (torch.randn(M, 4, C, device=DEV, generator=g) * 2 + torch.randn(M, 4, 1, device=DEV, generator=g)).to(dtype)
    gamma, beta = 1 + 0.1 * torch.randn(C, device=DEV, generator=g), 0.5 * torch.randn(C, device=DEV, generator=g)
    xbuf = torch.full((M, 4 * C + 8), NAN, device=DEV, dtype=dtype)
    xbuf[:, : 4 * C] = x.reshape(M, 4 * C)
    obuf = torch.full((4 * M + 1, C + 8), NAN, device=DEV, dtype=dtype)
    native.ln2d_gelu_wide(xbuf[:, : 4 * C], C, gamma, beta, EPS, obuf[: 4 * M, :C], (Hs, Ws))
    ref = F.gelu(F.layer_norm(x.float(), (C,), gamma, beta, EPS))  # [(p, y, x), (dy, dx), c]
    ref = ref.view(P, Hs, Ws, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(4 * M, C)
    assert torch.isfinite(obuf[: 4 * M, :C].float()).all() and _rel(obuf[: 4 * M, :C].float(), ref) < KTOL[dtype]
    _untouched(obuf[:, C:], "pad columns")
    _untouched(obuf[4 * M :], "the row after the last one")


# ------------------------------------------------------------------------------------------------ refusals of the C entry points
def _status(fn, *args):
    st = fn(*args, native.stream_ptr())
    torch.cuda.synchronize()
    return st


def _hq_args(H=6, W=10, dtype=native.MI355X_F32, w2_offset=0, null=None):
    P = 2
    keep = dict(y=torch.zeros(P * 8 * 12, 64, device=DEV), gamma=torch.ones(64, device=DEV), beta=torch.zeros(64, device=DEV), w2=torch.zeros(32 * 9 * 64 + 8, device=DEV),
                b2=torch.zeros(32, device=DEV), h=torch.zeros(P, 32, device=DEV), fq=torch.zeros(4 * 6, 128, device=DEV), out=torch.full((P, 1, 8, 12), NAN, device=DEV))
    a = native.SamHqMaskHeadArgs()
    a.dtype, a.P, a.H, a.W = dtype, P, H, W
    a.y, a.ldy, a.gamma, a.beta, a.eps = keep["y"].data_ptr(), 64, keep["gamma"].data_ptr(), keep["beta"].data_ptr(), EPS
    a.w2, a.b2 = keep["w2"].data_ptr() + w2_offset, keep["b2"].data_ptr()
    a.h, a.h_stride, a.fq, a.ldf = keep["h"].data_ptr(), 32, keep["fq"].data_ptr(), 128
    a.out, a.out_batch_stride = keep["out"].data_ptr(), 8 * 12
    if null:
        setattr(a, null, None)
    return a, keep


def test_sam_hq_mask_head_refusals():
    lib = native.load()
    cases = [("odd H", dict(H=5), ESHAPE), ("odd W", dict(W=9), ESHAPE), ("w2 4 bytes off 16-byte alignment", dict(w2_offset=4), ESHAPE),
             ("unknown dtype", dict(dtype=7), EDTYPE)] + [(f"{f} NULL", dict(null=f), EARG) for f in ("y", "gamma", "beta", "w2", "b2", "h", "fq")]
    for what, kw, want in cases:
        a, keep = _hq_args(**kw)
        assert _status(lib.mi355x_sam_hq_mask_head, ctypes.byref(a)) == want, what
        _untouched(keep["out"], what)
    a, keep = _hq_args(null="out")
    assert _status(lib.mi355x_sam_hq_mask_head, ctypes.byref(a)) == EARG
    a, keep = _hq_args(w2_offset=16)  # 16-byte aligned: accepted
    assert _status(lib.mi355x_sam_hq_mask_head, ctypes.byref(a)) == OK
    planes = keep["out"].reshape(2, -1)  # [6][10] contiguous at the head of each prompt's 96 elements
    assert torch.isfinite(planes[:, :60]).all() and torch.isnan(planes[:, 60:]).all()


def _up_args(nk=1, w_offset=0, ldu=32, u_offset=0, dtype=native.MI355X_F32, null_u=False):
    P, Hin, Win = 2, 5, 7
    keep = dict(x=torch.zeros(P * Hin * Win, 64, device=DEV), w=torch.zeros(64 * 128 + 8, device=DEV), b=torch.zeros(32, device=DEV), hyper=torch.zeros(P, 5, 32, device=DEV),
                out=torch.full((P, 5, 2 * Hin, 2 * Win), NAN, device=DEV), u=torch.full((4 * P * Hin * Win + 1, 40), NAN, device=DEV))
    a = native.SamMaskHeadUpArgs()
    a.dtype, a.P, a.Hin, a.Win, a.nk = dtype, P, Hin, Win, nk
    a.x, a.ldx, a.w, a.bias = keep["x"].data_ptr(), 64, keep["w"].data_ptr() + w_offset, keep["b"].data_ptr()
    a.hyper, a.ld_hyper, a.hyper_batch_stride = keep["hyper"].data_ptr(), 32, 5 * 32
    a.out, a.out_batch_stride = keep["out"].data_ptr(), 5 * 4 * Hin * Win
    a.u, a.ldu = (None if null_u else keep["u"].data_ptr() + u_offset), ldu
    return a, keep


def test_sam_mask_head_up_refusals():
    lib = native.load()
    cases = [("nk = 0", dict(nk=0), ESHAPE), ("nk = 5", dict(nk=5), ESHAPE), ("w misaligned", dict(w_offset=4), ESHAPE), ("ldu = 24", dict(ldu=24), ESHAPE),
             ("ldu = 34", dict(ldu=34), ESHAPE), ("u 4 bytes off", dict(u_offset=4), ESHAPE), ("unknown dtype", dict(dtype=7), EDTYPE), ("u NULL", dict(null_u=True), EARG)]
    for what, kw, want in cases:
        a, keep = _up_args(**kw)
        assert _status(lib.mi355x_sam_mask_head_up, ctypes.byref(a)) == want, what
        _untouched(keep["out"], what)
        _untouched(keep["u"], what)
    a, keep = _up_args(ldu=40)
    assert _status(lib.mi355x_sam_mask_head_up, ctypes.byref(a)) == OK
    assert torch.isfinite(keep["out"][:, :1]).all() and torch.isnan(keep["out"][:, 1:]).all()
    assert torch.isfinite(keep["u"][:-1, :32]).all() and torch.isnan(keep["u"][:, 32:]).all() and torch.isnan(keep["u"][-1]).all()


def test_ln2d_gelu_wide_refusals():
    lib = native.load()
    Hs, Ws = 4, 6
    x = torch.zeros(2 * Hs * Ws + 1, 4 * 256, device=DEV)
    gamma, beta = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    cases = [("C = 64", native.MI355X_F32, 64, 2 * Hs * Ws, Hs, Ws, ESHAPE), ("C = 192", native.MI355X_F32, 192, 2 * Hs * Ws, Hs, Ws, ESHAPE),
             ("no scatter grid", native.MI355X_F32, 128, 2 * Hs * Ws, 0, 0, ESHAPE), ("M not a multiple of Hs Ws", native.MI355X_F32, 256, 2 * Hs * Ws + 1, Hs, Ws, ESHAPE),
             ("unknown dtype", 7, 256, 2 * Hs * Ws, Hs, Ws, EDTYPE)]
    for what, dt, C_, M, hs, ws, want in cases:
        out = torch.full((4 * 3 * Hs * Ws, 256), NAN, device=DEV)
        st = _status(lib.mi355x_ln2d_gelu_wide, dt, x.data_ptr(), x.stride(0), M, C_, gamma.data_ptr(), beta.data_ptr(), EPS, out.data_ptr(), out.stride(0), hs, ws)
        assert st == want, what
        _untouched(out, what)
