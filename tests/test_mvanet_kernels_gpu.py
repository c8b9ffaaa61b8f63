"""The entry points of include/mi355x_refiners_mvanet.h (csrc/mvanet.hip) against the torch expressions they replace, and
mi355x_attention_general at the decoder's head shape, float32 and bfloat16, at the smallest shapes that reach each branch.

Inputs are rounded to the tested dtype first and the reference is computed in float64 from the rounded values through the MIRROR's own
modules (MultiPool, PatchMerge, PatchSplit, F.interpolate, prelu).  Bounds, as for the streaming kernels of tests/test_tiled_vae_kernels_gpu.py:
float32 arithmetic with a handful of roundings, so |err| <= K eps32 m with m the largest magnitude that enters an output and K = 16 (K = 256
for the gate: a 128-term dot product and the hardware exponential); bfloat16 adds the output's one rounding, |err| <= |ref| 2^-8 on top (half a bfloat16 ulp is at most that).
The attention is held to tests/kernel_cases._tol like the D = 160 cases of tests/test_kernels_gpu.py."""
import math

import pytest
import torch
import torch.nn.functional as F

from refiners_amd import mvanet as MV
from refiners_amd import native
from tests.kernel_cases import _tol, _vt_from_v

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
OK, EDTYPE, ESHAPE, EARG = 0, -1, -2, -4
EPS32 = 2.0**-23
E = 128


def _randn(*shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g).to(dtype)


def _close(got, ref, dtype, what, K=16):
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all(), what
    bound = K * EPS32 * float(ref.abs().max() + 1) + (ref.abs() * 2.0**-8 if dtype == torch.bfloat16 else 0)
    err = (got - ref).abs()
    print(f"{what}: max |err| = {float(err.max()):.3e}, max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (what, float((err / bound).max()))


def _maps(tokens, views, S):
    """[views S S, E] token rows -> (1, views, E, S, S) float64, the reference's layout."""
    return tokens.double().view(1, views, S, S, -1).permute(0, 1, 4, 2, 3)


def _rows(maps):
    """(B, E, H, W) -> [B H W, E]"""
    return maps.permute(0, 2, 3, 1).reshape(-1, maps.shape[1])


# ------------------------------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,ratios", [(8, [2, 8, 16]), (16, [2, 8, 16]), (8, [1, 2, 4]), (16, [1])])
def test_pool_of_the_merged_local_views(S, ratios, dtype):
    x = _randn(4 * S * S, E + 8, dtype=dtype, seed=S)[:, :E]  # rows wider than E: a leading dimension of its own
    want = MV.MultiPool(ratios)(MV.PatchMerge()(_maps(x, 4, S)))[0, :, 0]  # (rows, E)
    n = want.shape[0]
    rows = (n + 63) // 64 * 64
    out = torch.full((rows + 1, E), NAN, device=DEV, dtype=dtype)
    native.mvanet_pool(x, S, ratios, out[:rows], split=False)
    torch.cuda.synchronize()
    assert n == native.mvanet_pool_rows(2 * S, ratios)
    _close(out[:n], want, dtype, f"pool merge S {S} {ratios} {dtype}")
    assert bool((out[n:rows] == 0).all()) and torch.isnan(out[rows:].float()).all(), "padding rows are zeros, nothing past them is written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,ratios", [(8, [1, 2, 4]), (16, [1, 2, 4]), (16, [1])])
def test_pool_of_the_global_views_quadrants(S, ratios, dtype):
    x = _randn(S * S, E, dtype=dtype, seed=10 + S)
    want = MV.MultiPool(ratios)(MV.PatchSplit()(_maps(x, 1, S)[:, 0])[0])[:, :, 0]  # (4, rows, E)
    n = want.shape[1]
    rows = (n + 63) // 64 * 64
    out = torch.full((4, rows + 2, E), NAN, device=DEV, dtype=dtype)  # group stride > rows * ldo
    native.mvanet_pool(x, S, ratios, out[:, :rows], split=True)
    torch.cuda.synchronize()
    _close(out[:, :n], want, dtype, f"pool split S {S} {ratios} {dtype}")
    assert bool((out[:, n:rows] == 0).all()) and torch.isnan(out[:, rows:].float()).all()
    vt = torch.full((E, 4 * rows), NAN, device=DEV, dtype=dtype)  # V^T = W keys^T over the padded rows: every column the attention reads is finite
    w = _randn(E, E, dtype=dtype, seed=3)
    for v in range(4):
        native.gemm([(w, out[v, :rows])], vt[:, v * rows : (v + 1) * rows], weight_operand="x")
    torch.cuda.synchronize()
    assert torch.isfinite(vt.float()).all() and bool((vt.view(E, 4, rows)[:, :, n:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------ gate
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("in_place", [False, True])
def test_gate(dtype, in_place):
    S = 8
    x = _randn(5 * S * S, E, dtype=dtype, seed=21)
    w, b = (_randn(E, dtype=dtype, seed=22).float() * 0.3).to(dtype), _randn(1, dtype=dtype, seed=23)
    m = _maps(x, 5, S)
    gate = torch.sigmoid(F.conv2d(m[:, 4], w.double().view(1, E, 1, 1), b.double()))
    want = m[:, :4] * MV.PatchSplit()(F.interpolate(gate, size=(2 * S, 2 * S), mode="nearest"))
    local = x[: 4 * S * S].clone()
    out = local if in_place else torch.full_like(local, NAN)
    native.mvanet_gate(local, x[4 * S * S :], w, b, out, S)
    torch.cuda.synchronize()
    _close(out, _rows(want[0]), dtype, f"gate {dtype} in_place {in_place}", K=256)
    if not in_place:
        assert torch.equal(local, x[: 4 * S * S])


# ------------------------------------------------------------------------------------------------------------------------ resize + add
def _prelu(t, slope):
    return t if slope is None else F.prelu(t, slope.double().view(1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,hin,hout", [("bilinear", 16, 32), ("bilinear", 32, 8), ("nearest", 16, 8), ("nearest", 8, 16), ("bilinear", 8, 8)])
@pytest.mark.parametrize("fx,fy", [(False, False), (True, False), (False, True), (True, True)])
def test_resize_add(mode, hin, hout, fx, fy, dtype):
    B = 2
    x, y = _randn(B * hin * hin, E, dtype=dtype, seed=31), _randn(B * hout * hout, E, dtype=dtype, seed=32)
    sx = torch.tensor([0.25], device=DEV, dtype=dtype) if fx else None
    sy = torch.tensor([-0.5], device=DEV, dtype=dtype) if fy else None
    xm = _prelu(x.double().view(B, hin, hin, E).permute(0, 3, 1, 2), sx)
    want = F.interpolate(xm, size=(hout, hout), mode=mode) + _prelu(y.double().view(B, hout, hout, E).permute(0, 3, 1, 2), sy)
    out = torch.full_like(y, NAN)
    native.mvanet_resize_add(x, (hin, hin), y, out, (hout, hout), B=B, mode=mode, slope_x=sx, slope_y=sy)
    torch.cuda.synchronize()
    _close(out, _rows(want), dtype, f"{mode} {hin} -> {hout} prelu {fx} {fy} {dtype}")
    y2 = y.clone()
    native.mvanet_resize_add(x, (hin, hin), y2, y2, (hout, hout), B=B, mode=mode, slope_x=sx, slope_y=sy)  # in place on y
    torch.cuda.synchronize()
    assert torch.equal(y2, out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_add_with_merged_operands(dtype):
    S = 8
    x = _randn(5 * S * S, E, dtype=dtype, seed=41)
    slope = torch.tensor([0.2], device=DEV, dtype=dtype)
    m = _maps(x, 5, S)
    n = S * S
    # MCRM: global + nearest_down(PatchMerge(local))
    want = m[:, 4] + F.interpolate(MV.PatchMerge()(m[:, :4]), size=(S, S), mode="nearest")
    out = torch.full((n, E), NAN, device=DEV, dtype=dtype)
    native.mvanet_resize_add(x[: 4 * n], (2 * S, 2 * S), x[4 * n :], out, (S, S), mode="nearest", x_merge=True)
    torch.cuda.synchronize()
    _close(out, _rows(want), dtype, f"merged x, nearest down {dtype}")
    # RearrangeMultiView: PatchMerge(prelu(local)) + bilinear(prelu(global))
    want = MV.PatchMerge()(_prelu(m[:, :4], slope)) + F.interpolate(_prelu(m[:, 4], slope), size=(2 * S, 2 * S), mode="bilinear")
    out = torch.full((4 * n, E), NAN, device=DEV, dtype=dtype)
    native.mvanet_resize_add(x[4 * n :], (S, S), x[: 4 * n], out, (2 * S, 2 * S), mode="bilinear", slope_x=slope, slope_y=slope, y_merge=True)
    torch.cuda.synchronize()
    _close(out, _rows(want), dtype, f"merged y, bilinear up {dtype}")


# ------------------------------------------------------------------------------------------------------------------------ PReLU, views
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slope", [0.25, -0.75])
def test_prelu_in_place_reads_the_slope_at_every_launch(slope, dtype):
    x = _randn(3 * 41, E, dtype=dtype, seed=51)
    s = torch.tensor([slope], device=DEV, dtype=dtype)
    got = native.mvanet_prelu(x.clone(), s)
    torch.cuda.synchronize()
    _close(got, F.prelu(x.double(), s.double()), dtype, f"prelu {slope} {dtype}")
    s.fill_(2.0)
    got = native.mvanet_prelu(x.clone(), s)
    torch.cuda.synchronize()
    _close(got, F.prelu(x.double(), s.double()), dtype, f"prelu edited slope {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_views(dtype):
    img = _randn(1, 3, 24, 40, dtype=dtype, seed=61)
    want = MV.SplitMultiView()(img.double())[0]
    out = torch.full((5, 3, 12, 20), NAN, device=DEV, dtype=dtype)
    native.mvanet_split_views(img, out)
    torch.cuda.synchronize()
    assert torch.equal(out[:4], want[:4].to(dtype))
    _close(out[4], want[4], dtype, f"half-size view {dtype}")


# ------------------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lq", [64, 256, 1024])
@pytest.mark.parametrize("Lk", [21, 84, 276, 336])
def test_attention_general_one_head_of_128(Lq, Lk, dtype):
    B = 2
    q, k, v = (_randn(B, n, E, dtype=dtype, seed=70 + i) for i, n in enumerate((Lq, Lk, Lk)))
    v = (v.float() + 0.5).to(dtype)  # V with a mean: a row of probabilities that does not sum to one shows
    ref = torch.softmax(q.double() @ k.double().transpose(1, 2) / math.sqrt(E), dim=-1) @ v.double()
    out = torch.full((B, Lq, E), NAN, device=DEV, dtype=dtype)
    native.attention_general(q, k, _vt_from_v(v, (Lk + 63) // 64 * 64), out, 1, Lk)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"attention Lq {Lq} Lk {Lk} {dtype}: max-abs error / max|ref| = {err:.3e}")
    assert err <= _tol(dtype), err


# ------------------------------------------------------------------------------------------------------------------------ refusals
def _recorded(call):
    ops = []
    with native.recording(ops):
        call()
    fn, args, _what, _keep = ops[0]
    return fn, args


def _refuse(call, changes, out, fill=NAN):
    """Every changed argument set returns its status; after all of them `out` still holds `fill`; the untouched arguments then run."""
    same = lambda: bool(torch.isnan(out.float()).all() if math.isnan(fill) else (out.float() == fill).all())  # noqa: E731
    for what, change, status in changes:
        fn, args = _recorded(call)
        if callable(change):
            args = change(args)
        else:
            for k, v in change.items():
                setattr(args[0]._obj, k, v)
        assert fn(*args, native.stream_ptr()) == status, what
    torch.cuda.synchronize()
    assert same(), "a refused call wrote"
    fn, args = _recorded(call)
    assert fn(*args, native.stream_ptr()) == OK
    torch.cuda.synchronize()
    assert not same()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_write_nothing(dtype):
    S = 8
    n = S * S
    x = _randn(5 * n, E, dtype=dtype, seed=81)
    out = torch.full((4, 64, E), NAN, device=DEV, dtype=dtype)
    _refuse(lambda: native.mvanet_pool(x[4 * n :], S, [1, 2, 4], out, split=True), [
        ("dtype", dict(dtype=7), EDTYPE), ("mode", dict(mode=2), EARG), ("src NULL", dict(src=None), EARG), ("E 0", dict(E=0), EARG), ("odd S", dict(S=7), ESHAPE),
        ("no ratios", dict(n_ratios=0), ESHAPE), ("four ratios", dict(n_ratios=4), ESHAPE), ("rows short", dict(rows=20), ESHAPE), ("lds < E", dict(lds=E - 8), ESHAPE),
        ("ldo unaligned", dict(ldo=E + 1), ESHAPE), ("group stride short", dict(group_stride=63 * E), ESHAPE), ("out over src", dict(out=x[4 * n :].data_ptr()), EARG),
    ], out)
    fn, args = _recorded(lambda: native.mvanet_pool(x[4 * n :], S, [1, 2, 4], out, split=True))
    args[0]._obj.ratio[1] = 3  # does not divide the quadrant's side
    assert fn(*args, native.stream_ptr()) == ESHAPE
    w, b = _randn(E, dtype=dtype, seed=82), _randn(1, dtype=dtype, seed=83)
    out = torch.full((4 * n, E), NAN, device=DEV, dtype=dtype)
    _refuse(lambda: native.mvanet_gate(x[: 4 * n], x[4 * n :], w, b, out, S), [
        ("dtype", dict(dtype=7), EDTYPE), ("w NULL", dict(w=None), EARG), ("b NULL", dict(b=None), EARG), ("S 0", dict(S=0), ESHAPE), ("ldg < E", dict(ldg=E - 8), ESHAPE),
        ("ldo unaligned", dict(ldo=E + 1), ESHAPE), ("out over glb", dict(out=x[4 * n :].data_ptr()), EARG), ("out inside local", dict(out=x[n:].data_ptr()), EARG),
    ], out)
    out = torch.full((n, E), NAN, device=DEV, dtype=dtype)
    _refuse(lambda: native.mvanet_resize_add(x[: 4 * n], (2 * S, 2 * S), x[4 * n :], out, (S, S), mode="nearest", x_merge=True), [
        ("dtype", dict(dtype=7), EDTYPE), ("mode", dict(mode=2), EARG), ("a NULL", dict(a=None), EARG), ("merged batch", dict(B=2), ESHAPE), ("merged odd side", dict(Ha=15), ESHAPE),
        ("Wo 0", dict(Wo=0), ESHAPE), ("lda < E", dict(lda=E - 8), ESHAPE), ("ldb unaligned", dict(ldb=E + 1), ESHAPE), ("out over a", dict(out=x.data_ptr()), EARG),
        ("out inside b", dict(out=x[4 * n + 8 :].data_ptr(), Ho=4, Wo=4, Ha=8, Wa=8), EARG),
    ], out)
    s = torch.tensor([0.25], device=DEV, dtype=dtype)
    out = torch.full((n, E), -1.0, device=DEV, dtype=dtype)
    es = out.element_size()
    _refuse(lambda: native.mvanet_prelu(out, s), [
        ("dtype", lambda a: (7,) + a[1:], EDTYPE), ("x NULL", lambda a: (a[0], None) + a[2:], EARG), ("slope NULL", lambda a: a[:2] + (None,) + a[3:], EARG),
        ("n 0", lambda a: a[:3] + (0,), EARG), ("n off the vector", lambda a: a[:3] + (n * E - 1,), ESHAPE), ("x misaligned", lambda a: (a[0], a[1] + es) + a[2:], ESHAPE),
    ], out, fill=-1.0)
    img = _randn(1, 3, 16, 16, dtype=dtype, seed=84)
    out = torch.full((5, 3, 8, 8), NAN, device=DEV, dtype=dtype)
    _refuse(lambda: native.mvanet_split_views(img, out), [
        ("dtype", lambda a: (7,) + a[1:], EDTYPE), ("img NULL", lambda a: (a[0], None) + a[2:], EARG), ("odd H", lambda a: a[:4] + (15, 16), ESHAPE),
        ("C 0", lambda a: a[:3] + (0,) + a[4:], ESHAPE), ("out over img", lambda a: (a[0], a[1], a[1]) + a[3:], EARG),
    ], out)
