"""mi355x_window_attention (csrc/window_attention.hip) against float64 torch on the GPU: softmax(scale Q K^T + table[rel] + shift mask) V per
(window, head), float32 and bfloat16, with the operands laid out as the engine passes them -- q / k / v as column views of ONE packed buffer
with a wider leading dimension, NaN wherever the kernel has no business reading or writing.

Inputs are rounded to the tested dtype first and the reference is computed from the rounded values.  The bound is the one the attention
kernels of this project are held to (tests/kernel_cases._tol): max-abs error <= 1e-3 max|ref| for float32, 1.6e-2 max|ref| for bfloat16."""
import pytest
import torch

from refiners_amd import native
from refiners_amd.swin import canonical_relative_position_index, shift_mask
from tests.kernel_cases import _tol

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
OK, EDTYPE, ESHAPE, EARG = 0, -1, -2, -4
D = 32

#: (ws, windows per side, batch, heads, shifted)
SHAPES = [
    (12, 2, 1, 4, True),   # with the shift all four mask classes appear (interior, last row, last column, corner)
    (12, 2, 1, 4, False),
    (12, 3, 2, 8, True),   # interior windows, two images, two (bf16) / four (f32) head groups
    (7, 2, 1, 2, True),    # N = 49: ragged 16-token blocks
    (12, 2, 1, 1, True),   # a single head: idle waves in the workgroup
    (7, 2, 1, 1, False),
]


def _inputs(ws, nw, B, H, dtype, seed, q_gain=1.0, slot=None):
    """-> (buf, out, table, views) : buf [nW, slot, 3 H D + 32] and out [nW, slot, H D + 16] NaN-filled, rows < N of buf's first 3 H D columns drawn."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    N, nW = ws * ws, B * nw * nw
    slot = slot or N
    C = H * D
    buf = torch.full((nW, slot, 3 * C + 32), NAN, device=DEV, dtype=dtype)
    qkv = torch.randn(nW, N, 3, H, D, device=DEV, generator=g)
    qkv[:, :, 0] *= q_gain
    qkv[:, :, 2] += 0.5  # V with a mean: a row of probabilities that does not sum to one shows
    buf[:, :N, : 3 * C] = qkv.reshape(nW, N, 3 * C).to(dtype)
    out = torch.full((nW, slot, C + 16), NAN, device=DEV, dtype=dtype)
    table = 0.5 * torch.randn((2 * ws - 1) ** 2, H, device=DEV, generator=g)
    return buf, out, table


def _views(buf, out, ws, H):
    N, C = ws * ws, H * D
    return buf[:, :N, :C], buf[:, :N, C : 2 * C], buf[:, :N, 2 * C : 3 * C], out[:, :N, :C]


def _ref(buf, table, ws, nw, H, shift, mask_value=-100.0):
    N, C = ws * ws, H * D
    nW = buf.shape[0]
    q, k, v = (t.double() for t in buf[:, :N, : 3 * C].reshape(nW, N, 3, H, D).unbind(2))
    bias = table.double()[canonical_relative_position_index(ws).to(DEV)].permute(2, 0, 1)  # [H, N, N]
    s = torch.einsum("wnhd,wmhd->whnm", q, k) * D**-0.5 + bias[None]
    if shift:
        m = shift_mask(nw * ws, ws).to(DEV).double()  # [nw^2, N, N], -100 / 0
        m = torch.where(m != 0, mask_value, 0.0).repeat(nW // (nw * nw), 1, 1)
        s = s + m[:, None]
    return torch.einsum("whnm,wmhd->wnhd", s.softmax(-1), v).reshape(nW, N, C)


def _run(buf, out, table, ws, nw, H, shift):
    q, k, v, o = _views(buf, out, ws, H)
    native.window_attention(q, k, v, table, o, H, ws, nw=nw, shift=shift)
    torch.cuda.synchronize()


def _check(buf, out, table, ws, nw, H, shift, dtype, what):
    N, C = ws * ws, H * D
    pristine = buf.clone()
    _run(buf, out, table, ws, nw, H, shift)
    ref = _ref(buf, table, ws, nw, H, shift)
    got = out[:, :N, :C].double()
    assert torch.isfinite(got).all(), what
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"{what}: max-abs error / max|ref| = {err:.3e}")
    assert err <= _tol(dtype), (what, err)
    assert torch.isnan(out[:, :, C:].float()).all() and torch.isnan(out[:, N:].float()).all(), f"{what}: wrote outside rows < N / its columns"
    assert torch.equal(buf.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), pristine.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), f"{what}: inputs changed"
    first = out.clone()
    out[:, :N, :C] = 0
    _run(buf, out, table, ws, nw, H, shift)
    assert torch.equal(out[:, :N, :C], first[:, :N, :C]), f"{what}: the second call differs from the first"
    return ref, got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws,nw,B,H,shifted", SHAPES)
def test_window_attention_matches_float64(ws, nw, B, H, shifted, dtype):
    shift = ws // 2 if shifted else 0
    slot = 64 if ws == 7 else None  # ragged windows in 64-row slots: rows >= N are NaN and must stay so
    buf, out, table = _inputs(ws, nw, B, H, dtype, seed=ws * 100 + nw * 10 + H, slot=slot)
    _check(buf, out, table, ws, nw, H, shift, dtype, f"ws {ws} {nw}x{nw} B {B} H {H} shift {shift} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_spiked_keys(dtype):
    """Two key rows scaled x6: their scores tower over the row, the true-maximum softmax must not lose the rest."""
    ws, nw, H = 12, 2, 4
    buf, out, table = _inputs(ws, nw, 1, H, dtype, seed=5)
    C = H * D
    for row in (3, 77):
        buf[:, row, C : 2 * C] *= 6
    _check(buf, out, table, ws, nw, H, ws // 2, dtype, f"spike {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_is_additive(dtype):
    """Scores of +-60: each token's query points away from its own region's direction and towards every other region's, so the pairs the
    shift mask hits score +60 and all others -60.  With -100 ADDED the masked pairs still lead by 20 and carry nearly all the weight;
    a -inf mask gives a different answer -- the reference with -inf in place of -100 must miss the bound by far, and the kernel must not."""
    ws, nw, H = 12, 2, 4
    N, C = ws * ws, H * D
    shift = ws // 2
    buf, out, table = _inputs(ws, nw, 1, H, dtype, seed=9)
    from refiners_amd.swin import partition_windows, region_ids

    reg = partition_windows(region_ids(nw * ws, ws).view(1, nw * ws, nw * ws, 1), ws).reshape(nw * nw, N).to(DEV)  # region id (0..8) per token
    onehot = torch.nn.functional.one_hot(reg, D).float()  # [nW, N, D]: direction e_region
    c = (60.0 * D**0.5) ** 0.5  # scale c^2 = 60
    present = torch.zeros(D, device=DEV)
    present[:9] = 1
    qdir = (present[None, None] - 2 * onehot) * c  # -c on the token's own region, +c on the other eight
    kdir = onehot * c
    noise = 0.05
    qkv = buf[:, :N, : 3 * C].float().reshape(nw * nw, N, 3, H, D)
    qkv[:, :, 0] = qkv[:, :, 0] * noise + qdir[:, :, None]
    qkv[:, :, 1] = qkv[:, :, 1] * noise + kdir[:, :, None]
    buf[:, :N, : 3 * C] = qkv.reshape(nw * nw, N, 3 * C).to(dtype)
    ref, got = _check(buf, out, table, ws, nw, H, shift, dtype, f"additive mask {dtype}")
    wrong = _ref(buf, table, ws, nw, H, shift, mask_value=float("-inf"))
    miss = float((wrong - ref).abs().max() / ref.abs().max())
    assert miss > 10 * _tol(dtype), f"the case does not tell -100 from -inf ({miss:.3e})"
    assert float((got - wrong).abs().max() / ref.abs().max()) > 10 * _tol(dtype)


def _recorded(buf, out, table, ws, nw, H, shift):
    ops = []
    q, k, v, o = _views(buf, out, ws, H)
    with native.recording(ops):
        native.window_attention(q, k, v, table, o, H, ws, nw=nw, shift=shift)
    fn, args, _what, _keep = ops[0]
    return fn, args, args[0]._obj


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_write_nothing(dtype):
    ws, nw, H = 12, 2, 2
    es = 4 if dtype == torch.float32 else 2
    buf, out, table = _inputs(ws, nw, 1, H, dtype, seed=3)
    cases = [
        ("dtype", dict(dtype=7), EDTYPE),
        ("ws 13", dict(ws=13), ESHAPE),
        ("ws 0", dict(ws=0), ESHAPE),
        ("shift == ws", dict(shift=ws), ESHAPE),
        ("shift < 0", dict(shift=-1), ESHAPE),
        ("nW no multiple of nw^2", dict(nw=3), ESHAPE),
        ("ldq < H 32", dict(ldq=H * D - 16), ESHAPE),
        ("ldo < H 32", dict(ldo=H * D - 16), ESHAPE),
        ("ldk unaligned", dict(ldk=3 * H * D + 32 + 1), ESHAPE),
        ("q NULL", dict(q=None), EARG),
        ("table NULL", dict(table=None), EARG),
        ("out NULL", dict(out=None), EARG),
        ("nW 0", dict(nW=0), EARG),
        ("H 0", dict(H=0), EARG),
    ]
    for what, change, status in cases:
        fn, args, a = _recorded(buf, out, table, ws, nw, H, ws // 2)
        for k, v in change.items():
            setattr(a, k, v)
        assert fn(*args, native.stream_ptr()) == status, what
    fn, args, a = _recorded(buf, out, table, ws, nw, H, ws // 2)
    a.v = a.v + es  # off the 16-byte grid
    assert fn(*args, native.stream_ptr()) == ESHAPE
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()
    fn, args, a = _recorded(buf, out, table, ws, nw, H, ws // 2)
    assert fn(*args, native.stream_ptr()) == OK  # the untouched arguments run
    torch.cuda.synchronize()
    assert torch.isfinite(out[:, :, : H * D].float()).all()
