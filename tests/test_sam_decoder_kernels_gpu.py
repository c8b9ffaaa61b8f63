"""Edge-case parity of the SAM mask-decoder kernels (csrc/sam_decoder.hip) against float64 torch on the GPU.

Every test rounds its inputs to the tested dtype first and computes the reference in float64 from those rounded values.  The kernels
compute in float32 and store the dtype, so what separates them from the reference is float32 arithmetic (about 1e-6 of the output's
magnitude here) and, for bfloat16, the final rounding of a float32 result to 8 significant bits: at most 2^-9 of the element.  Each
output element must satisfy

    |out - ref| <= a |ref| + b max|ref|          float32: a = b = 1e-5;   bfloat16: a = 2^-8 (twice the final rounding), b = 2e-5.

The b term covers elements near zero, whose float32 error is relative to the row's terms, not to the element.  LayerNorm adds a
per-element term for its own conditioning (groups whose spread is tiny against their mean; see _ln_gelu_ref).  postprocess_masks is the
exception to "float64 reference": torch computes its tap positions in float32 (scale = in / out as float for float input), and a float64
resize would move the taps by up to 1e-4 px, so its reference is postprocess_masks(low.float()) on the GPU with the same bounds.

Outputs (and the pad columns of inputs) are filled with NaN before a call: every element the kernel owns must come back finite, every
element it does not own (pad columns, the gap between batch strides, the plane after the last one) must still be NaN.  That turns
"each output written by exactly one lane" and "nothing read or written out of bounds" into assertions."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from refiners_amd import native
from refiners_amd.segment_anything import compute_scaled_size, postprocess_masks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.bfloat16]
BOUND = {torch.float32: (1e-5, 1e-5), torch.bfloat16: (2.0**-8, 2e-5)}
NAN = float("nan")
OK, EDTYPE, ESHAPE, EARG = 0, -1, -2, -4


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _check(out, ref, dtype, what="", extra=0.0):
    """out (the kernel's, any dtype) against the float64 reference, element by element (extra: a per-element term of the operation's
    own conditioning, see _ln_gelu_ref)."""
    a, b = BOUND[dtype]
    out, ref = out.double(), ref.double()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{what}: {int((~torch.isfinite(out)).sum())} elements not written (or not finite)"
    err = (out - ref).abs()
    bound = a * ref.abs() + b * ref.abs().max() + extra
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; worst err {float(err.max()):.3e}, "
                           f"max|ref| {float(ref.abs().max()):.3e}, first at {tuple(int(i) for i in bad.nonzero()[0])}")


def _untouched(t, what=""):
    assert torch.isnan(t.float()).all(), f"{what}: {int((~torch.isnan(t.float())).sum())} elements written outside the operation"


# ------------------------------------------------------------------------------------------------ attention
SCALE = 0.5  # not the default D^-0.5 of either width; a power of two, so q * scale is exact and the structured logits below are exact


def _attn_inputs(Bq, Bk, Lq, Lk, H, D, seed):
    """q [Bq, Lq, H, D], k / v [Bk, Lk, H, D] float64 with structure that makes a lost key visible.  The last six dimensions of every
    head are markers (the others are random): k[:, :, D-1] = 1 for every key; k[:, j < 256, D-2] = -1 (the first key chunk);
    k[:, j_i, D-3-i] = 1 at the spike keys j_i = Lk-1, 256, 255, 0 (those < Lk).  Query qi is of kind qi % 8:
      0..3  spike: q = 40 on spike i's marker, +20 on that key's logit, so it holds almost all of the softmax mass (a dropped or
            duplicated key moves the output by O(1));
      4     large: q = 192 on the constant marker, every logit about +96 (exp without max subtraction overflows float32);
      5     chunk: q = 200 on the first-chunk marker, the first chunk's keys 100 below the rest (with more than one chunk its
            combine factor underflows to 0; with one chunk every logit is about -100);
      6     all-equal: q = 0, every logit 0 (the output is the mean of v);
      7     plain random."""
    g = _gen(seed)
    q = torch.randn(Bq, Lq, H, D, device=DEV, generator=g, dtype=torch.float64) * 0.5
    k = torch.randn(Bk, Lk, H, D, device=DEV, generator=g, dtype=torch.float64) * 0.5
    v = torch.randn(Bk, Lk, H, D, device=DEV, generator=g, dtype=torch.float64)
    q[..., D - 6 :] = 0
    k[..., D - 6 :] = 0
    k[..., D - 1] = 1.0
    k[:, :256, :, D - 2] = -1.0
    spikes = list(dict.fromkeys(j for j in (Lk - 1, 256, 255, 0) if j < Lk))
    for i, j in enumerate(spikes):
        k[:, j, :, D - 3 - i] = 1.0
    kind = torch.arange(Lq, device=DEV) % 8
    for t in range(4):
        q[:, kind == t, :, D - 3 - t % len(spikes)] = 40.0
    q[:, kind == 4, :, D - 1] = 192.0
    q[:, kind == 5, :, D - 2] = 200.0
    q[:, kind == 6] = 0.0
    return q, k, v


def _attn_ref(q, k, v, B):
    """float64 softmax(q k^T * SCALE) v, [B, Lq, H, D]."""
    q, k, v = (t.expand(B, -1, -1, -1) for t in (q, k, v))
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * SCALE, dim=-1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v)


# (D, Lq, Lk, B, H, shared): every Lk of both regimes, every Lq, B in {1, 3}, H in {1, 8}, batch stride 0 on q and on k / v
SHORT_KEYS = [(16, 1, 1, 1, 1, ""), (32, 255, 2, 3, 8, "q"), (16, 256, 63, 3, 8, "kv"), (32, 257, 64, 1, 8, ""), (16, 4096, 64, 3, 8, "kv"),
              (32, 4096, 63, 1, 1, ""), (16, 257, 2, 1, 8, ""), (32, 1, 64, 3, 1, "q")]
SPLIT = [(16, 1, 4097, 1, 8, ""), (32, 3, 65, 3, 8, "kv"), (16, 4, 255, 3, 1, ""), (32, 5, 256, 3, 8, "q"), (16, 63, 257, 3, 8, "kv"),
         (32, 64, 512, 3, 8, "kv"), (16, 64, 513, 1, 1, ""), (32, 64, 4097, 3, 8, "kv"), (32, 1, 257, 1, 1, ""), (16, 5, 4097, 3, 8, "q"),
         (32, 4, 4097, 1, 8, "")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,Lq,Lk,B,H,shared", SHORT_KEYS + SPLIT)
def test_sam_attention_edges(dtype, D, Lq, Lk, B, H, shared):
    """Both regimes of mi355x_sam_attention (Lk <= 64: sam_attn_short_keys; else sam_attn_split_partial + _combine, 256-key chunks)
    at their boundaries.  k and v are column views of one [Lk, 2 H D + 16] tensor as the engine passes them; q and out have a leading
    dimension wider than H D, and out a batch stride two rows longer than Lq * ldo."""
    HD = H * D
    Bq, Bk = (1 if "q" in shared else B), (1 if "kv" in shared else B)
    q, k, v = _attn_inputs(Bq, Bk, Lq, Lk, H, D, seed=Lq * 7919 + Lk + D)
    q, k, v = (t.to(dtype) for t in (q, k, v))
    qbuf = torch.full((Bq, Lq, HD + 24), NAN, device=DEV, dtype=dtype)
    qbuf[..., :HD] = q.reshape(Bq, Lq, HD)
    kv = torch.full((Bk, Lk, 2 * HD + 16), NAN, device=DEV, dtype=dtype)
    kv[..., :HD], kv[..., HD : 2 * HD] = k.reshape(Bk, Lk, HD), v.reshape(Bk, Lk, HD)
    obuf = torch.full((B, Lq + 2, HD + 8), NAN, device=DEV, dtype=dtype)
    out = obuf[:, :Lq, :HD]
    need = native.sam_attention_ws_floats(B, H, D, Lq, Lk)
    assert need == (0 if Lk <= 64 else B * H * -(-Lk // 256) * Lq * (D + 2))
    ws = torch.full((need,), NAN, device=DEV) if need else None
    args = (qbuf[..., :HD], kv[..., :HD], kv[..., HD : 2 * HD], out, H)
    native.sam_attention(*args, ws=ws, scale=SCALE)
    ref = _attn_ref(q.double(), k.double(), v.double(), B).reshape(B, Lq, HD)
    _check(out, ref, dtype, f"{dtype} D={D} Lq={Lq} Lk={Lk}")
    _untouched(obuf[:, :Lq, HD:], "pad columns")
    _untouched(obuf[:, Lq:], "gap between batch strides")
    first = out.clone()
    native.sam_attention(*args, ws=ws, scale=SCALE)
    assert torch.equal(out, first), "two calls differ"
    if need:  # the workspace is never read before it is written: a zero-filled one gives the same bits
        ws.zero_()
        native.sam_attention(*args, ws=ws, scale=SCALE)
        assert torch.equal(out, first), "NaN- and zero-filled workspaces differ"


# ------------------------------------------------------------------------------------------------ LayerNorm2d + GELU
def _ln_gelu_rows(M, width, dtype, g):
    """[M, width] float64 rows, exactly representable in dtype, with the rows LayerNorm gets wrong first: row 0 constant (variance 0:
    eps alone), row 1 of variance ~1e-8 (eps dominates; SAM's eps is 1e-6), rows 2..4 of mean 1024 and small spread (a one-pass
    E[x^2] - E[x]^2 cancels; the values are multiples of 2^-7 (float32) or 8 (bfloat16), so even float32 sums of 64 of them are
    exact and the mean is exact), then random rows with random offsets."""
    x = torch.randn(M, width, device=DEV, generator=g, dtype=torch.float64) * 2 + torch.randn(M, 1, device=DEV, generator=g, dtype=torch.float64)
    x[0] = 0.37
    x[1] = torch.randn(width, device=DEV, generator=g, dtype=torch.float64) * 1e-4
    step, spread = (2.0**-7, 1.0) if dtype == torch.float32 else (8.0, 8.0)
    x[2:5] = 1024 + step * torch.round(torch.randn(3, width, device=DEV, generator=g, dtype=torch.float64) * spread / step)
    return x.to(dtype).double()


def _ln_gelu_ref(x, gamma, beta, eps):
    """float64 LayerNorm over the last dimension (biased variance) + exact-erf GELU, and the conditioning term of its bound.

    LayerNorm is ill-conditioned where the spread is small against the mean: any float32 mean of C values carries an error up to
    log2(C) 2^-24 mean|x| (the C lanes add in log2(C) rounded steps), every normalised value moves by that over sqrt(var + eps), and
    GELU' <= 1.13 passes it on.  Where var is near eps that is far above 1e-5 of the output (a group of two close values of magnitude 2
    gives 4.5e-5), so the bound adds 2 (log2(C) + 1) 2^-24 |gamma| mean|x| / sqrt(var + eps) per element.  A one-pass variance or a lost
    lane still fails it: on the mean-1024 rows it is ~5e-4 |gamma|, against errors of several percent."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    y = F.gelu((x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double())
    C = x.shape[-1]
    cond = 2 * C.bit_length() * 2.0**-24 * gamma.double().abs() * x.abs().mean(-1, keepdim=True) / torch.sqrt(var + eps)
    return y, cond


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,G", [(1, 4), (2, 2), (4, 4), (8, 8), (16, 1), (32, 2), (64, 1), (64, 4)])
def test_ln_gelu_groups(dtype, C, G):
    """Hs = 0: G groups of C channels per row, in place of the input layout (the MaskEncoder uses (4, 4) and (16, 1)).  M = 1023 leaves
    a partial last block whenever G C < 256; ldx and ldo are wider than G C, and the pad columns must stay NaN."""
    g = _gen(100 + C * 8 + G)
    M, eps = 1023, 1e-6
    x = _ln_gelu_rows(M, G * C, dtype, g)
    gamma, beta = (torch.randn(C, device=DEV, generator=g) for _ in range(2))
    xbuf = torch.full((M, G * C + 3), NAN, device=DEV, dtype=dtype)
    xbuf[:, : G * C] = x.to(dtype)
    obuf = torch.full((M, G * C + 5), NAN, device=DEV, dtype=dtype)
    native.convt2x2_ln_gelu(xbuf[:, : G * C], C, G, gamma, beta, eps, obuf[:, : G * C])
    ref, cond = _ln_gelu_ref(x.view(M, G, C), gamma, beta, eps)
    _check(obuf[:, : G * C], ref.view(M, G * C), dtype, f"C={C} G={G}", extra=cond.view(M, G * C))
    _untouched(obuf[:, G * C :], "pad columns")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_gelu_scatter_production_geometry(dtype):
    """Hs = Ws = 64, P = 3, C = 64, G = 4 (the DenseEmbeddingUpscaling of three prompts): 3.1 M lanes, more than the 8192 x 256 grid, so
    the grid-stride loop runs.  Group (dy, dx) of pixel (p, y, x) goes to row (p, 2y + dy, 2x + dx) of the NHWC output."""
    g = _gen(7)
    P, Hs, Ws, C, eps = 3, 64, 64, 64, 1e-6
    M = P * Hs * Ws
    x = _ln_gelu_rows(M, 4 * C, dtype, g)
    gamma, beta = (torch.randn(C, device=DEV, generator=g) for _ in range(2))
    xbuf = torch.full((M, 4 * C + 8), NAN, device=DEV, dtype=dtype)
    xbuf[:, : 4 * C] = x.to(dtype)
    obuf = torch.full((4 * M, C + 8), NAN, device=DEV, dtype=dtype)
    native.convt2x2_ln_gelu(xbuf[:, : 4 * C], C, 4, gamma, beta, eps, obuf[:, :C], scatter_hw=(Hs, Ws))
    y, cond = _ln_gelu_ref(x.view(M, 4, C), gamma, beta, eps)  # [(p, y, x), (dy, dx), c]
    scatter = lambda t: t.view(P, Hs, Ws, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(4 * M, C)  # noqa: E731
    _check(obuf[:, :C], scatter(y), dtype, "scatter", extra=scatter(cond))
    _untouched(obuf[:, C:], "pad columns")


# ------------------------------------------------------------------------------------------------ mask head
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nk,P,Hin,Win", [(1, 3, 7, 9), (2, 5, 13, 11), (3, 2, 1, 70), (4, 2, 128, 128), (2, 1100, 1, 70), (3, 64, 128, 128)])
def test_sam_mask_head_edges(dtype, nk, P, Hin, Win):
    """7 x 9 (one partial tile), 13 x 11 (a partial last tile), 1 x 70 (one row; 64 + 6 pixels), 128 x 128 (the product size).  P = 1100
    at 1 x 70 (2200 tiles) and P = 64 at 128 x 128 (16384 tiles) exceed the 2048-workgroup grid, so workgroups cross from one prompt to
    another and reload the hypernetwork vectors.  hyper is a strided slice of [P, 5, 48], x has ldx = 72, out has an extra plane per prompt."""
    g = _gen(200 + nk * 31 + P + Hin)
    HW = Hin * Win
    x = torch.randn(P, Hin, Win, 64, device=DEV, generator=g, dtype=torch.float64).to(dtype)
    weight = torch.randn(64, 32, 2, 2, device=DEV, generator=g) / 8
    bias = torch.randn(32, device=DEV, generator=g)
    hyper = torch.randn(P, nk, 32, device=DEV, generator=g, dtype=torch.float64).to(dtype)
    xbuf = torch.full((P * HW, 72), NAN, device=DEV, dtype=dtype)
    xbuf[:, :64] = x.reshape(P * HW, 64)
    hbuf = torch.full((P, 5, 48), NAN, device=DEV, dtype=dtype)
    hbuf[:, 1 : 1 + nk, 8:40] = hyper
    obuf = torch.full((P, nk + 1, 2 * Hin, 2 * Win), NAN, device=DEV, dtype=dtype)
    w = weight.permute(0, 2, 3, 1).reshape(64, 128).contiguous()
    native.sam_mask_head(xbuf[:, :64], P, Hin, Win, w, bias, hbuf[:, 1 : 1 + nk, 8:40], obuf[:, :nk])
    up = F.gelu(F.conv_transpose2d(x.double().permute(0, 3, 1, 2), weight.double(), bias.double(), stride=2))
    ref = torch.einsum("pkc,pchw->pkhw", hyper.double(), up)
    del up
    _check(obuf[:, :nk], ref, dtype, f"nk={nk} P={P} {Hin}x{Win}")
    _untouched(obuf[:, nk:], "the plane after the last mask")


# ------------------------------------------------------------------------------------------------ postprocess_masks
# (original size, low-res plane, R, planes): outputs smaller and larger than R (the outer resize down- and upsamples), crops with sh or
# sw = R and = 1, H or W = 1, a non-square low-res plane, and 64 x 3 planes (11.5 M outputs: the grid-stride loop runs)
POST = [((600, 900), (256, 256), 1024, (2, 3)), ((1024, 1024), (256, 256), 1024, (1, 3)), ((1500, 2000), (256, 256), 1024, (2, 3)),
        ((4000, 300), (256, 256), 1024, (1, 3)), ((1, 1024), (256, 256), 1024, (1, 3)), ((1024, 1), (256, 256), 1024, (1, 3)),
        ((300, 200), (64, 48), 256, (2, 1)), ((200, 300), (256, 256), 1024, (64, 3))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size,plane,R,lead", POST)
def test_sam_postprocess_masks_edges(dtype, size, plane, R, lead):
    g = _gen(300 + size[0] + size[1])
    low = torch.randn(*lead, *plane, device=DEV, generator=g).to(dtype)
    scaled = compute_scaled_size(size, R)
    N = low.numel() // (plane[0] * plane[1])
    obuf = torch.full((N + 1, *size), NAN, device=DEV, dtype=dtype)
    out = obuf[:N].view(*lead, *size)
    native.sam_postprocess_masks(low, R, scaled, out)
    ref = postprocess_masks(low.float(), size, R)
    _check(out, ref, dtype, f"{size} from {plane}, crop {scaled}")
    _untouched(obuf[N:], "the plane after the last one")
    for thr, odt in [(0.0, torch.uint8), (0.5, torch.bool), (-1.0, torch.uint8), (0.0, torch.bool), (0.5, torch.uint8), (-1.0, torch.bool)]:
        bbuf = torch.full((N + 1, *size), 171, device=DEV, dtype=torch.uint8)
        binary = bbuf[:N].view(*lead, *size)
        native.sam_postprocess_masks(low, R, scaled, binary.view(odt) if odt == torch.bool else binary, threshold=thr)
        assert bool(((binary == 0) | (binary == 1)).all()), (thr, odt, "values other than 0 / 1")
        assert bool((bbuf[N:] == 171).all()), (thr, odt, "written past the last plane")
        sure = (ref - thr).abs() > 1e-4 * ref.abs().max()
        assert torch.equal(binary.bool()[sure], (ref > thr)[sure]), (thr, odt)


# ------------------------------------------------------------------------------------------------ refusals of the C entry points
def _status(fn, *args):
    st = fn(*args, native.stream_ptr())
    torch.cuda.synchronize()
    return st


def _attn_args(dtype=native.MI355X_F32, B=2, H=2, D=16, Lq=8, Lk=8, ws_floats=None):
    """SamAttnArgs over real allocations big enough for what the call would launch if its refusal were lost: 64-wide heads, Lq and Lk
    as given, and a workspace of the size a split launch with D = 64 needs."""
    cols = H * 64
    keep = dict(q=torch.zeros(B, Lq, cols, device=DEV), kv=torch.zeros(B, Lk, 2 * cols, device=DEV),
                out=torch.full((B, Lq, cols), NAN, device=DEV), ws=torch.zeros(max(native.sam_attention_ws_floats(B, H, 64, Lq, Lk), 1), device=DEV))
    a = native.SamAttnArgs()
    a.dtype, a.B, a.H, a.D, a.Lq, a.Lk = dtype, B, H, D, Lq, Lk
    a.q, a.ldq, a.q_batch_stride = keep["q"].data_ptr(), cols, Lq * cols
    a.k, a.ldk, a.k_batch_stride = keep["kv"].data_ptr(), 2 * cols, Lk * 2 * cols
    a.v, a.ldv, a.v_batch_stride = keep["kv"].data_ptr() + 4 * cols, 2 * cols, Lk * 2 * cols
    a.out, a.ldo, a.o_batch_stride = keep["out"].data_ptr(), cols, Lq * cols
    a.scale = 0.25
    a.ws = keep["ws"].data_ptr()
    a.ws_floats = keep["ws"].numel() if ws_floats is None else ws_floats
    return a, keep


def test_sam_attention_refusals():
    lib = native.load()
    need = native.sam_attention_ws_floats(2, 2, 16, 8, 300)
    cases = [("D = 8", dict(D=8), ESHAPE), ("D = 64", dict(D=64), ESHAPE), ("D = 64, split", dict(D=64, Lk=300), ESHAPE),
             ("Lq and Lk > 64", dict(Lq=65, Lk=65), ESHAPE), ("ws one short", dict(Lk=300, ws_floats=need - 1), EARG),
             ("bad dtype", dict(dtype=7), EDTYPE), ("bad dtype, split", dict(dtype=7, Lk=300), EDTYPE)]
    for what, kw, want in cases:
        a, keep = _attn_args(**kw)
        assert _status(lib.mi355x_sam_attention, ctypes.byref(a)) == want, what
        _untouched(keep["out"], what)
    a, keep = _attn_args(Lk=300, ws_floats=0)
    a.ws = None  # (ws_floats = 0 as well: a lost ESHAPE check then meets the size check, not a NULL workspace)
    assert _status(lib.mi355x_sam_attention, ctypes.byref(a)) == ESHAPE, "split without a workspace"
    _untouched(keep["out"], "split without a workspace")
    a, keep = _attn_args(Lk=300, ws_floats=need)  # the exact size is accepted
    assert _status(lib.mi355x_sam_attention, ctypes.byref(a)) == OK
    assert torch.isfinite(keep["out"][..., :32]).all() and torch.isnan(keep["out"][..., 32:]).all()


def test_convt2x2_ln_gelu_refusals():
    lib = native.load()
    Hs, Ws = 4, 6
    x = torch.zeros(2 * Hs * Ws + 1, 4 * 128, device=DEV)
    gamma, beta = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    cases = [("C = 3", 3, 4, 2 * Hs * Ws, 0, 0), ("C = 128", 128, 4, 2 * Hs * Ws, 0, 0), ("scatter with G = 2", 64, 2, 2 * Hs * Ws, Hs, Ws),
             ("M not a multiple of Hs Ws", 64, 4, 2 * Hs * Ws + 1, Hs, Ws)]
    for what, C_, G, M, hs, ws in cases:
        out = torch.full((4 * 3 * Hs * Ws, 4 * 128), NAN, device=DEV)  # room for any of these launches
        st = _status(lib.mi355x_convt2x2_ln_gelu, native.MI355X_F32, x.data_ptr(), x.stride(0), M, C_, G, gamma.data_ptr(), beta.data_ptr(), 1e-6,
                     out.data_ptr(), out.stride(0), hs, ws)
        assert st == ESHAPE, what
        _untouched(out, what)


def _mask_head_args(nk=2, w_offset=0):
    P, Hin, Win = 2, 5, 7
    keep = dict(x=torch.zeros(P * Hin * Win, 64, device=DEV), w=torch.zeros(64 * 128 + 8, device=DEV), b=torch.zeros(32, device=DEV),
                hyper=torch.zeros(P, 5, 32, device=DEV), out=torch.full((P, 5, 2 * Hin, 2 * Win), NAN, device=DEV))
    a = native.SamMaskHeadArgs()
    a.dtype, a.P, a.Hin, a.Win, a.nk = native.MI355X_F32, P, Hin, Win, nk
    a.x, a.ldx, a.w, a.bias = keep["x"].data_ptr(), 64, keep["w"].data_ptr() + w_offset, keep["b"].data_ptr()
    a.hyper, a.ld_hyper, a.hyper_batch_stride = keep["hyper"].data_ptr(), 32, 5 * 32
    a.out, a.out_batch_stride = keep["out"].data_ptr(), 5 * 4 * Hin * Win
    return a, keep


def test_sam_mask_head_refusals():
    lib = native.load()
    for what, kw in [("nk = 0", dict(nk=0)), ("nk = 5", dict(nk=5)), ("w 4 bytes off 16-byte alignment", dict(w_offset=4))]:
        a, keep = _mask_head_args(**kw)
        assert _status(lib.mi355x_sam_mask_head, ctypes.byref(a)) == ESHAPE, what
        _untouched(keep["out"], what)
    a, keep = _mask_head_args(w_offset=16)  # 16-byte aligned: accepted
    assert _status(lib.mi355x_sam_mask_head, ctypes.byref(a)) == OK
    assert torch.isfinite(keep["out"][:, :2]).all() and torch.isnan(keep["out"][:, 2:]).all()


def test_sam_postprocess_refusals():
    lib = native.load()
    low = torch.zeros(3, 16, 16, device=DEV)  # one plane more than the calls name
    for what, sh, sw in [("sh > R", 65, 40), ("sw = 0", 64, 0)]:
        out = torch.full((2, 48, 40), NAN, device=DEV)
        a = native.SamPostprocessArgs()
        a.dtype, a.N, a.Hin, a.Win, a.R, a.sh, a.sw, a.H, a.W = native.MI355X_F32, 2, 16, 16, 64, sh, sw, 48, 40
        a.in_, a.in_plane_stride, a.out, a.binarize, a.threshold = low.data_ptr(), 256, out.data_ptr(), 0, 0.0
        assert _status(lib.mi355x_sam_postprocess_masks, ctypes.byref(a)) == ESHAPE, what
        _untouched(out, what)
