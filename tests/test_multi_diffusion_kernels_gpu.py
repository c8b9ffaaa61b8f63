"""pytest -m gpu: the three MultiDiffusion kernels (mi355x_md_gather, mi355x_md_target_step, mi355x_md_blend) against their torch model
(tests/multi_diffusion_cases.py, evaluated on the CPU) -- no UNet, milliseconds each.

Bounds.  gather and blend are written with single-rounding operations in the reference's order, so in float32 they must give the model's BITS
(torch.equal); in bf16 the model sees the same rounded inputs, computes in float32 and rounds once: 2^-8 relative l2 is the bound of
tests/test_style_aligned_gpu.py (one rounding to 8 significant bits is <= 2^-9 per element).  target_step repeats the arithmetic of
mi355x_cfg_ddim_step / mi355x_cfg_linear_step, whose products may be contracted into fused multiply-adds: bit-equal to those kernels at T = 1,
and against the float64 model 1e-5 (float32: a few roundings apart) / 2^-8 (bf16)."""
import pytest
import torch

from refiners_amd import native
from tests.multi_diffusion_cases import blend_model, gather_model, target_step_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
KTOL = {torch.float32: 1e-5, torch.bfloat16: 2.0**-8}
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


def _rel(got, ref):
    return float((got.double().cpu() - ref.double().cpu()).norm() / ref.double().cpu().norm())


def _same(got, ref, dtype, what):
    if dtype == torch.float32:
        assert torch.equal(got.cpu(), ref.cpu()), (what, float((got.cpu() - ref.cpu()).abs().max()))
    else:
        e = _rel(got, ref)
        assert e < KTOL[dtype], (what, e)


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W,tile", [(16, (8, 4)), (16, (7, 5)), (27, (16, 16)), (27, (7, 5))])
def test_gather_lefts_widths_both_sources(dtype, W, tile):
    """Lefts {0, 1, 11} on canvas widths {16, 27}: aligned and odd row starts, the vector (w % 4 == 0) and the element path, a crop and a noised-init row
    side by side, a model-input scale that is not 1."""
    g = torch.Generator().manual_seed(W * 100 + tile[1])
    C, H, (h, w) = 4, 20, tile
    canvas, noise = torch.randn(1, C, H, W, generator=g).to(dtype), torch.randn(1, C, H, W, generator=g).to(dtype)
    init = torch.randn(2, C, h, w, generator=g).to(dtype)
    rows = [(0, 3, 0, 0, 1.0, 0.0, 0.7), (1, H - h, 1, 1, 0.8, 0.6, 1.0), (0, 0, 11, 0, 1.0, 0.0, 0.31), (1, 2, 11, 0, 0.25, 0.97, 0.5)]
    host = native.md_gather_rows(rows)
    view = torch.full((4, C, h, w), 7.0, device=DEV, dtype=dtype)
    model_in = torch.full((8, C, h, w), 7.0, device=DEV, dtype=dtype)
    native.md_gather(canvas.to(DEV), noise.to(DEV), init.to(DEV), host.to(DEV), host, view, model_in)
    rv, rm = gather_model(canvas, noise, init, rows, h, w)
    _same(view, rv, dtype, "view")
    _same(model_in, rm, dtype, "model_in")
    assert torch.equal(view[0].cpu(), canvas[0, :, 3 : 3 + h, 0:w]) and torch.equal(model_in[:4], model_in[4:])


# ---- target step ------------------------------------------------------------------------------------------------------------------------
DDIM_ROWS = [[5.0, 0.62, 0.7846, 0.66, 0.7513, 0, 0, 0], [7.5, 0.9, 0.4359, 0.93, 0.3676, 0, 0, 0], [1.0, 0.3, 0.9539, 0.35, 0.9367, 0, 0, 0]]
LINEAR_ROWS = [[5.0, 1.6, -1.25, 0.93, 0.0, 0.11, -0.04, 1.0], [7.5, 0.0, 1.0, 1.0, -0.37, 0.0, 0.0, 0.9], [2.0, 1.1, -0.46, 0.8, 0.0, 0.3, 0.0, 1.0]]


def _step_inputs(T, shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n: torch.randn(n, *shape, generator=g).to(dtype).to(DEV)  # noqa: E731
    return mk(T), mk(2 * T), mk(T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(4, 16, 16), (3, 7, 5)])
def test_target_step_of_one_target_is_the_batch_kernels_bits(dtype, shape):
    view, uo, hist = _step_inputs(1, shape, dtype, 11)
    coef = torch.tensor(DDIM_ROWS[:1], dtype=torch.float32, device=DEV)
    x = view.clone()
    native.cfg_ddim_step(x, uo, coef)
    stepped = torch.empty_like(view)
    native.md_target_step(view, uo, stepped, None, coef, linear=False)
    assert torch.equal(stepped, x) and not torch.equal(stepped, view)
    coef = torch.tensor(LINEAR_ROWS[:1], dtype=torch.float32, device=DEV)
    x, h1 = view.clone(), hist.clone()
    native.cfg_linear_step(x, uo, h1, None, coef)
    h2 = hist.clone()
    native.md_target_step(view, uo, stepped, h2, coef, linear=True)
    assert torch.equal(stepped, x) and torch.equal(h2, h1) and not torch.equal(h2, hist)
    inplace = view.clone()  # stepped may be the view itself
    native.md_target_step(inplace, uo, inplace, hist.clone(), coef, linear=True)
    assert torch.equal(inplace, x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(4, 16, 16), (3, 7, 5)])
def test_target_step_three_targets_three_rows(dtype, shape):
    view, uo, hist = _step_inputs(3, shape, dtype, 12)
    for rows, linear in ((DDIM_ROWS, False), (LINEAR_ROWS, True)):
        coef = torch.tensor(rows, dtype=torch.float32, device=DEV)
        stepped, h = torch.empty_like(view), hist.clone()
        native.md_target_step(view, uo, stepped, h if linear else None, coef, linear=linear)
        rs, rh = target_step_model(view.cpu(), uo.cpu(), hist.cpu(), coef.cpu(), linear)
        e = [_rel(stepped[t], rs[t]) for t in range(3)]
        print(f"target_step {dtype} linear={linear} {shape}: {e}")
        assert max(e) < KTOL[dtype], e
        if linear:
            assert max(_rel(h[t], rh[t]) for t in range(3)) < KTOL[dtype]
        # a row is its target's alone: target 1 under row 1 equals a one-target call with that row
        one = torch.empty_like(view[1:2])
        h1 = hist[1:2].clone()
        native.md_target_step(view[1:2].contiguous(), torch.cat((uo[1:2], uo[4:5])), one, h1 if linear else None, coef[1:2].contiguous(), linear=linear)
        assert torch.equal(one[0], stepped[1])


# ---- blend ------------------------------------------------------------------------------------------------------------------------------
def _layouts():
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    tiles_a = [(0, 0), (0, 11), (8, 0), (8, 11)]
    zero_block = rnd(1, 1, 16, 16) * 0.9 + 0.1
    zero_block[:, :, 4:10, 3:9] = 0.0
    return {
        # (C, H, W, [(top, left, h, w, weight, mask)])
        "case_a_four_fold": (4, 24, 27, [(t, l, 16, 16, 2 if i == 1 else 1, None) for i, (t, l) in enumerate(tiles_a)]),
        "untouched_canvas": (4, 24, 27, []),
        "partly_covered_zero_block": (4, 24, 27, [(0, 0, 16, 16, 1, zero_block), (8, 11, 16, 16, 1, None)]),
        "zero_weight_mask": (4, 16, 28, [(0, 0, 16, 16, 1, torch.zeros(1, 1, 16, 16)), (0, 12, 16, 16, 3, None)]),
        "mask_shapes": (4, 16, 28, [(0, 0, 16, 16, 1, rnd(16, 16)), (0, 6, 16, 16, 2, rnd(1, 1, 16, 16)), (0, 12, 16, 16, 1, rnd(1, 4, 16, 16))]),
        "sixty_four_targets": (4, 8, 9, [(k % 5, (3 * k) % 6, 4, 4, 1 + k % 3, [None, rnd(4, 4), rnd(1, 1, 4, 4), rnd(1, 4, 4, 4)][k % 4]) for k in range(64)]),
        "mixed_sizes_vector_width": (3, 12, 32, [(0, 0, 12, 16, 1, None), (2, 9, 7, 5, 2, rnd(1, 3, 7, 5)), (0, 16, 12, 16, 1, None)]),
    }


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", list(_layouts()))
def test_blend_layouts(dtype, layout):
    C, H, W, spec = _layouts()[layout]
    g = torch.Generator().manual_seed(len(layout))
    canvas = torch.randn(1, C, H, W, generator=g).to(dtype)
    rows, parts, off = [], [torch.randn(5, generator=g).to(dtype)], 5  # (the first tile does not start the buffer)
    for top, left, h, w, weight, mask in spec:
        rows.append((top, left, h, w, weight, off, mask))
        parts.append(torch.randn(C * h * w, generator=g).to(dtype))
        off += C * h * w
    stepped = torch.cat(parts)
    want = blend_model(canvas, stepped, rows)
    dev_masks = [None if m is None else (m.to(DEV).expand(1, C, r[2], r[3]) if m.dim() == 4 else m.to(DEV).expand(C, r[2], r[3])) for r, m in ((r, r[6]) for r in rows)]
    host = native.md_blend_rows([(*r[:6], m) for r, m in zip(rows, dev_masks)])
    n = len(rows)
    desc = host.to(DEV) if n else torch.zeros(1, 64, dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        c = canvas.to(DEV)
        native.md_blend(c, stepped.to(DEV), desc, host if n else torch.zeros(1, 64, dtype=torch.uint8), n)
        outs.append(c)
    assert torch.equal(outs[0], outs[1])  # two replays: bit-equal
    _same(outs[0], want, dtype, layout)
    if layout == "untouched_canvas":
        assert torch.equal(outs[0].cpu(), canvas)
    if layout == "partly_covered_zero_block":
        assert torch.equal(outs[0].cpu()[:, :, 4:8, 3:9], canvas[:, :, 4:8, 3:9]) and torch.equal(outs[0].cpu()[:, :, 16:, :11], canvas[:, :, 16:, :11])
        assert not torch.equal(outs[0].cpu()[:, :, :4, :], canvas[:, :, :4, :])
    if layout == "zero_weight_mask":
        assert torch.equal(outs[0].cpu()[:, :, :, :12], canvas[:, :, :, :12])  # num_updates == 0 under the all-zero mask alone


# ---- contract ---------------------------------------------------------------------------------------------------------------------------
def test_contract_violations_return_their_code_and_launch_nothing():
    C, H, W, h, w = 4, 12, 13, 8, 8
    canvas, noise = torch.randn(1, C, H, W, device=DEV), torch.randn(1, C, H, W, device=DEV)
    keep = canvas.clone()
    view, model_in = torch.full((2, C, h, w), 7.0, device=DEV), torch.full((4, C, h, w), 7.0, device=DEV)
    dev = lambda t: t.to(DEV)  # noqa: E731

    def gather(rows, cv=canvas, ns=noise, init=None, v=view, m=model_in):
        host = native.md_gather_rows(rows)
        native.md_gather(cv, ns, init, dev(host), host, v, m)

    ok = [(0, 0, 0, 0, 1.0, 0.0, 1.0), (0, 4, 5, 0, 1.0, 0.0, 1.0)]
    for bad, code in (((0, 5, 0, 0, 1, 0, 1), "ESHAPE"), ((0, 0, 6, 0, 1, 0, 1), "ESHAPE"), ((0, -1, 0, 0, 1, 0, 1), "ESHAPE"), ((2, 0, 0, 0, 1, 0, 1), "EARG"),
                      ((1, 0, 0, 0, 1, 0, 1), "EARG")):  # below / right of / above the canvas, an unknown source, noised init latents without an init buffer
        with pytest.raises(native.NativeError, match=code):
            gather([ok[0], bad])
    with pytest.raises(native.NativeError, match="EARG"):  # init row 1 of a one-row buffer
        gather([ok[0], (1, 0, 0, 1, 1, 0, 1)], init=torch.zeros(1, C, h, w, device=DEV))
    both = torch.zeros(6, C, h, w, device=DEV)
    with pytest.raises(native.NativeError, match="EARG"):  # the views inside the model input
        gather(ok, v=both[:2], m=both[1:5])
    flat = torch.zeros(C * H * W + 2 * C * h * w, device=DEV)
    with pytest.raises(native.NativeError, match="EARG"):  # the views on top of the canvas they are cut from
        gather(ok, cv=flat[: C * H * W].view(1, C, H, W), v=flat[C * H * W - 8 : C * H * W - 8 + 2 * C * h * w].view(2, C, h, w))
    assert torch.equal(view, torch.full_like(view, 7.0)) and torch.equal(model_in, torch.full_like(model_in, 7.0))
    # a device row that left the contract after validation moves nothing either
    host = native.md_gather_rows(ok)
    native.md_gather(canvas, noise, None, dev(native.md_gather_rows([ok[0], (0, 5, 0, 0, 1, 0, 1)])), host, view, model_in)
    assert torch.equal(view[0], canvas[0, :, :h, :w]) and torch.equal(view[1], torch.full_like(view[1], 7.0))

    # target step
    uo, coef = torch.randn(4, C, h, w, device=DEV), torch.ones(2, 8, device=DEV)
    stepped = torch.full((2, C, h, w), 7.0, device=DEV)
    with pytest.raises(native.NativeError, match="EARG"):  # the linear form without a history buffer
        native.md_target_step(view, uo, stepped, None, coef, linear=True)
    with pytest.raises(native.NativeError, match="EARG"):  # history on top of the UNet output
        native.md_target_step(view, uo, stepped, uo[:2], coef, linear=True)
    with pytest.raises(native.NativeError, match="EARG"):  # stepped shifted over the views (only stepped == view is an in-place update)
        native.md_target_step(both[:2], uo, both[1:3], None, coef, linear=False)
    big = torch.zeros(65, 1, 1, 4, device=DEV)
    with pytest.raises(native.NativeError, match="ESHAPE"):  # T above MI355X_MD_MAX_TARGETS
        native.md_target_step(big, torch.zeros(130, 1, 1, 4, device=DEV), torch.empty_like(big), None, torch.ones(65, 8, device=DEV), linear=False)
    assert torch.equal(stepped, torch.full_like(stepped, 7.0))

    # blend
    tiles = torch.randn(2 * C * h * w, device=DEV)

    def blend(rows, cv=canvas, st=tiles, n=None):
        host = native.md_blend_rows(rows)
        native.md_blend(cv, st, dev(host), host, len(rows) if n is None else n)

    good = (0, 0, h, w, 1.0, 0, None)
    for bad, code in (((5, 0, h, w, 1.0, 0, None), "ESHAPE"), ((0, 6, h, w, 1.0, 0, None), "ESHAPE"), ((0, 0, 0, w, 1.0, 0, None), "ESHAPE"),
                      ((0, 0, h, w, 1.0, C * h * w + 1, None), "EARG"), ((0, 0, h, w, 1.0, -1, None), "EARG")):
        with pytest.raises(native.NativeError, match=code):
            blend([good, bad])
    with pytest.raises(native.NativeError, match="ESHAPE"):  # 65 targets
        blend([good] * 65)
    with pytest.raises(native.NativeError, match="EARG"):  # the tiles inside the canvas buffer
        blend([good], cv=flat[: C * H * W].view(1, C, H, W), st=flat[8:])
    assert torch.equal(canvas, keep)
    blend([good])  # (well formed: the first tile's area is replaced)
    assert torch.equal(canvas[0, :, :h, :w], tiles[: C * h * w].view(C, h, w)) and torch.equal(canvas[0, :, h:], keep[0, :, h:])
