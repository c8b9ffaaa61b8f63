"""InformativeDrawings on the CPU: the mirror against the reference's fixtures (tests/golden/lineart.safetensors, lineart_keys.json), the
phase-weight packing of the transposed convolution and the ring index helper against torch, the extension header's binding, dry-run
lowerings on the meta device and the fallbacks."""
import ctypes as C
import os
import sys
import warnings
from collections import Counter
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import refiners_amd.fluxion.layers as fl
from refiners_amd import native
from refiners_amd.engine import lineart as EL
from refiners_amd.engine.packing import Unsupported
from refiners_amd.latent_diffusion.preprocessors import InformativeDrawings
from tests import lineart_cases as LC
from tests import support as S

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")


@pytest.fixture(scope="module")
def gold():
    return S.golden("lineart")


# ------------------------------------------------------------------------------------------------ mirror
@pytest.mark.parametrize("n", LC.BLOCK_COUNTS)
def test_mirror_repr_and_keys_equal_the_reference(n):
    model = InformativeDrawings(n_residual_blocks=n, device="meta")
    ref = LC.reference_tree(n)
    sd = model.state_dict()
    assert repr(model) == ref["repr"]
    assert list(sd) == list(ref["keys"]) and {k: tuple(v.shape) for k, v in sd.items()} == ref["keys"]


def test_new_layers_wrap_the_torch_modules():
    norm, pad = fl.InstanceNorm2d(8, eps=1e-3), fl.ReflectionPad2d(2)
    assert isinstance(norm, torch.nn.InstanceNorm2d) and not norm.affine and not norm.track_running_stats and norm.eps == 1e-3 and not list(norm.parameters())
    assert isinstance(pad, torch.nn.ReflectionPad2d) and tuple(pad.padding) == (2, 2, 2, 2)
    x = torch.randn(2, 8, 5, 6)
    assert torch.equal(norm(x), F.instance_norm(x, eps=1e-3)) and torch.equal(pad(x), F.pad(x, (2, 2, 2, 2), mode="reflect"))


@pytest.mark.parametrize("case", list(LC.LINEART_CASES))
def test_mirror_forward_matches_reference(case, gold):
    with torch.no_grad():
        y = LC.mirror(case)(LC.image(case))
    B, _c, H, W = LC.LINEART_CASES[case]["shape"]
    assert tuple(y.shape) == LC.out_shape(case) == (B, 1) + EL.out_size(H, W)
    l2, mx = S.rel_err(y, gold[f"{case}.out"])
    assert l2 <= 1e-5 and mx <= 1e-5, (case, l2, mx)


# ------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("C_,Cp", [(5, 3), (256, 128)])
def test_phase_weights_equal_conv_transpose(C_, Cp):
    g = torch.Generator().manual_seed(C_)
    w = torch.randn(C_, Cp, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(2, C_, 5, 7, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    packed = EL.pack_convt_phases(w)
    assert tuple(packed.shape) == (4 * Cp, C_, 3, 3) and int((packed != 0).sum()) == 9 * C_ * Cp  # 1 + 2 + 2 + 4 taps: every weight once
    quad = F.conv2d(x, packed, padding=1)  # [B, (py, px, c'), a, b]
    got = quad.view(2, 2, 2, Cp, 5, 7).permute(0, 3, 4, 1, 5, 2).reshape(2, Cp, 10, 14)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("h,w", [(2, 3), (4, 9)])
def test_ring_index_equals_reflection_padding(h, w, p):
    if p >= min(h, w):  # ReflectionPad2d itself refuses a padding that is not smaller than the side: so does the helper
        with pytest.raises(AssertionError):
            EL.reflect_index(min(h, w), p)
        with pytest.raises(RuntimeError):
            F.pad(torch.zeros(1, 1, h, w), (p,) * 4, mode="reflect")
        return
    x = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w)
    iy, ix = EL.reflect_index(h, p), EL.reflect_index(w, p)
    assert torch.equal(x[:, :, iy][:, :, :, ix], F.pad(x, (p,) * 4, mode="reflect"))


def test_reflected_3x3_is_the_interior_of_the_zero_padded_one():
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(1, 4, 2, 3, generator=g, dtype=torch.float64), torch.randn(5, 4, 3, 3, generator=g, dtype=torch.float64)
    ringed = F.pad(x, (1, 1, 1, 1), mode="reflect")
    assert torch.equal(F.conv2d(ringed, w), F.conv2d(ringed, w, padding=1)[:, :, 1:-1, 1:-1])


# ------------------------------------------------------------------------------------------------ ABI
def test_lineart_header_is_bound_and_exported():
    """Two prototypes of the lineart header written out by hand (its names, layouts and exports: tests/test_abi_header_cpu.py), and its one
    host-side function."""
    from refiners_amd.build_native import build_native

    build_native()
    lib = native.load()
    assert lib.mi355x_lineart_head.argtypes == [C.POINTER(native.LineartHeadArgs), C.c_void_p] and lib.mi355x_lineart_in_stats_ws_floats.restype == C.c_int64
    # the scratch the statistics ask for is host arithmetic: slabs x columns x (mean, M2), four column groups for the quadrant layout
    assert native.lineart_in_stats_ws_floats(1, 2, 3, 64) == 1 * 64 * 2 and native.lineart_in_stats_ws_floats(2, 4, 6, 64, native.LINEART_QUAD) == 2 * 256 * 2
    assert native.lineart_in_stats_ws_floats(1, 512, 512, 64) == 1024 * 64 * 2 and native.lineart_in_stats_ws_floats(1, 19, 25, 128) == 4 * 128 * 2


# ------------------------------------------------------------------------------------------------ dry lowerings
def _dry(model, shape, dtype=torch.float32):
    x = torch.empty(shape, device="meta", dtype=dtype)
    out = torch.empty((shape[0], 1) + EL.out_size(shape[2], shape[3]), device="meta", dtype=dtype)
    return EL.lower(model, x, out)


@pytest.mark.parametrize("case", ["A", "C"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dry_lowering_has_the_expected_launches(case, dtype):
    cfg = LC.LINEART_CASES[case]
    n = cfg["n_residual_blocks"]
    B, _c, H, W = cfg["shape"]
    model = InformativeDrawings(n_residual_blocks=n, device="meta", dtype=dtype)
    low = _dry(model, cfg["shape"], dtype)
    assert low.stats["fallback_nodes"] == [] and all(e[0] is not None for e in low.step) and low.prologue == []
    kinds = Counter(e[2] for e in low.step)
    assert kinds == {"mi355x_lineart_stem": 1, "mi355x_lineart_head": 1, "mi355x_gemm(conv)": 4 + 2 * n, "mi355x_lineart_in_stats": 5 + 2 * n, "mi355x_lineart_in_apply": 4 + 2 * n}
    assert len(low.step) == 15 + 6 * n  # 33 for the default three blocks
    h, w = EL.out_size(H, W)[0] // 4, EL.out_size(H, W)[1] // 4
    convs = [e[1][0]._obj for e in low.step if e[2] == "mi355x_gemm(conv)"]
    # the residual convolutions run over the ringed (h + 2) x (w + 2) image; the transposed ones write four column groups
    assert [(c.M, c.N) for c in convs] == ([(B * (H // 2) * (W // 2), 128), (B * h * w, 256)] + [(B * (h + 2) * (w + 2), 256)] * (2 * n) + [(B * h * w, 512), (B * 4 * h * w, 256)])
    assert all(c.seg[0].ksize == 3 and not c.bias for c in convs)  # no convolution keeps its bias: an InstanceNorm2d follows each
    applies = [e[1][0]._obj for e in low.step if e[2] == "mi355x_lineart_in_apply"]
    # (a meta tensor has no address: the residual operand shows in its leading dimension)
    assert [(a.layout, a.pad, a.ring, a.ldr > 0, a.relu) for a in applies] == (
        [(native.LINEART_ROWS, 0, 0, False, 1)] * 2 + [(native.LINEART_ROWS, 0, 1, False, 1)]
        + [(native.LINEART_PADDED, 1, 1, False, 1), (native.LINEART_PADDED, 1, 1, True, 0)] * (n - 1) + [(native.LINEART_PADDED, 1, 1, False, 1), (native.LINEART_PADDED, 1, 0, True, 0)]
        + [(native.LINEART_QUAD, 0, 0, False, 1)])
    head = next(e[1][0]._obj for e in low.step if e[2] == "mi355x_lineart_head")
    assert (head.layout, head.B, head.H, head.W) == (native.LINEART_QUAD, B, 4 * h, 4 * w)


def test_dry_lowering_without_residual_blocks_writes_no_ring():
    low = _dry(InformativeDrawings(n_residual_blocks=0, device="meta"), (1, 3, 5, 5))
    assert len(low.step) == 15 and all(e[1][0]._obj.ring == 0 for e in low.step if e[2] == "mi355x_lineart_in_apply")


VARIANTS = {
    "out_channels": (dict(out_channels=3), "out_channels 3"),
    "in_channels": (dict(in_channels=5), "in_channels 5"),
}


def _affine(model):
    chain = model[0]
    chain.replace(chain[2], torch.nn.InstanceNorm2d(64, affine=True))


def _running(model):
    chain = model[1]
    chain.replace(chain[1], torch.nn.InstanceNorm2d(128, track_running_stats=True))


def _odd_tree(model):
    model.insert(3, fl.Identity())


@pytest.mark.parametrize("what", ["out_channels", "in_channels", "affine", "running", "tree"])
def test_unsupported_variants_fall_back_with_a_warning(what):
    """Refused before anything is launched, so this runs without a GPU."""
    kw, match = VARIANTS.get(what, ({}, {"affine": "affine parameters", "running": "running statistics", "tree": "unexpected InformativeDrawings layout"}.get(what)))
    model = LC.mirror("C", **kw) if kw else LC.mirror("C")
    if what in ("affine", "running"):
        # (torch's own class stands in for a norm with parameters: fl.InstanceNorm2d has no such option, and nodes are matched by class name)
        (_affine if what == "affine" else _running)(model)
    elif what == "tree":
        _odd_tree(model)
    model.eval()
    fast = EL.CompiledInformativeDrawings(model)
    shape = (1, kw.get("in_channels", 3), 8, 12)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1))
    with pytest.warns(RuntimeWarning, match=match):
        got = fast(x)
    with torch.no_grad():
        want = model(x)
    assert torch.equal(got, want) and fast.stats["whole_fallback"] and fast.stats["step_ops"] == 0 and fast.program is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fast(x)  # the refusal is remembered: no second lowering attempt, no second warning


@pytest.mark.parametrize("shape,n", [((1, 3, 3, 8), 0), ((1, 3, 8, 3), 3), ((1, 3, 4, 4), 0), ((1, 3, 4, 8), 1)])
def test_sizes_the_model_refuses_raise_before_anything_is_launched(shape, n):
    model = InformativeDrawings(n_residual_blocks=n, device="meta")
    fast = EL.CompiledInformativeDrawings(model)
    with pytest.raises(RuntimeError) as e:
        fast(torch.empty(shape, device="meta"))
    assert isinstance(e.value, fl.ChainError) and fast.lowerings == 0
    with pytest.raises(RuntimeError):  # the same kind of error the model's own forward ends in
        InformativeDrawings(n_residual_blocks=n)(torch.rand(shape))
    # (a 1 x 2 quarter-resolution map without residual blocks is accepted by the reference, and lowered)
    assert len(_dry(InformativeDrawings(n_residual_blocks=0, device="meta"), (1, 3, 4, 8)).step) == 15


def test_refusals_name_their_reason():
    for kw, why in VARIANTS.values():
        with pytest.raises(Unsupported, match=why):
            _dry(InformativeDrawings(n_residual_blocks=1, device="meta", **kw), (1, kw.get("in_channels", 3), 8, 12))


@pytest.mark.skipif(not (REF / "refiners").exists(), reason="no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
def test_lowering_accepts_the_real_refiners_tree():
    sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF)]
    from refiners.foundationals.latent_diffusion.preprocessors.informative_drawings import InformativeDrawings as RefDrawings

    for case, cfg in LC.LINEART_CASES.items():
        programs = []
        for cls in (RefDrawings, InformativeDrawings):
            low = _dry(cls(n_residual_blocks=cfg["n_residual_blocks"], device="meta"), cfg["shape"])
            programs.append(([e[2] for e in low.step], low.stats["fallback_nodes"]))
        assert programs[0] == programs[1], case
    ref = RefDrawings(n_residual_blocks=1)
    ref.load_state_dict(LC.weights("C"))  # a checkpoint of the reference's keys loads into either tree unchanged
    LC.mirror("C").load_state_dict(ref.state_dict())
