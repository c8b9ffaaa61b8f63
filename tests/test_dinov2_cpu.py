"""DINOv2 on the CPU: the mirror against the reference's fixtures (tests/golden/dinov2*.safetensors, dinov2_keys.json), the host tap tables of
the position resampling against torch's own interpolate, the LayerScale fold, and dry-run lowerings on the meta device."""
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
from refiners_amd import dinov2 as DV
from refiners_amd.engine import dinov2 as ED
from refiners_amd.engine.packing import Unsupported
from tests import dinov2_cases as DC
from tests import support as S

REF = Path(os.environ.get("REFINERS_SRC") or Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "src")
NAMED = [f"DINOv2_{size}{reg}" for size in ("small", "base", "large", "giant") for reg in ("", "_reg")]
#: (source side, output rows, output columns): the issue's list, the identity among them
RESAMPLE_SHAPES = [(5, 3, 7), (5, 8, 4), (5, 16, 16), (5, 2, 2), (5, 1, 9), (37, 16, 16), (37, 40, 30), (5, 5, 5), (37, 37, 37)]
MODES = [("bicubic", False), ("bicubic", True), ("bilinear", False)]


@pytest.fixture(scope="module")
def gold():
    return S.golden("dinov2")


# ------------------------------------------------------------------------------------------------ mirror
@pytest.mark.parametrize("case", list(DC.DINOV2_CASES))
def test_mirror_keys_equal_the_reference(case):
    sd = DV.ViT(**DC.model_kwargs(case, fl), device="meta").state_dict()
    assert list(sd) == list(DC.key_shapes(case))
    assert {k: tuple(v.shape) for k, v in sd.items()} == DC.key_shapes(case)


@pytest.mark.parametrize("name", NAMED)
def test_named_models_equal_the_reference(name):
    model = getattr(DV, name)(device="meta")
    sd = model.state_dict()
    assert list(sd) == list(DC.key_shapes(name)) and {k: tuple(v.shape) for k, v in sd.items()} == DC.key_shapes(name)
    assert model.patch_size == 14 and model.image_size == 518 and model.num_registers == (4 if name.endswith("_reg") else 0)
    ie = next(m for m in model.modules() if isinstance(m, DV.InterpolateEmbedding))
    assert ie.antialias == name.endswith("_reg") and ie.mode == "bicubic"
    act = next(m for m in model.modules() if isinstance(m, DV.FeedForward))[1]
    assert isinstance(act, fl.GLU) == ("giant" in name)


@pytest.mark.parametrize("case", list(DC.DINOV2_CASES))
def test_mirror_forward_matches_reference(case, gold):
    with torch.no_grad():
        y = DC.mirror(case)(DC.image(case))
    assert tuple(y.shape) == (DC.DINOV2_CASES[case]["batch"], DC.tokens(case), DC.DINOV2_CASES[case]["model"]["embedding_dim"])
    for k, v in DC.output_sample(y).items():
        err = S.rel_err(v, gold[f"{case}.{k}"])[0]
        assert err <= 1e-5, (case, k, err)


def test_preprocess_is_a_host_function():
    from PIL import Image

    img = Image.new("RGB", (30, 20), (255, 0, 128))
    t = DV.preprocess(img, 28)
    assert tuple(t.shape) == (3, 28, 28) and t.dtype == torch.float32
    want = (torch.tensor([1.0, 0.0, 128 / 255]) - torch.tensor([0.485, 0.456, 0.406])) / torch.tensor([0.229, 0.224, 0.225])
    assert torch.allclose(t[:, 3, 5], want, atol=1e-6)


# ------------------------------------------------------------------------------------------------ tap tables
@pytest.fixture(scope="module")
def grids():
    g = torch.Generator().manual_seed(5)
    return {m: torch.randn(m, m, 24, generator=g) for m in (5, 37)}


@pytest.mark.parametrize("mode,aa", MODES)
@pytest.mark.parametrize("m,h,w", RESAMPLE_SHAPES)
def test_tap_tables_equal_torch_interpolate(m, h, w, mode, aa, grids):
    """The tables, applied with float32 weights as plain matmuls, against F.interpolate in float32 on unit-normal data: 1e-5 maximum
    absolute difference; the native grid is the identity bit for bit."""
    src = grids[m]
    ty, tx = ED.axis_table(m, h, mode, aa), ED.axis_table(m, w, mode, aa)
    got = ED.resample_host(src, ty, tx)
    want = F.interpolate(src.permute(2, 0, 1).unsqueeze(0), size=(h, w), mode=mode, antialias=aa).squeeze(0).permute(1, 2, 0)
    err = float((got - want).abs().max())
    print(f"{mode} aa={aa} {m}x{m} -> {h}x{w}: max abs diff {err:.3e}")
    if (h, w) == (m, m):
        assert torch.equal(got, src) and all(int(c) == 1 for t in (ty, tx) for c in t.host[1])
    assert err <= 1e-5, err


def test_tap_tables_are_in_range_and_normalised():
    for mode, aa in MODES:
        for n_in, n_out in [(5, 1), (5, 3), (5, 9), (37, 16), (37, 40), (1, 4), (4, 1)]:
            t = ED.axis_table(n_in, n_out, mode, aa)
            first, count, offset, weight = t.host
            assert bool((first >= 0).all()) and bool((first + count <= n_in).all()) and int(offset[-1] + count[-1]) == weight.numel()
            sums = torch.stack([weight[int(o) : int(o) + int(c)].double().sum() for o, c in zip(offset, count)])
            assert float((sums - 1).abs().max()) < 1e-6
    # antialiased downsampling to one cell spans the whole axis: the tap count is not capped
    assert int(ED.axis_table(37, 1, "bicubic", True).host[1][0]) == 37
    with pytest.raises(AssertionError):
        native.Dinov2Axis(torch.tensor([4]), torch.tensor([2]), torch.tensor([0]), torch.ones(2), n_src=5)  # taps 4, 5 of a 5-long axis


# ------------------------------------------------------------------------------------------------ LayerScale fold
def test_layer_scale_fold_equals_the_residual():
    torch.manual_seed(0)
    lin = fl.Linear(24, 16, dtype=torch.float64)
    ls = DV.LayerScale(16, dtype=torch.float64)
    with torch.no_grad():
        ls.weight.copy_(torch.empty(16, dtype=torch.float64).uniform_(-1.5, 1.5))
    x = torch.randn(7, 16, dtype=torch.float64)
    res = fl.Residual(fl.Lambda(lambda t: t[:, :1].expand(7, 24) + 1), lin, ls)  # any inner chain: x + ls(lin(f(x)))
    inner = x[:, :1].expand(7, 24) + 1
    w, b = ED.fold_layer_scale(lin.weight.detach(), lin.bias.detach(), ls.weight.detach())
    with torch.no_grad():
        want = res(x)
    got = x + inner @ w.t() + b
    assert float((got - want).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ dry lowerings
def _dry(model, shape, dtype=torch.float32):
    low = ED.DINOv2Lowering(torch.device("meta"), dtype)
    B, _c, H, W = ED.cropped_shape(shape, model.patch_size)
    x = torch.empty(B, 3, H, W, device="meta", dtype=dtype)
    T = 1 + model.num_registers + (H // model.patch_size) * (W // model.patch_size)
    out = torch.empty(B * ED.token_rows(T), model.embedding_dim, device="meta", dtype=dtype)
    low.lower(model, x, out)
    return low


@pytest.mark.parametrize("case", list(DC.DINOV2_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dry_lowering_has_the_expected_launches(case, dtype):
    cfg = DC.DINOV2_CASES[case]
    model = DV.ViT(**DC.model_kwargs(case, fl), device="meta", dtype=dtype)
    low = _dry(model, (cfg["batch"], 3) + cfg["size"], dtype)
    layers = cfg["model"]["num_layers"]
    swiglu = bool(cfg["model"].get("swiglu"))
    assert low.stats["fallback_nodes"] == [] and all(e[0] is not None for e in low.step + low.prologue)
    assert (low.T, low.Tp) == (DC.tokens(case), ED.token_rows(DC.tokens(case)))
    # the position table is resampled in the prologue, never in the replayed step
    assert [e[2] for e in low.prologue] == ["mi355x_dinov2_pos_resample"]
    kinds = Counter(e[2] for e in low.step)
    assert kinds["mi355x_dinov2_pos_resample"] == 0
    assert kinds["mi355x_patchify_nchw"] == 1 and kinds["mi355x_dinov2_tokens"] == 1
    assert kinds["mi355x_attention_general"] == layers
    assert kinds["mi355x_glu_silu"] == (layers if swiglu else 0)
    # one patch GEMM over all B * n rows; per layer Q|K|V, out-projection, FF1, FF2
    assert kinds["mi355x_gemm"] == 1 + 4 * layers
    # (the meta device lowers every LayerNorm standalone; on the GPU all but the first layer's first are folded into their GEMMs)
    assert kinds["mi355x_layernorm"] == 2 * layers + 1
    assert set(kinds) == {"mi355x_patchify_nchw", "mi355x_dinov2_tokens", "mi355x_attention_general", "mi355x_gemm", "mi355x_layernorm"} | ({"mi355x_glu_silu"} if swiglu else set())
    # the patch GEMM runs over all images at once; the attention masks keys beyond T
    gemm0 = next(e[1][0]._obj for e in low.step if e[2] == "mi355x_gemm")
    n = (cfg["size"][0] // 14) * (cfg["size"][1] // 14)
    assert gemm0.M == cfg["batch"] * n and gemm0.N == cfg["model"]["embedding_dim"]
    att = [e[1][0]._obj for e in low.step if e[2] == "mi355x_attention_general"]
    assert all(a.Lk == low.T and a.Lq == low.Tp and a.B == cfg["batch"] and not a.causal for a in att)
    tok = next(e[1][0]._obj for e in low.step if e[2] == "mi355x_dinov2_tokens")
    assert (tok.B, tok.n, tok.R, tok.rows) == (cfg["batch"], n, cfg["model"].get("num_registers", 0), low.Tp)


def test_dry_lowering_of_geglu():
    model = DV.ViT(embedding_dim=128, patch_size=14, image_size=70, num_layers=1, num_heads=2, feedforward_dim=256, activation=fl.GLU(fl.GeLU()), device="meta")
    low = _dry(model, (1, 3, 70, 70))
    kinds = Counter(e[2] for e in low.step)
    assert low.stats["fallback_nodes"] == [] and kinds["mi355x_glu_silu"] == 0 and kinds["mi355x_gemm"] == 5


def _refusal(model, shape=(1, 3, 70, 70), dtype=torch.float32):
    with pytest.raises(Unsupported) as e:
        _dry(model, shape, dtype)
    return str(e.value)


def test_refusals():
    kw = dict(embedding_dim=128, patch_size=14, image_size=70, num_layers=1, num_heads=2, device="meta")
    assert "interpolation mode 'nearest'" in _refusal(DV.ViT(**{**kw, "interpolate_mode": "nearest"}))
    assert "activation" in _refusal(DV.ViT(**kw, activation=fl.SiLU()))
    assert "activation" in _refusal(DV.ViT(**kw, activation=fl.GeLU(fl.GeLUApproximation.TANH)))
    assert "head dim 4" in _refusal(DV.ViT(**{**kw, "num_heads": 32}))
    assert "head dim 192" in _refusal(DV.ViT(**{**kw, "embedding_dim": 192, "num_heads": 1}))
    assert "smaller than one" in _refusal(DV.ViT(**kw), shape=(1, 3, 13, 70))


@pytest.mark.parametrize("what", ["mode", "activation", "head_dim"])
def test_compiled_falls_back_to_the_stock_forward_with_a_warning(what):
    """Refused before anything is launched, so this runs without a GPU."""
    over = {"mode": dict(interpolate_mode="nearest"), "activation": dict(activation=fl.SiLU()), "head_dim": dict(num_heads=32)}[what]
    match = {"mode": "interpolation mode", "activation": "activation", "head_dim": "head dim 4"}[what]
    model = DC.mirror("A", **over)
    fast = ED.CompiledDINOv2(model)
    x = DC.image("A")
    with pytest.warns(RuntimeWarning, match=match):
        got = fast(x)
    with torch.no_grad():
        want = model(x)
    assert torch.equal(got, want)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fast(x)  # the refusal is remembered: no second lowering attempt, no second warning


@pytest.mark.skipif(not (REF / "refiners").exists(), reason="no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
def test_lowering_accepts_the_real_refiners_tree():
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "oracle" / "shim"), str(REF)]
    import refiners.fluxion.layers as rfl
    from refiners.foundationals.dinov2.vit import ViT as RefViT

    for case in DC.DINOV2_CASES:
        cfg = DC.DINOV2_CASES[case]
        programs = []
        for cls, ns in ((RefViT, rfl), (DV.ViT, fl)):
            model = cls(**DC.model_kwargs(case, ns), device="meta")
            low = _dry(model, (cfg["batch"], 3) + cfg["size"])
            programs.append((Counter(e[2] for e in low.step), [e[2] for e in low.prologue], low.stats["fallback_nodes"]))
        assert programs[0] == programs[1], case
