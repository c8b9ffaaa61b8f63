"""Swin Transformer on the CPU: the mirror against the reference's fixtures (tests/golden/swin*.safetensors, swin_keys.json), the static
index tables and the mask arithmetic of the lowering against torch's own roll / pad / reshape, and dry-run lowerings on the meta device."""
import os
import sys
import warnings
from collections import Counter
from pathlib import Path

import pytest
import torch

from refiners_amd import swin as SW
from refiners_amd.engine import swin as ES
from refiners_amd.engine.packing import Unsupported
from tests import support as S
from tests import swin_cases as SC

REF = Path(os.environ.get("REFINERS_SRC") or Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "src")


@pytest.fixture(scope="module")
def gold():
    return S.golden("swin")


@pytest.mark.parametrize("case", list(SC.SWIN_CASES))
def test_mirror_keys_equal_the_reference(case):
    model = SW.SwinTransformer(**SC.SWIN_CASES[case]["model"], device="meta")
    sd = model.state_dict()
    assert list(sd) == list(SC.key_shapes(case))
    assert {k: tuple(v.shape) for k, v in sd.items()} == SC.key_shapes(case)
    idx = [k for k in sd if k.endswith("relative_position_index")]
    assert idx and all(sd[k].dtype == torch.int64 for k in idx)


@pytest.mark.parametrize("case", list(SC.SWIN_CASES))
def test_mirror_forward_matches_reference(case, gold):
    with torch.no_grad():
        ys = SC.mirror(case)(SC.image(case))
    names = SC.output_names(case)
    assert isinstance(ys, tuple) and len(ys) == len(names)
    for name, y in zip(names, ys):
        for k, v in SC.output_sample(y).items():
            err = S.rel_err(v, gold[f"{case}.{name}.{k}"])[0]
            assert err <= 1e-5, (case, name, k, err)


@pytest.mark.parametrize("ws", [2, 7, 12])
def test_canonical_index(ws):
    idx = SW.canonical_relative_position_index(ws)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (ws * ws, ws * ws) and torch.equal(idx, ES.canonical_index(ws))
    # the textbook construction: pairwise coordinate differences, offset to >= 0, row-major over (2 ws - 1) x (2 ws - 1)
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + ws - 1
    assert torch.equal(idx, rel[..., 0] * (2 * ws - 1) + rel[..., 1])
    assert idx.min() == 0 and idx.max() == (2 * ws - 1) ** 2 - 1 and torch.equal(idx.diagonal(), torch.full((ws * ws,), idx[0, 0].item()))


@pytest.mark.parametrize("B,g,ws,shift", [(2, 12, 6, 0), (2, 12, 6, 3), (1, 13, 6, 3), (2, 25, 12, 6), (1, 14, 7, 3), (1, 50, 12, 0)])
def test_gather_tables_equal_roll_pad_reshape(B, g, ws, shift):
    """The tables applied to an index tensor == Pad + Roll(-shift) + ToWindows and FromWindows + Roll(+shift) + Unpad of the mirror."""
    part, merge, nw = ES.window_tables(B, g, ws, shift)
    ids = torch.arange(B * g * g, dtype=torch.float32).view(B, g, g, 1) + 1  # + 1: padding (0) differs from token 0
    padded = SW.Pad(ws)(ids)
    assert padded.shape[1] == nw * ws
    windows = SW.ToWindows(ws)(SW.Roll((1, -shift), (2, -shift))(padded))
    want = windows.reshape(-1).long() - 1  # -1 where the pad sits
    assert torch.equal(part.long(), want)
    # the way back: give every row of the window layout its own number and undo
    rows = torch.arange(B * nw * nw * ws * ws, dtype=torch.float32).view(B, nw * nw, ws * ws, 1)
    back = SW.Roll((1, shift), (2, shift))(SW.FromWindows()(rows))[:, :g, :g]
    assert torch.equal(merge.long(), back.reshape(-1).long())
    assert torch.equal(part.long()[merge.long()], torch.arange(B * g * g))  # merge picks exactly the rows that hold real tokens


@pytest.mark.parametrize("B,g", [(2, 12), (1, 13), (2, 25)])
def test_merging_tables_equal_the_mirror(B, g):
    pm = SW.PatchMerging(1, device="meta")
    ids = torch.arange(B * g * g, dtype=torch.float32).view(B, g * g, 1) + 1
    x = ids
    for layer in list(pm)[:7]:  # everything before the LayerNorm
        x = layer(x)
    tabs, g2 = ES.merging_tables(B, g)
    assert tuple(x.shape) == (B, g2 * g2, 4)
    for j, t in enumerate(tabs):
        assert torch.equal(t.long(), x[..., j].reshape(-1).long() - 1), j


@pytest.mark.parametrize("nw,ws", [(2, 12), (3, 12), (5, 12), (2, 7), (4, 7), (2, 6)])
def test_kernel_mask_arithmetic_equals_the_mirror(nw, ws):
    want = SW.shift_mask(nw * ws, ws)
    got = ES.shift_mask_model(nw, ws, ws // 2)
    assert tuple(want.shape) == tuple(got.shape) and torch.equal(want, got)
    assert set(want.unique().tolist()) == {-100.0, 0.0}


def test_one_window_shifted_stage_raises_like_the_reference():
    sd = SW.WindowSDPA(4, 1, shift=True)
    with pytest.raises(IndexError):
        sd(torch.zeros(1, 1, 16, 3 * 32))


def _dry(model, B, S_, dtype=torch.float32):
    low = ES.SwinLowering(torch.device("meta"), dtype)
    x = torch.empty(B, 3, S_, S_, device="meta", dtype=dtype)
    outs = [torch.empty(s, device="meta", dtype=dtype) for s in ES.output_shapes(model, B, S_)]
    low.lower(model, x, outs)
    return low


@pytest.mark.parametrize("case", ["A", "B", "C"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dry_lowering_has_the_expected_launches(case, dtype):
    cfg = SC.SWIN_CASES[case]
    model = SW.SwinTransformer(**cfg["model"], device="meta", dtype=dtype)
    low = _dry(model, cfg["batch"], cfg["side"], dtype)
    kinds = Counter(e[2] for e in low.step)
    depths = cfg["model"]["depths"]
    blocks, stages = sum(depths), len(depths)
    assert low.stats["fallback_nodes"] == [] and all(e[0] is not None for e in low.step)
    assert kinds["mi355x_window_attention"] == blocks
    assert kinds["mi355x_patchify_nchw"] == 1 and kinds["mi355x_nhwc_to_nchw"] == stages + 1
    assert kinds["mi355x_gather_rows"] == 2 * blocks + 4 * (stages - 1)
    assert kinds["mi355x_gemm"] == 1 + 4 * blocks + (stages - 1)
    # (the meta device lowers every LayerNorm standalone; on the GPU the MLP's is folded into its GEMM)
    assert kinds["mi355x_layernorm"] == 1 + 2 * blocks + stages + (stages - 1)
    assert set(kinds) == {"mi355x_window_attention", "mi355x_patchify_nchw", "mi355x_nhwc_to_nchw", "mi355x_gather_rows", "mi355x_gemm", "mi355x_layernorm"}
    # the shifted blocks carry their shift and window count into the kernel's arguments
    wa = [e[1][0]._obj for e in low.step if e[2] == "mi355x_window_attention"]
    ws = cfg["model"]["window_size"]
    assert [a.shift for a in wa] == [(i % 2) * (ws // 2) for d in depths for i in range(d)]
    assert all(a.ws == ws and a.nw >= 2 and a.nW == cfg["batch"] * a.nw * a.nw for a in wa)


def _refusal(model, B=1, S_=192, dtype=torch.float32):
    with pytest.raises(Unsupported) as e:
        _dry(model, B, S_, dtype)
    return str(e.value)


def test_refusals():
    kw = dict(embedding_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=12, device="meta")
    assert "head dim 16" in _refusal(SW.SwinTransformer(**{**kw, "num_heads": [4, 8]}))
    assert "tokens" in _refusal(SW.SwinTransformer(**{**kw, "window_size": 13}), S_=208)
    assert "not divisible by the patch" in _refusal(SW.SwinTransformer(**kw), S_=190)
    assert "K block" in _refusal(SW.SwinTransformer(**{**kw, "embedding_dim": 32, "num_heads": [1, 2]}), dtype=torch.bfloat16)
    assert "at least 2 per side" in _refusal(SW.SwinTransformer(**kw), S_=96)  # 24 -> 2x2, then 12 -> ONE window
    low = ES.SwinLowering(torch.device("meta"), torch.float32)
    model = SW.SwinTransformer(**kw)
    with pytest.raises(Unsupported, match="non-square"):
        low.lower(model, torch.empty(1, 3, 192, 144, device="meta"), [])


def test_refuses_a_foreign_relative_position_index():
    model = SC.mirror("C")
    idx = next(m for m in model.modules() if isinstance(m, SW.RelativePositionBias)).relative_position_index
    low = ES.SwinLowering(torch.device("cpu"), torch.float32)
    x = torch.empty(1, 3, 112, 112)
    outs = [torch.empty(s) for s in ES.output_shapes(model, 1, 112)]
    low.lower(model, x, outs)  # canonical: lowers (nothing is launched while recording)
    idx[0, 1] = idx[1, 0]
    with pytest.raises(Unsupported, match="canonical"):
        ES.SwinLowering(torch.device("cpu"), torch.float32).lower(model, x, outs)


def test_refuses_lora_on_a_swin_linear():
    import refiners_amd.fluxion.layers as fl
    from refiners_amd.fluxion.adapters import LinearLora, LoraAdapter

    model = SW.SwinTransformer(embedding_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=12, device="meta")
    wa = next(m for m in model.modules() if isinstance(m, SW.WindowAttention))
    target = wa.layer("Linear_1", fl.Linear)
    LoraAdapter(target, LinearLora("l", in_features=64, out_features=192, rank=4, device="meta")).inject(wa)
    assert "LoRA" in _refusal(model)


def test_compiled_falls_back_to_the_stock_forward_with_a_warning():
    """Head dim 16: refused before anything is launched, so this runs without a GPU."""
    model = SC.mirror("C", num_heads=[4, 8])
    fast = ES.CompiledSwinTransformer(model)
    x = SC.image("C")
    with pytest.warns(RuntimeWarning, match="head dim 16"):
        got = fast(x)
    with torch.no_grad():
        want = model(x)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fast(x)  # the refusal is remembered: no second lowering attempt, no second warning


@pytest.mark.skipif(not (REF / "refiners").exists(), reason="no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
def test_lowering_accepts_the_real_refiners_tree():
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "oracle" / "shim"), str(REF)]
    from refiners.foundationals.swin.swin_transformer import SwinTransformer as RefSwin

    for case in ("A", "B", "C"):
        cfg = SC.SWIN_CASES[case]
        programs = []
        for cls in (RefSwin, SW.SwinTransformer):
            model = cls(**cfg["model"], device="meta")
            assert repr(model) == repr(SW.SwinTransformer(**cfg["model"], device="meta"))
            low = _dry(model, cfg["batch"], cfg["side"])
            programs.append((Counter(e[2] for e in low.step), low.stats["fallback_nodes"]))
        assert programs[0] == programs[1], case
