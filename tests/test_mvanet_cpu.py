"""MVANet on the CPU: the mirror against the reference's fixtures (tests/golden/mvanet*.safetensors, mvanet_keys.json), the host folds and
tables of the lowering against the mirror's own modules, dry-run lowerings on the meta device, and the refusals."""
import os
import sys
import warnings
from collections import Counter
from pathlib import Path

import pytest
import torch

from refiners_amd import mvanet as MV
from refiners_amd import native
from refiners_amd.engine import mvanet as EM
from refiners_amd.engine.packing import Unsupported
from refiners_amd.fluxion.tree import ChainError
from tests import mvanet_cases as MC
from tests import support as S

REF = Path(os.environ.get("REFINERS_SRC") or Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "src")
E = MC.E


@pytest.fixture(scope="module")
def gold():
    return S.golden("mvanet")


def _model(case, **overrides):
    cls, kw, _side = MC.MVANET_CASES[case]
    return getattr(MV, cls)(**{**kw, **overrides}, device="meta").eval()


@pytest.mark.parametrize("case", list(MC.MVANET_CASES))
def test_mirror_keys_equal_the_reference(case):
    sd = _model(case).state_dict()
    assert list(sd) == list(MC.key_shapes(case))
    assert {k: tuple(v.shape) for k, v in sd.items()} == MC.key_shapes(case)


def test_net_has_the_reference_size():
    shapes = MC.key_shapes("NET")
    n = sum(torch.Size(s).numel() for s in shapes.values())
    assert len(shapes) == 377 and 43.5e6 < n < 43.8e6


@pytest.mark.parametrize("case", MC.BLOCK_CASES)
def test_mirror_forward_matches_reference(case, gold):
    with torch.no_grad():
        y = MC.build(case)(MC.case_input(case))
    e = S.rel_err(MC.views(y), gold[f"{case}.out"])[0]
    assert e <= 1e-5, e


@pytest.mark.parametrize("bias", [True, False])
def test_batchnorm_fold_equals_conv_then_batchnorm(bias):
    g = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv2d(8, 6, 3, padding=1, bias=bias).double()
    bn = torch.nn.BatchNorm2d(6).double().eval()
    with torch.no_grad():
        for p in (bn.weight, bn.bias, bn.running_mean):
            p.copy_(torch.randn(6, generator=g))
        bn.running_var.copy_(0.2 + torch.rand(6, generator=g))
    x = torch.randn(2, 8, 9, 7, generator=g).double()
    w, b = EM.fold_batchnorm(conv.weight, conv.bias, bn)
    with torch.no_grad():
        want = bn(conv(x))
    got = torch.nn.functional.conv2d(x, w, b, padding=1)
    assert S.rel_err(got, want)[0] <= 1e-13


@pytest.mark.parametrize("h,w", [(16, 16), (4, 2), (1, 1), (5, 3)])
def test_position_table_equals_the_mirror(h, w):
    want = MV.PositionEmbeddingSine(E // 2)(h, w)[:, 0]
    got = EM.position_embedding(h, w, E)
    assert tuple(got.shape) == (h * w, E) and torch.allclose(got, want, rtol=0, atol=2e-6)


def test_pool_positions_equal_the_mirror():
    pos = MV.PositionEmbeddingSine(E // 2)
    want = MV.MultiPoolPos([2, 8, 16], pos)(32, 32)[:, 0]
    assert torch.allclose(EM.pool_positions(32, [2, 8, 16], E), want, rtol=0, atol=2e-6)


@pytest.mark.parametrize("S_", [2, 8, 16])
def test_merge_and_quadrant_tables_equal_the_mirror(S_):
    n = S_ * S_
    ids = torch.arange(5 * n, dtype=torch.float64).view(1, 5, 1, S_, S_)  # every token carries its row number
    merged = MV.PatchMerge()(ids[:, :4])[0, 0]
    assert torch.equal(EM.merged_rows(S_), merged.long())
    quads = MV.PatchSplit()(ids[:, 4])[0, :, 0] - 4 * n
    for q in range(4):
        assert torch.equal(EM.quadrant_rows(S_, q), quads[q].long())


@pytest.mark.parametrize("S_,ratios", [(8, [1, 2, 4]), (16, [1, 2, 4]), (16, [1])])
def test_pool_model_of_the_quadrants_equals_the_mirror(S_, ratios):
    x = torch.randn(S_ * S_, 8, generator=torch.Generator().manual_seed(S_)).double()
    maps = x.view(1, S_, S_, 8).permute(0, 3, 1, 2)
    want = MV.MultiPool(ratios)(MV.PatchSplit()(maps)[0])[:, :, 0]
    for q in range(4):
        got = EM.pool_model(x, EM.quadrant_rows(S_, q), ratios)
        assert got.shape[0] == native.mvanet_pool_rows(S_ // 2, ratios) and torch.allclose(got, want[q], rtol=0, atol=1e-14)


@pytest.mark.parametrize("S_,ratios", [(8, [2, 8, 16]), (16, [2, 8, 16])])
def test_pool_model_of_the_merged_views_equals_the_mirror(S_, ratios):
    x = torch.randn(4 * S_ * S_, 8, generator=torch.Generator().manual_seed(S_)).double()
    maps = x.view(1, 4, S_, S_, 8).permute(0, 1, 4, 2, 3)
    want = MV.MultiPool(ratios)(MV.PatchMerge()(maps))[0, :, 0]
    assert torch.allclose(EM.pool_model(x, EM.merged_rows(S_), ratios), want, rtol=0, atol=1e-14)


def _dry(model, case, dtype=torch.float32, image=None):
    low = EM.MVANetLowering(torch.device("meta"), dtype)
    if case == "NET":
        image = image if image is not None else torch.empty(1, 3, 1024, 1024, device="meta", dtype=dtype)
        low.lower_net(model, image, torch.empty(1, 1, 1024, 1024, device="meta", dtype=dtype))
    else:
        side = MC.MVANET_CASES[case][2]
        x = torch.empty(5 * side * side, E, device="meta", dtype=dtype)
        low.lower_block(model, x, torch.empty_like(x))
    return low


MCRM_LAUNCHES = {"mi355x_mvanet_gate": 1, "mi355x_mvanet_pool": 1, "mi355x_gemm": 4 * 4 + 2, "mi355x_attention_general": 1, "mi355x_layernorm": 2, "mi355x_mvanet_resize_add": 1}
MCLM_LAUNCHES = {"mi355x_mvanet_pool": 2, "mi355x_gemm": 4 + 2 + 4 * 4 + 2, "mi355x_attention_general": 2, "mi355x_layernorm": 4}


@pytest.mark.parametrize("case", list(MC.MVANET_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dry_lowering_has_the_expected_launches(case, dtype):
    low = _dry(_model(case), case, dtype)
    kinds = Counter(e[2] for e in low.step)
    assert low.stats["fallback_nodes"] == [] and all(e[0] is not None for e in low.step)
    if case == "MCLM":
        assert kinds == MCLM_LAUNCHES
    elif case != "NET":
        assert kinds == MCRM_LAUNCHES
        att = next(e[1][0]._obj for e in low.step if e[2] == "mi355x_attention_general")
        side = MC.MVANET_CASES[case][2]
        assert (att.B, att.H, att.Dqk, att.Dv, att.Lq, att.Lk) == (4, 1, E, E, side * side, (side // 2) ** 2 * 21 // 16)
    else:
        blocks = 8  # depths [2, 2, 2, 2]
        swin = {"mi355x_patchify_nchw": 1, "mi355x_window_attention": blocks, "mi355x_gather_rows": 2 * blocks + 4 * 3, "mi355x_axpby": 1}
        assert all(kinds[k] == v for k, v in swin.items()) and kinds["mi355x_nhwc_to_nchw"] == 1  # the backbone's maps stay token rows: only the logits are transposed
        assert kinds["mi355x_mvanet_split_views"] == 1 and kinds["mi355x_nchw_to_nhwc"] == 1
        assert kinds["mi355x_gemm(conv)"] == 1 + 5 + 4 + 3 + 2 + 1  # shallow, laterals, one per MCRM, RearrangeMultiView, ShallowUpscaler, logits
        assert kinds["mi355x_mvanet_prelu"] == 3 and kinds["mi355x_mvanet_gate"] == 4 and kinds["mi355x_mvanet_pool"] == 2 + 4
        assert kinds["mi355x_mvanet_resize_add"] == 4 + 4 + 1 + 2  # pyramid sums, MCRM global updates, RearrangeMultiView, the two shallow sums
        assert kinds["mi355x_attention_general"] == 2 + 4
        keys = sorted(e[1][0]._obj.Lk for e in low.step if e[2] == "mi355x_attention_general")
        assert keys == [64, 276, 336, 1344, 5376, 5376]
        decoder_gemms = MCLM_LAUNCHES["mi355x_gemm"] + 4 * MCRM_LAUNCHES["mi355x_gemm"]
        assert kinds["mi355x_gemm"] == (1 + 4 * blocks + 3) + decoder_gemms
        assert kinds["mi355x_layernorm"] == (1 + 2 * blocks + 4 + 3) + 4 + 4 * 2
        gelu = [e[1][0]._obj.geglu for e in low.step if e[2] == "mi355x_gemm(conv)"]
        assert gelu.count(2) == 2 and set(gelu) == {0, 2}


def _refusal(model, case, **kw):
    with pytest.raises(Unsupported) as e:
        _dry(model, case, **kw)
    return str(e.value)


def test_refusals():
    net = _model("NET")
    assert "1 x 3 x 1024 x 1024" in _refusal(net, "NET", image=torch.empty(2, 3, 1024, 1024, device="meta"))
    assert "1 x 3 x 1024 x 1024" in _refusal(net, "NET", image=torch.empty(1, 3, 512, 512, device="meta"))
    assert "training mode" in _refusal(_model("NET").train(), "NET")
    assert "2 attention heads" in _refusal(_model("MCRM8", num_heads=2), "MCRM8")
    assert "gate convolution" in _refusal(MV.MCRM(64, 8, device="meta"), "MCRM8")  # a block of another width than its token rows
    with pytest.raises(Unsupported, match="token rows"):
        EM.MVANetLowering(torch.device("meta"), torch.float32).lower_block(MV.MCRM(64, 8, device="meta"), torch.empty(5 * 64, 64, device="meta"), torch.empty(5 * 64, 64, device="meta"))
    assert "built for views of 8" in _refusal(_model("MCRM8"), "MCRM16")
    assert "16 x 16" in _refusal(_model("MCLM"), "MCRM8")
    # whatever SwinLowering refuses: head dim 16 in the backbone
    assert "head dim" in _refusal(_model("NET", num_heads=[8, 16, 32, 64]), "NET")


def test_refuses_lora_on_a_decoder_layer():
    import refiners_amd.fluxion.layers as fl
    from refiners_amd.fluxion.adapters import LinearLora, LoraAdapter

    model = _model("MCRM8")
    ff = next(m for m in model.modules() if isinstance(m, MV.FeedForward))
    LoraAdapter(ff.layer("Linear_1", fl.Linear), LinearLora("l", in_features=E, out_features=2 * E, rank=4, device="meta")).inject(ff)
    assert "LoRA" in _refusal(model, "MCRM8")


def test_compiled_falls_back_to_the_stock_forward_with_a_warning():
    """Refused before anything is launched, so this runs without a GPU."""
    block = MC.build("MCRM8")
    wrong = MV.MCRM(E, 8, num_heads=2).eval()
    wrong.load_state_dict(block.state_dict())
    fast = EM.CompiledMVANetBlock(wrong)
    x = MC.case_input("MCRM8")
    tokens = x[0].permute(0, 2, 3, 1).reshape(-1, E).contiguous()
    with pytest.warns(RuntimeWarning, match="2 attention heads"):
        got = fast(tokens)
    with torch.no_grad():
        want = wrong(x)
    assert torch.equal(got.view(5, 8, 8, E).permute(0, 3, 1, 2), want[0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fast(tokens)  # the refusal is remembered: no second lowering attempt, no second warning
    net = EM.CompiledMVANet(_model("NET"))
    with pytest.warns(RuntimeWarning, match="1 x 3 x 1024 x 1024"), pytest.raises((ChainError, NotImplementedError, RuntimeError)):
        net(torch.zeros(2, 3, 64, 64))  # the stock forward is what runs (and raises, as the reference does for this shape)


@pytest.mark.skipif(not (REF / "refiners").exists(), reason="no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
def test_lowering_accepts_the_real_refiners_tree():
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "oracle" / "shim"), str(REF)]
    import refiners.foundationals.swin.mvanet.mclm as ref_mclm
    import refiners.foundationals.swin.mvanet.mcrm as ref_mcrm
    import refiners.foundationals.swin.mvanet.mvanet as ref_net

    classes = {"MCLM": ref_mclm.MCLM, "MCRM": ref_mcrm.MCRM, "MVANet": ref_net.MVANet}
    for case, (cls, kw, _side) in MC.MVANET_CASES.items():
        programs = []
        for model in (classes[cls](**kw, device="meta").eval(), _model(case)):
            low = _dry(model, case)
            programs.append((Counter(e[2] for e in low.step), low.stats["fallback_nodes"]))
        assert programs[0] == programs[1], case
