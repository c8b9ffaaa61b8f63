"""CompiledMVANet and the block entry points (refiners_amd/engine/mvanet.py) on the GPU against the reference's fixtures
(tests/golden/mvanet*.safetensors, written by tools/make_golden_mvanet.py from refiners' own classes on CPU float32)."""
import sys
import warnings
from pathlib import Path

import pytest
import torch

from refiners_amd import mvanet as MV
from refiners_amd.engine.mvanet import CompiledMVANet, CompiledMVANetBlock
from tests import mvanet_cases as MC
from tests.support import golden, rel_err
from tests.swin_cases import output_sample

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
REF = Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "src"
BAR = 1e-3  # the project's float32 bar (relative l2)


@pytest.fixture(scope="module")
def gold():
    return golden("mvanet")


@pytest.fixture(scope="module")
def net32():
    """The mirror's NET with the fixture's weights, float32 on the GPU, and its engine: built once for every whole-net test of this file."""
    model = MC.build("NET", device=DEV)
    return model, CompiledMVANet(model)


def _tokens(x):
    """(1, 5, E, S, S) -> [5 S S, E]"""
    return x[0].permute(0, 2, 3, 1).reshape(-1, x.shape[2]).contiguous()


def _maps(t, S):
    """[5 S S, E] -> (5, E, S, S)"""
    return t.view(5, S, S, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", MC.BLOCK_CASES)
def test_blocks_float32_match_the_reference(case, gold):
    model = MC.build(case, device=DEV)
    S = MC.MVANET_CASES[case][2]
    x = _tokens(MC.case_input(case).to(DEV))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        direct = CompiledMVANetBlock(model, use_graph=False)
        y0 = direct(x)
        fast = CompiledMVANetBlock(model)
        y1, y2 = fast(x), fast(x)  # the direct run that also captures, then the replay
    assert fast.stats["fallback_nodes"] == [] and fast.lowerings == 1
    e = rel_err(_maps(y0, S), gold[f"{case}.out"])[0]
    print(f"{case} float32: rel l2 = {e:.3e}, {fast.stats['step_ops']} launches")
    assert e <= BAR, e
    assert torch.equal(y0, y1) and torch.equal(y1, y2), "the graph replay differs from the direct run"


def test_net_float32_matches_the_reference(net32, gold):
    model, _shared = net32
    image = MC.case_input("NET").to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fast = CompiledMVANet(model)
        fast.keep_intermediates = True  # copies of the Pyramid and RearrangeMultiView outputs, so that a failure can be located
        y1 = fast(image)
        y2 = fast(image)
        y0 = CompiledMVANet(model, use_graph=False)(image)
    assert fast.stats["fallback_nodes"] == []
    got = dict(fast.intermediates, logits=y1)
    for name in MC.NET_TENSORS:
        for k, v in output_sample(got[name]).items():
            e = rel_err(v, gold[f"NET.{name}.{k}"])[0]
            print(f"NET float32 {name}.{k}: rel l2 = {e:.3e} ({fast.stats['step_ops']} launches)")
            assert e <= BAR, (name, k, e)
    assert torch.equal(y1, y2) and torch.equal(y0, y1), "the graph replay differs from the direct run"


def _bf16_pair(case, gold, net=False):
    """(engine error, unfused mirror error) of bfloat16 against the float32 fixture: relative l2 where the fixture is sampled, which is what
    tests/test_swin_gpu.py compares.  NET's other two stored figures are printed: its logits have ONE channel, so `mean` and `meanabs` are one
    number each, and the ratio of two single numbers' errors is not a measure of accuracy (measured: sample 1.61e-2 against 2.25e-2 unfused,
    meanabs 1.70e-3 against 1.33e-2, mean 2.80e-1 against 9.02e-2 of a mean that is 4 % of the logits' rms)."""
    model = MC.build(case, device=DEV, dtype=torch.bfloat16)
    x = MC.case_input(case).to(DEV, torch.bfloat16)
    if net:
        with torch.no_grad():
            stock = model(x)
        fast = CompiledMVANet(model)(x)
        a, b = output_sample(fast), output_sample(stock)
        errs = [(rel_err(a[k], gold[f"NET.logits.{k}"])[0], rel_err(b[k], gold[f"NET.logits.{k}"])[0]) for k in a]
        for k, (e, m) in zip(a, errs):
            print(f"NET bfloat16 logits.{k}: engine rel l2 = {e:.3e}, unfused mirror = {m:.3e}")
        return errs[list(a).index("sample")]
    S = MC.MVANET_CASES[case][2]
    with torch.no_grad():
        stock = model(x)
    fast = CompiledMVANetBlock(model)(_tokens(x))
    return rel_err(_maps(fast, S), gold[f"{case}.out"])[0], rel_err(stock[0], gold[f"{case}.out"])[0]


@pytest.mark.parametrize("case", ["MCRM32", "NET"])
def test_bfloat16_is_no_worse_than_the_unfused_forward(case, gold):
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        e, m = _bf16_pair(case, gold, net=case == "NET")
    print(f"{case} bfloat16: engine rel l2 = {e:.3e}, unfused mirror = {m:.3e}, ratio {e / m:.3f}")
    assert e <= 1.15 * m, (e, m)


def test_second_image_and_live_edits(net32):
    model, fast = net32
    g = torch.Generator().manual_seed(7)
    image = torch.randn(1, 3, 1024, 1024, generator=g).to(DEV)
    fast(MC.case_input("NET").to(DEV))
    n = fast.lowerings
    y = fast(image)
    assert fast.lowerings == n, "a second image re-lowered"
    direct = CompiledMVANet(model, use_graph=False)
    assert torch.equal(y, direct(image))
    prelu = next(m for m in model.modules() if isinstance(m, MV.PReLU))
    conv = model[6][1][2]  # RearrangeMultiView's last convolution
    saved = prelu.weight.detach().clone(), conv.weight.detach().clone()
    try:
        with torch.no_grad():
            prelu.weight.mul_(-1.0)
        y2 = fast(image)
        assert fast.lowerings == n, "a PReLU slope edit re-lowered"
        with torch.no_grad():
            want = model(image)
        assert not torch.equal(y2, y) and rel_err(y2, want)[0] <= BAR
        with torch.no_grad():
            conv.weight.mul_(0.5)
        y3 = fast(image)
        assert fast.lowerings == n + 1, "a convolution weight edit did not re-lower"
        with torch.no_grad():
            want = model(image)
        assert rel_err(y3, want)[0] <= BAR
    finally:
        with torch.no_grad():
            prelu.weight.copy_(saved[0])
            conv.weight.copy_(saved[1])


def test_fallbacks_warn_and_run_the_stock_forward(net32):
    from refiners_amd.fluxion.tree import ChainError

    model, _fast = net32
    fast = CompiledMVANet(model)
    with pytest.warns(RuntimeWarning, match="1 x 3 x 1024 x 1024"), pytest.raises(ChainError):  # the stock forward raises for batch 2, as the reference does
        fast(torch.zeros(2, 3, 1024, 1024, device=DEV))
    trained = MC.build("NET", device=DEV).train()  # (a model of its own: a training-mode forward moves the running statistics)
    image = MC.case_input("NET").to(DEV)
    fast = CompiledMVANet(trained)
    with pytest.warns(RuntimeWarning, match="training mode"):
        y = fast(image)
    with torch.no_grad():
        want = trained(image)
    assert fast.lowerings == 0 and rel_err(y, want)[0] <= 1e-5


@pytest.mark.skipif(not REF.exists(), reason="the reference checkout is not staged under oracle/_ref (build() stages it where the checkout exists)")
def test_refiners_own_tree_runs_natively(gold):
    sys.path[:0] = [str(REF.parent.parent / "shim"), str(REF)]
    import refiners.foundationals.swin.mvanet.mvanet as ref_net

    model = MC.build("NET", namespace=ref_net, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fast = CompiledMVANet(model)
        y = fast(MC.case_input("NET").to(DEV))
    assert fast.stats["fallback_nodes"] == []
    for k, v in output_sample(y).items():
        assert rel_err(v, gold[f"NET.logits.{k}"])[0] <= BAR, k
