"""pytest -m gpu: reference-only control on the MI355X against what the reference's own classes computed on CPU (tests/golden/reference_only*,
tools/make_golden_reference_only.py): `CompiledUNet` on the mirror's SD1 UNet + ReferenceOnlyControlAdapter.  Both UNet passes run in one lowered
step program; the guide is a step input; `style_cfg` is live.  float32 bar: the project's, relative l2 and max <= 1e-3 against the reference's
outputs; bfloat16: the lowered step is closer to the float32 reference than the unfused bfloat16 Chain forward of the same tree."""
import os
import sys
import warnings
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import refiners_amd
from refiners_amd.engine.compiled import CompiledUNet
from refiners_amd.latent_diffusion import ReferenceOnlyControlAdapter
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from tests import ella_cases as E
from tests import reference_only_cases as R
from tests import support as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
REF = next((Path(c) for c in (os.environ.get("REFINERS_SRC"), ROOT / "oracle" / "_ref" / "src") if c and (Path(c) / "refiners").exists()), None)
F32_TOL = 1e-3


@pytest.fixture(scope="module")
def gold():
    return S.golden("reference_only")


def _within(got, ref, what):
    l2, mx = S.rel_err(got, ref)
    print(f"{what}: l2 {l2:.2e} max {mx:.2e}")
    assert l2 <= F32_TOL and mx <= F32_TOL, (what, l2, mx)


def _tree(dtype=torch.float32, lora=False):
    unet = SD1UNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sd1", R.SEED["weight_seed"]), device="cuda", dtype=dtype)
    if lora:  # before the adapter: its structural copies carry the LoRAs
        R.add_lora(unet, R.lora_api(refiners_amd.namespace()), S.key_shapes("sd1"), device="cuda", dtype=dtype)
    return unet, ReferenceOnlyControlAdapter(unet).inject()


_ON_DEVICE: dict = {}


def _inputs(case, dtype=torch.float32):
    """A case's inputs on the device, the same tensors at every call (another text tensor is another prompt: the prologue would run again)."""
    if (case, dtype) not in _ON_DEVICE:
        _ON_DEVICE[(case, dtype)] = {k: v.to(device="cuda", dtype=dtype) for k, v in R.inputs(case).items()}
    return _ON_DEVICE[(case, dtype)]


def _run(fast, unet, adapter, case, ts, dtype=torch.float32, inputs=None):
    inp = inputs or _inputs(case, dtype)
    if adapter is not None:
        adapter.set_controlnet_condition(inp["guide"])
    unet.set_clip_text_embedding(inp["text"])
    unet.set_timestep(R.timestep(ts).cuda())
    return fast(inp["x"])


def _set_style(adapter, value):
    for sub in adapter.sub_adapters:
        sub.style_cfg = value


def test_both_passes_run_lowered_and_the_guide_is_a_step_input(gpu_device, gold):
    unet, adapter = _tree()
    t0, t1 = R.CASES["main"]["timesteps"]
    fast = CompiledUNet(unet)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # a whole-tree fallback warns
        direct = _run(fast, unet, adapter, "main", t0)  # launched directly, then captured
        replayed = _run(fast, unet, adapter, "main", t0)  # the captured graph
        y1 = _run(fast, unet, adapter, "main", t1)
    assert "whole_fallback" not in fast.stats and fast.stats["fallback_nodes"] == [] and fast.stats["reference_only_sites"] == 16
    assert 0 < fast.stats["reference_only_guide_ops"] < fast.stats["step_ops"] / 2
    _within(direct, gold["main.t0"], "main t0 direct")
    assert torch.equal(direct, replayed) and fast.graph is not None, "a graph replay is not bit-equal to the direct launches"
    _within(y1, gold["main.t1"], "main t1 (graph replay)")
    assert fast.lowerings == 1 and fast.prologue_runs == 1
    assert S.rel_err(direct, gold["main.bare"])[0] > 1e-2, "the guide did not move the output"
    # another guide, same everything else: a step input, so no prologue run and no lowering -- and the output moves
    other = dict(_inputs("main"))
    other["guide"] = other["guide"].flip(0) * 0.5
    moved = _run(fast, unet, adapter, "main", t0, inputs=other)
    assert fast.lowerings == 1 and fast.prologue_runs == 1 and S.rel_err(moved, direct)[0] > 1e-3
    _within(_run(fast, unet, adapter, "main", t0), gold["main.t0"], "main t0 again")


def test_latents_where_no_level_is_a_multiple_of_64_keys(gpu_device, gold):
    unet, adapter = _tree()
    fast = CompiledUNet(unet)
    ts = R.CASES["odd"]["timesteps"][0]
    _within(_run(fast, unet, adapter, "odd", ts), gold["odd.t0"], "odd t0 direct")
    _within(_run(fast, unet, adapter, "odd", ts), gold["odd.t0"], "odd t0 (graph replay)")
    assert fast.stats["fallback_nodes"] == [] and fast.stats["reference_only_sites"] == 16


def test_style_cfg_is_live(gpu_device, gold):
    unet, adapter = _tree()
    fast = CompiledUNet(unet)
    ts = R.CASES["main"]["timesteps"][0]
    _within(_run(fast, unet, adapter, "main", ts), gold["main.t0"], "style_cfg 0.5")
    _within(_run(fast, unet, adapter, "main", ts), gold["main.t0"], "style_cfg 0.5 (graph)")
    graph = fast.graph
    for value, key in ((1.0, "main.s1"), (0.0, "main.s0"), (0.5, "main.t0")):
        _set_style(adapter, value)
        _within(_run(fast, unet, adapter, "main", ts), gold[key], f"style_cfg {value} assigned live")
        assert fast.lowerings == 1 and fast.graph is graph and fast.prologue_runs == 1
    adapter.sub_adapters[7].style_cfg = 0.25  # sites set apart by hand: no longer the lowered pattern
    with pytest.warns(RuntimeWarning, match="different style_cfg"):
        _run(fast, unet, adapter, "main", ts)
    assert "different style_cfg" in fast.stats["whole_fallback"]
    _set_style(adapter, 0.5)
    _within(_run(fast, unet, adapter, "main", ts), gold["main.t0"], "style_cfg 0.5 again, lowered again")
    assert "whole_fallback" not in fast.stats


@pytest.mark.parametrize("lora_mode", ["fused", "merged"])
def test_lora_on_the_self_attention_linears(gpu_device, gold, lora_mode):
    unet, adapter = _tree(lora=True)
    fast = CompiledUNet(unet, lora_mode=lora_mode)
    ts = R.CASES["main"]["timesteps"][0]
    y = _run(fast, unet, adapter, "main", ts)
    _within(y, gold["main.lora"], f"rank-16 LoRA on q / k / v / out of the 16 sites ({lora_mode})")
    assert fast.stats["fallback_nodes"] == [] and fast.stats["reference_only_sites"] == 16 and fast.stats["lora_sites"] == 64
    assert S.rel_err(y, gold["main.t0"])[0] > 1e-2, "the LoRA did not move the output"
    _within(_run(fast, unet, adapter, "main", ts), gold["main.lora"], "the same, graph replay")


def test_eject_returns_to_the_bare_program(gpu_device, gold):
    unet, adapter = _tree()
    fast = CompiledUNet(unet)
    ts = R.CASES["main"]["timesteps"][0]
    _within(_run(fast, unet, adapter, "main", ts), gold["main.t0"], "before eject")
    adapter.eject()
    _within(_run(fast, unet, None, "main", ts), gold["main.bare"], "ejected")
    assert "reference_only_sites" not in fast.stats and fast.stats["fallback_nodes"] == [] and fast.io.guide is None
    bare = E.program_digest(fast.low.step)
    plain = SD1UNet(4, device="meta")
    S.load_mirror_weights(plain, S.weights("sd1", R.SEED["weight_seed"]), device="cuda", dtype=torch.float32)
    other = CompiledUNet(plain)
    _run(other, plain, None, "main", ts)
    assert E.program_digest(other.low.step) == bare, "the ejected tree does not lower to the bare program"
    adapter.inject()
    _within(_run(fast, unet, adapter, "main", ts), gold["main.t0"], "after inject")


def test_a_batch_of_four_runs_the_stock_forward(gpu_device):
    unet, adapter = _tree()
    fast = CompiledUNet(unet)
    cuda = {k: torch.cat([v, v.flip(0)]) for k, v in _inputs("main").items()}
    ts = R.CASES["main"]["timesteps"][0]
    with pytest.warns(RuntimeWarning, match="batch of 4"):
        y = _run(fast, unet, adapter, "main", ts, inputs=cuda)
    assert "batch of 4" in fast.stats["whole_fallback"]
    adapter.set_controlnet_condition(cuda["guide"])
    unet.set_clip_text_embedding(cuda["text"])
    unet.set_timestep(R.timestep(ts).cuda())
    with torch.no_grad():
        want = unet(cuda["x"].clone())
    # the same torch forward on the same values twice; torch's float32 convolutions and GEMMs pick their algorithms per call and are not bit-reproducible, so the
    # two runs differ by reordered float32 sums only: 1e-5, the bar the suite holds "the same arithmetic in another order" to (a lowered result would sit at 3e-6
    # from the reference but is excluded by stats["whole_fallback"] above)
    l2, mx = S.rel_err(y, want)
    print(f"batch of 4, stock forward through the engine against the tree's own: l2 {l2:.2e} max {mx:.2e}")
    assert l2 <= 1e-5 and mx <= 1e-5


def test_bfloat16_step_beats_the_unfused_chain(gpu_device, gold):
    unet, adapter = _tree(torch.bfloat16)
    ts = R.CASES["main"]["timesteps"][0]
    fast = CompiledUNet(unet)
    y = _run(fast, unet, adapter, "main", ts, dtype=torch.bfloat16)
    assert fast.stats["fallback_nodes"] == [] and fast.stats["reference_only_sites"] == 16
    chain = R.run(unet, adapter, "main", ts, device="cuda", dtype=torch.bfloat16)
    mine, stock = S.rel_err(y, gold["main.t0"]), S.rel_err(chain, gold["main.t0"])
    print(f"bf16 against the float32 reference: lowered l2 {mine[0]:.3e} max {mine[1]:.3e} | unfused Chain l2 {stock[0]:.3e} max {stock[1]:.3e}")
    assert torch.isfinite(y.float()).all() and mine[0] < stock[0]


@pytest.mark.skipif(REF is None, reason="no refiners checkout (REFINERS_SRC / oracle/_ref)")
def test_reference_tree_with_its_own_adapter(gpu_device, gold):
    sys.path[:0] = [p for p in (str(ROOT / "oracle" / "shim"), str(REF)) if p not in sys.path]
    from refiners.foundationals.latent_diffusion.reference_only_control import ReferenceOnlyControlAdapter as RefAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet as RefUNet

    unet = RefUNet(4, device="meta")
    unet.load_state_dict({k: v.cuda() for k, v in S.weights("sd1", R.SEED["weight_seed"]).items()}, assign=True)
    adapter = RefAdapter(unet).inject()
    assert type(unet).__module__.startswith("refiners.")
    fast = CompiledUNet(unet)
    for i, ts in enumerate(R.CASES["main"]["timesteps"]):
        _within(_run(fast, unet, adapter, "main", ts), gold[f"main.t{i}"], f"refiners' own tree + ReferenceOnlyControlAdapter t{i}")
    assert fast.stats["fallback_nodes"] == [] and fast.stats["reference_only_sites"] == 16 and fast.prologue_runs == 1 and fast.lowerings == 1


def test_sampling_loop_reads_the_guide_at_every_step(gpu_device):
    """CompiledSDXL.step on the SD1 tree: one program for the pair (no cfg_split), the guide read from the adapter's context on every call.  The UNet
    output of a step is what CompiledUNet computes at that step's timestep from the same guide."""
    from refiners_amd.engine.compiled import CompiledSDXL

    unet, adapter = _tree()
    inp = _inputs("main")
    pipe = CompiledSDXL(unet, num_inference_steps=10)
    pipe.set_inputs(inp["x"][:1], clip_text_embedding=inp["text"])
    fast = CompiledUNet(unet)
    for s, guide in ((3, inp["guide"]), (4, inp["guide"].flip(0))):
        adapter.set_controlnet_condition(guide)
        pipe.set_inputs(inp["x"][:1], clip_text_embedding=inp["text"])
        pipe.step(s)
        got = pipe.engine.io.out.clone()
        assert pipe.engine.stats["fallback_nodes"] == [] and pipe.engine.stats["reference_only_sites"] == 16 and pipe.engine_c is None
        pair = dict(inp, x=torch.cat([inp["x"][:1], inp["x"][:1]]), guide=guide)
        want = _run(fast, unet, adapter, "main", float(pipe.ts_table[s]), inputs=pair)
        l2, mx = S.rel_err(got, want)
        print(f"sampling loop, step {s}: l2 {l2:.2e} max {mx:.2e} against CompiledUNet")
        assert l2 <= 1e-5 and mx <= 1e-5  # the same kernels on the same values; only the time table's row count differs
    assert pipe.engine.lowerings == 1 and pipe.engine.prologue_runs == 1
