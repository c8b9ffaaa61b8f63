"""pytest -m gpu: ELLA on the MI355X against what the reference's own classes computed on CPU (tests/golden/ella*, tools/make_golden_ella.py).

`CompiledELLA` alone at the cases of tests/ella_cases.py, then the whole SD1 UNet with SD1ELLAAdapter through `CompiledUNet`: the resampler
and the K / V^T projections of its tokens run inside the step program, the prologue runs once per prompt, eject / inject switch between the
plain and the ELLA program.  float32 bar: the project's, relative l2 and max <= 1e-3 against the reference's outputs; bfloat16: the lowered
step is closer to the float32 reference than the unfused bfloat16 Chain forward of the same tree (the project's bf16 convention)."""
import os
import sys
import warnings
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import refiners_amd
from refiners_amd import synth
from refiners_amd.engine.compiled import CompiledUNet
from refiners_amd.engine.ella import CompiledELLA
from refiners_amd.latent_diffusion import SD1ELLAAdapter
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from tests import ella_cases as E
from tests import support as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
REF = next((Path(c) for c in (os.environ.get("REFINERS_SRC"), ROOT / "oracle" / "_ref" / "src") if c and (Path(c) / "refiners").exists()), None)
F32_TOL = 1e-3


@pytest.fixture(scope="module")
def gold():
    return S.golden("ella")


def _within(got, ref, what):
    l2, mx = S.rel_err(got, ref)
    print(f"{what}: l2 {l2:.2e} max {mx:.2e}")
    assert l2 <= F32_TOL and mx <= F32_TOL, (what, l2, mx)


# ------------------------------------------------------------------------------------------------ the resampler alone
@pytest.mark.parametrize("case", list(E.ELLA_CASES))
def test_compiled_ella_matches_the_reference(gpu_device, case, gold):
    cfg = E.ELLA_CASES[case]
    fast = CompiledELLA(E.mirror(case, device="cuda"))
    llm = E.llm_embedding(case).cuda()
    t0, t1 = cfg["timesteps"]
    direct = fast(E.timestep(t0), llm)  # first call: launched directly, then captured
    m = cfg["model"]
    assert tuple(direct.shape) == (cfg["batch"], m["num_latents"], m.get("out_dim") or m["width"])
    _within(direct, gold[f"{case}.t0"], f"{case} t0 direct")
    replayed = fast(E.timestep(t0), llm)  # the captured graph
    assert torch.equal(direct, replayed) and fast.entries[next(iter(fast.entries))].program.graph is not None
    _within(fast(E.timestep(t1), llm), gold[f"{case}.t1"], f"{case} t1 graph")
    _within(fast(E.timestep(t0), llm), gold[f"{case}.t0"], f"{case} t0 again")
    assert fast.lowerings == 1 and fast.prologue_runs == 1 and fast.stats["ella_layers"] == m["num_layers"]
    # 7 launches per layer, around them: RangeEncoder (sinusoid, 2 GEMMs, SiLU), SiLU + time table, latents, and the output stage
    project, ragged = m.get("out_dim") is not None, m["num_latents"] % 64 != 0
    tail = int(project) + (cfg["batch"] if ragged else int(project))  # OutputProjection's Linear | its LayerNorm (or a copy) per sample where samples are no whole 64-row blocks
    assert fast.stats["step_ops"] == 7 * m["num_layers"] + 7 + tail, fast.stats
    other = E.llm_embedding(case, shift=1).cuda()
    moved = fast(E.timestep(t0), other)
    assert fast.prologue_runs == 2 and fast.lowerings == 1 and not torch.allclose(moved, direct, atol=1e-3)


def test_compiled_ella_padding_rows_stay_zero(gpu_device):
    fast = CompiledELLA(E.mirror("odd", device="cuda"))
    fast(E.timestep(250.0), E.llm_embedding("odd").cuda())
    entry = fast.entries[next(iter(fast.entries))]
    rows = entry.out.view(3, 64, -1)
    assert bool((rows[:, 16:] == 0).all()) and bool((rows[:, :16] != 0).any())


# ------------------------------------------------------------------------------------------------ the UNet with the adapter
def _tree(dtype=torch.float32):
    c = E.UNET_CASE
    unet = SD1UNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sd1", c["unet_weight_seed"]), device="cuda", dtype=dtype)
    adapter = SD1ELLAAdapter(unet)
    adapter.latents_encoder.load_state_dict({k: v.to(device="cuda", dtype=dtype) for k, v in E.weights("sd1_full").items()}, assign=True)
    adapter.inject()
    inp = {k: v.to(device="cuda", dtype=dtype) for k, v in E.unet_inputs().items()}
    return unet, adapter, inp


def _run(fast, unet, adapter, ts, llm, x):
    adapter.set_llm_text_embedding(llm)
    unet.set_timestep(E.timestep(ts).cuda())
    return fast(x)


def test_unet_with_ella_runs_lowered_and_keeps_its_prologue(gpu_device, gold):
    unet, adapter, inp = _tree()
    t0, t1 = E.UNET_CASE["timesteps"]
    fast = CompiledUNet(unet)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # a whole-tree fallback warns
        y0 = _run(fast, unet, adapter, t0, inp["llm"], inp["x"])
        y1 = _run(fast, unet, adapter, t1, inp["llm"], inp["x"])
    assert "whole_fallback" not in fast.stats and fast.stats["fallback_nodes"] == [] and fast.stats["ella_sites"] == 16 and fast.stats["ella_layers"] == 6
    _within(y0, gold["unet.t0"], "unet + ella t0")
    _within(y1, gold["unet.t1"], "unet + ella t1 (graph replay)")
    assert fast.prologue_runs == 1 and fast.stats["prologue_runs"] == 1 and fast.lowerings == 1 and fast.graph is not None
    assert S.rel_err(y1, y0)[0] > 1e-3, "the conditioning did not move with the timestep"
    _within(_run(fast, unet, adapter, t0, inp["llm"], inp["x"]), gold["unet.t0"], "unet + ella t0 again")
    assert fast.prologue_runs == 1
    other = E.unet_inputs(shift=1)["llm"].cuda()
    _within(_run(fast, unet, adapter, t0, other, inp["x"]), gold["unet.llm2"], "unet + ella, another LLM embedding")
    assert fast.prologue_runs == 2 and fast.lowerings == 1


def test_engine_given_the_adapter_chain(gpu_device, gold):
    unet, adapter, inp = _tree()
    fast = CompiledUNet(adapter)
    y = _run(fast, unet, adapter, E.UNET_CASE["timesteps"][0], inp["llm"], inp["x"])
    _within(y, gold["unet.t0"], "CompiledUNet(adapter)")
    assert fast.stats["fallback_nodes"] == [] and fast.stats["ella_sites"] == 16


def test_eject_returns_to_the_plain_program_and_inject_to_ella(gpu_device, gold):
    unet, adapter, inp = _tree()
    t0 = E.UNET_CASE["timesteps"][0]
    fast = CompiledUNet(unet)
    _within(_run(fast, unet, adapter, t0, inp["llm"], inp["x"]), gold["unet.t0"], "before eject")
    ella_ops = fast.stats["step_ops"]
    adapter.eject()
    cfg = S.CASES["sd1_bare"]
    x = torch.randn((1, 4, *cfg["latent_hw"]), generator=synth._gen("in.x", cfg["input_seed"])).cuda()
    text = torch.randn((1, 77, 768), generator=synth._gen("in.text", cfg["input_seed"])).cuda()
    unet.set_clip_text_embedding(text)
    unet.set_timestep(torch.tensor([cfg["timestep"]], device="cuda"))
    _within(fast(x), S.golden("sd1_bare")["unet_out"], "ejected: sd1_bare")
    assert "ella_sites" not in fast.stats and fast.stats["fallback_nodes"] == [] and fast.stats["step_ops"] < ella_ops - 49
    assert not any(e[2] == "mi355x_ella_adaln" for e in fast.low.step)
    adapter.inject()
    unet.set_context("cross_attention_block", {"clip_text_embedding": None})  # (the one-row CLIP embedding of the plain run: every token input has the latents' batch)
    _within(_run(fast, unet, adapter, t0, inp["llm"], inp["x"]), gold["unet.t0"], "after inject")
    assert fast.stats["ella_sites"] == 16 and fast.stats["step_ops"] == ella_ops


def test_table_mode_in_the_sampling_loop_matches_the_step_computed_table(gpu_device):
    """CompiledSDXL knows the solver's timesteps: ELLA's RangeEncoder and time-table GEMM run in the prologue for every (timestep, batch row) and the
    step gathers its rows.  The UNet output of a step is what CompiledUNet computes at that step's timestep with the table made in the step."""
    from refiners_amd.engine.compiled import CompiledSDXL

    unet, adapter, inp = _tree()
    pipe = CompiledSDXL(unet, num_inference_steps=10, classifier_free_guidance=False)
    pipe.set_inputs(inp["x"], clip_text_embedding=torch.zeros(2, 77, 768, device="cuda"), llm_text_embedding=inp["llm"])
    outs = []
    for s in (3, 4):
        pipe.set_inputs(inp["x"], clip_text_embedding=pipe.inputs["tokens"][("cross_attention_block", "clip_text_embedding")], llm_text_embedding=inp["llm"])
        pipe.step(s)
        outs.append(pipe.engine.io.out.clone())
    st = pipe.engine.stats
    assert st["fallback_nodes"] == [] and st["ella_sites"] == 16 and st["time_table_rows"] == 2 * 10 and pipe.engine.prologue_runs == 1
    names = [e[2] for e in pipe.engine.low.step if e[0] is not None]
    assert names.count("mi355x_gather_rows") == 2 and names.count("mi355x_sinusoidal") == 0  # the UNet's own table and ELLA's
    fast = CompiledUNet(unet)
    for s, got in zip((3, 4), outs):
        want = _run(fast, unet, adapter, float(pipe.ts_table[s]), inp["llm"], inp["x"])
        l2, mx = S.rel_err(got, want)
        print(f"table mode, step {s} (timestep {float(pipe.ts_table[s]):.0f}): l2 {l2:.2e} max {mx:.2e} against the step-computed table")
        assert l2 <= 1e-5 and mx <= 1e-5  # the same kernels on the same values; only the GEMMs' row counts (B x S against B) differ


def test_lora_on_the_cross_attention_projections_of_ellas_tokens(gpu_device, gold):
    unet, adapter, inp = _tree()
    c = E.UNET_CASE
    shapes = S.key_shapes("sd1")
    spec = synth.lora_spec(shapes, "ella_kv", c["lora_scale"], rank=c["lora_rank"], seed=3, targets=E.unet_lora_targets(shapes))
    synth.apply_adapters(unet, refiners_amd.namespace(), loras=[spec], device="cuda", dtype=torch.float32)
    fast = CompiledUNet(unet)
    y = _run(fast, unet, adapter, c["timesteps"][0], inp["llm"], inp["x"])
    _within(y, gold["unet.lora"], "unet + ella + K/V LoRA")
    assert fast.stats["fallback_nodes"] == [] and fast.stats["ella_sites"] == 16 and fast.stats["lora_sites"] == 32
    assert S.rel_err(y, gold["unet.t0"])[0] > 1e-2, "the LoRA did not move the output"
    _within(_run(fast, unet, adapter, c["timesteps"][0], inp["llm"], inp["x"]), gold["unet.lora"], "unet + ella + K/V LoRA (graph replay)")


def test_bfloat16_step_beats_the_unfused_chain(gpu_device, gold):
    unet, adapter, inp = _tree(torch.bfloat16)
    t0 = E.UNET_CASE["timesteps"][0]
    fast = CompiledUNet(unet)
    y = _run(fast, unet, adapter, t0, inp["llm"], inp["x"])
    assert fast.stats["fallback_nodes"] == [] and fast.stats["ella_sites"] == 16
    adapter.set_llm_text_embedding(inp["llm"])
    unet.set_timestep(E.timestep(t0).cuda())
    with torch.no_grad():
        chain = unet(inp["x"])
    mine, stock = S.rel_err(y, gold["unet.t0"]), S.rel_err(chain, gold["unet.t0"])
    print(f"bf16 against the float32 reference: lowered l2 {mine[0]:.3e} max {mine[1]:.3e} | unfused Chain l2 {stock[0]:.3e} max {stock[1]:.3e}")
    assert torch.isfinite(y.float()).all() and mine[0] < stock[0]


@pytest.mark.skipif(REF is None, reason="no refiners checkout (REFINERS_SRC / oracle/_ref)")
def test_reference_tree_with_its_own_adapter(gpu_device, gold):
    sys.path[:0] = [p for p in (str(ROOT / "oracle" / "shim"), str(REF)) if p not in sys.path]
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.ella_adapter import SD1ELLAAdapter as RefAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet as RefUNet

    c = E.UNET_CASE
    unet = RefUNet(4, device="meta")
    unet.load_state_dict({k: v.cuda() for k, v in S.weights("sd1", c["unet_weight_seed"]).items()}, assign=True)
    adapter = RefAdapter(unet)
    adapter.latents_encoder.load_state_dict({k: v.cuda() for k, v in E.weights("sd1_full").items()}, assign=True)
    adapter.inject()
    assert type(unet).__module__.startswith("refiners.")
    inp = {k: v.cuda() for k, v in E.unet_inputs().items()}
    fast = CompiledUNet(unet)
    for i, ts in enumerate(c["timesteps"]):
        y = _run(fast, unet, SimpleNamespace(set_llm_text_embedding=adapter.set_llm_text_embedding), ts, inp["llm"], inp["x"])
        _within(y, gold[f"unet.t{i}"], f"refiners' own tree + SD1ELLAAdapter t{i}")
    assert fast.stats["fallback_nodes"] == [] and fast.stats["ella_sites"] == 16 and fast.prologue_runs == 1
