"""pytest -m gpu: CompiledMultiDiffusion on the MI355X against the REAL reference's goldens (tests/golden/multi_diffusion.safetensors, written by
tools/make_golden_multi_diffusion.py from refiners' SDXLMultiDiffusion / SD1MultiDiffusion on CPU float32).

Bounds: float32 at the project's float32 bar (F32_TOL of tests/test_engine_gpu.py) on both figures of tests/support.rel_err.  bf16: the canvas is a
weighted mean of tiles that each went through one bf16 CFG step, so its error against the float32 golden is bounded by the worst tile's plus the
blend's own rounding; the test measures one tile's error with a plain CompiledSDXL.step in bf16 and allows twice that for the tile-to-tile spread."""
import os
import sys
import warnings
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

import refiners_amd.fluxion.layers as fl
from refiners_amd import native
from refiners_amd.engine.compiled import CompiledSDXL
from refiners_amd.engine.multi_diffusion import CompiledMultiDiffusion
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from refiners_amd.latent_diffusion.sdxl import SDXLUNet
from tests import support as S
from tests.multi_diffusion_cases import MD_CASES, STEPS, build_targets, canvas_inputs, mirror_namespace, mirror_solver

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_TOL = 1e-3
ROOT = Path(__file__).resolve().parent.parent
REF = next((Path(c) for c in (os.environ.get("REFINERS_SRC"), ROOT / "oracle" / "_ref" / "src") if c and (Path(c) / "refiners").exists()), Path("/nonexistent"))


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


def _unet(family, dtype):
    unet = (SDXLUNet if family == "sdxl" else SD1UNet)(4, device="meta")
    S.load_mirror_weights(unet, S.weights(family, 0), device=DEV, dtype=dtype)
    return unet


@pytest.fixture(scope="module")
def sdxl_f32():
    """One float32 SDXL UNet and ONE engine over it for the whole module: tests change `tile_batch` on it, the packed weights are shared."""
    unet = _unet("sdxl", torch.float32)
    return unet, CompiledMultiDiffusion(unet)


@pytest.fixture(scope="module")
def gold():
    return S.golden("multi_diffusion")


def _targets(name, ns=None, make_solver=mirror_solver, dtype=torch.float32):
    return build_targets(MD_CASES[name], ns or mirror_namespace(), make_solver, device=DEV, dtype=dtype)


def _run(md, name, targets, gold, tol=F32_TOL):
    case = MD_CASES[name]
    x, noise = (t.to(DEV) for t in canvas_inputs(case))
    for s in case["steps"]:
        x = md(x, noise=noise, step=s, targets=targets)
        l2, mx = S.rel_err(x, gold[f"{name}.canvas{s}"])
        print(f"{name} canvas{s} tile_batch={md.tile_batch}: l2 {l2:.2e} max {mx:.2e} {md.stats}")
        assert l2 < tol and mx < tol, (name, s, l2, mx)
    return x


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_sdxl_cases_match_reference(sdxl_f32, gold, name):
    _, md = sdxl_f32
    md.tile_batch = 4
    targets = _targets(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # the native path, not the host loop
        x = _run(md, name, targets, gold)  # case c: two consecutive calls, the second on the canvas the first returned
    assert "whole_fallback" not in md.stats and x is md.canvas
    want = {"a": [((0, 1, 2, 3), (16, 16), False)], "b": [((0, 1), (16, 16), False), ((3,), (24, 16), False)], "c": [((0, 1), (16, 16), True)]}[name]
    assert md.stats["chunks"] == want and md.stats["skipped"] == ([2] if name == "b" else [])
    if name == "c":
        assert md.stats["graph_replayed"]  # step 1 replays the graph step 0 captured: same active set, other coefficients and timestep
        # the history is per target: without it step 1 would be a second-order update on zeros
        for _, h in md.hist_of.values():
            assert float(h.abs().max()) > 0


def test_sd1_case_matches_reference(gold):
    md = CompiledMultiDiffusion(_unet("sd1", torch.float32))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        _run(md, "d", _targets("d"), gold)
    assert md.stats["chunks"] == [((0,), (16, 16), False), ((1,), (16, 16), True)] and len(md.engines) == 2


@pytest.mark.parametrize("tile_batch", [1, 2, 4])
@pytest.mark.parametrize("name", ["a", "b"])
def test_tile_batch_gives_the_same_canvas(sdxl_f32, gold, name, tile_batch):
    _, md = sdxl_f32
    md.tile_batch = tile_batch
    try:
        _run(md, name, _targets(name), gold)
        assert max(len(c[0]) for c in md.stats["chunks"]) <= tile_batch
        if name == "a":
            assert len(md.stats["chunks"]) == 4 // tile_batch
    finally:
        md.tile_batch = 4


def test_replay_of_an_unchanged_step_is_bit_equal(sdxl_f32, gold):
    _, md = sdxl_f32
    md.tile_batch = 4
    targets = _targets("b")
    x0, noise = (t.to(DEV) for t in canvas_inputs(MD_CASES["b"]))
    first = md(x0.clone(), noise=noise, step=11, targets=targets).clone()
    assert not md.stats["graph_replayed"]  # new target objects: captured
    again = md(x0.clone(), noise=noise, step=11, targets=targets).clone()
    assert md.stats["graph_replayed"] and torch.equal(first, again)
    md(x0.clone(), noise=noise, step=12, targets=targets)
    assert md.stats["graph_replayed"]  # target 1 went from its noised init latents to the canvas crop: the same graph, another descriptor
    md(x0.clone(), noise=noise, step=10, targets=targets)
    assert not md.stats["graph_replayed"] and md.stats["skipped"] == [1]  # another active set
    third = md(x0.clone(), noise=noise, step=11, targets=targets)
    assert torch.equal(first, third) and S.rel_err(third, gold["b.canvas11"])[0] < F32_TOL
    direct = CompiledMultiDiffusion(md.unet, use_graph=False)
    direct.engine.cache = md.engine.cache
    assert torch.equal(direct(x0.clone(), noise=noise, step=11, targets=targets), first)  # the captured graph and the direct launches: the same bits


@pytest.mark.skipif(not (REF / "refiners").exists(), reason="no refiners checkout (REFINERS_SRC / oracle/_ref)")
def test_reference_target_classes_are_accepted(sdxl_f32, gold):
    sys.path[:0] = [p for p in (str(ROOT / "oracle" / "shim"), str(REF)) if p not in sys.path]
    from refiners.foundationals.latent_diffusion.multi_diffusion import Tile
    from refiners.foundationals.latent_diffusion.solvers import DDIM as RefDDIM
    from refiners.foundationals.latent_diffusion.solvers import DPMSolver as RefDPM
    from refiners.foundationals.latent_diffusion.stable_diffusion_xl.multi_diffusion import SDXLTarget

    _, md = sdxl_f32
    md.tile_batch = 4
    ns = SimpleNamespace(Tile=Tile, SDXLTarget=SDXLTarget)
    make = lambda kind, first: (RefDDIM if kind == "ddim" else RefDPM)(num_inference_steps=STEPS, first_inference_step=first)  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for name in ("b", "c"):
            _run(md, name, _targets(name, ns, make), gold)


def test_refused_tree_warns_and_the_host_loop_matches_reference(sdxl_f32, gold):
    """A node the lowering does not know that reads the context store at run time (numerically the ResidualConcatenator it replaces): Unsupported at
    the first chunk, a RuntimeWarning, the mirror's loop over the stock forward -- and the same canvas."""
    from refiners_amd.latent_diffusion.blocks import ResidualConcatenator

    class OtherConcatenator(fl.Chain):
        def __init__(self, n: int) -> None:
            super().__init__(fl.Concatenate(fl.Identity(), fl.UseContext(context="unet", key="residuals").compose(lambda r: r[n]), dim=1))

    unet, _ = sdxl_f32
    md = CompiledMultiDiffusion(unet)
    md.engine.cache = sdxl_f32[1].engine.cache
    block = unet.layer(("UpBlocks", 0), fl.Chain)
    original = block.ensure_find(ResidualConcatenator)
    other = OtherConcatenator(original.n)
    block.replace(original, other)
    try:
        targets = _targets("b", make_solver=lambda k, f: mirror_solver(k, f, device=DEV))
        with pytest.warns(RuntimeWarning, match="host loop over the stock Chain forward"):
            _run(md, "b", targets, gold)
        assert "OtherConcatenator" in md.stats["whole_fallback"]
    finally:
        block.replace(other, original)
    # a refusal the engine makes itself: a canvas batch of 2 is two independent canvases for the host loop
    md2 = CompiledMultiDiffusion(unet)
    md2.engine.cache = sdxl_f32[1].engine.cache
    x, noise = (t.to(DEV) for t in canvas_inputs(MD_CASES["a"]))
    targets = _targets("a", make_solver=lambda k, f: mirror_solver(k, f, device=DEV))
    for t in targets:  # (the host loop's UNet call sees cat(x, x) of a batch of 2: four rows of embeddings)
        t.clip_text_embedding = t.clip_text_embedding.repeat_interleave(2, 0)
        t.pooled_text_embedding = t.pooled_text_embedding.repeat_interleave(2, 0)
        t.time_ids = t.time_ids.repeat_interleave(2, 0)
    with pytest.warns(RuntimeWarning, match="canvas batch of 2"):
        y = md2(torch.cat((x, x)), noise=torch.cat((noise, noise)), step=11, targets=targets)
    assert S.rel_err(y[:1], gold["a.canvas11"])[0] < F32_TOL and S.rel_err(y[1:], gold["a.canvas11"])[0] < F32_TOL


def test_bf16_canvas_error_is_bounded_by_a_single_tiles(gold):
    """Both figures are relative l2 errors against the float32 goldens; what the MI355X gave is recorded in DESIGN.md."""
    unet = _unet("sdxl", torch.bfloat16)
    case = MD_CASES["a"]
    targets = _targets("a", dtype=torch.bfloat16)
    x, noise = (t.to(DEV) for t in canvas_inputs(case))
    md = CompiledMultiDiffusion(unet)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = md(x, noise=noise, step=11, targets=targets)
    canvas_err = S.rel_err(y.float(), gold["a.canvas11"])[0]
    t0 = targets[0]
    sd = CompiledSDXL(unet, num_inference_steps=STEPS, condition_scale=t0.condition_scale)
    sd.engine.cache = md.engine.cache
    sd.set_inputs(t0.crop(x), clip_text_embedding=t0.clip_text_embedding, pooled_text_embedding=t0.pooled_text_embedding, time_ids=t0.time_ids)
    tile_err = S.rel_err(sd.step(11).float(), gold["a.target0.step11"])[0]
    print(f"bf16 case a: canvas l2 {canvas_err:.3e}, single tile (CompiledSDXL.step) l2 {tile_err:.3e}")
    assert canvas_err <= 2 * tile_err, (canvas_err, tile_err)
