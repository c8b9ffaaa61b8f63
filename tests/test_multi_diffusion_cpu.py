"""MultiDiffusion, host side (CPU): the mirror (refiners_amd/latent_diffusion/multi_diffusion.py) against the REAL reference
(tests/golden/multi_diffusion.safetensors and multi_diffusion_tiles.json, tools/make_golden_multi_diffusion.py), the torch model of the three
kernels against the mirror bit for bit, the engine's chunk plan and graph key, its host logic over the modelled kernels, and what the engine refuses.  The kernels and the engine are
checked on the GPU in tests/test_multi_diffusion_kernels_gpu.py and tests/test_multi_diffusion_gpu.py."""
import json
from functools import lru_cache

import pytest
import torch

import refiners_amd
import refiners_amd.fluxion.layers as fl
from refiners_amd.engine.multi_diffusion import CompiledMultiDiffusion, chunk_plan, graph_key
from refiners_amd.engine.packing import Unsupported
from refiners_amd.latent_diffusion import multi_diffusion as M
from refiners_amd.latent_diffusion.sampling import DDIM, SDXLDenoiser
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from refiners_amd.latent_diffusion.sdxl import SDXLUNet
from refiners_amd.latent_diffusion.solvers import LCMSolver
from tests import support as S
from tests.multi_diffusion_cases import (MD_CASES, STEPS, TILE_RECIPES, blend_model, build_targets, canvas_inputs, gather_model, mirror_namespace, mirror_solver, model_call,
                                         target_step_model)
from tests.test_lowering_cpu import _dry

TOL = 2e-4  # mirror against reference, the bar of tests/test_mirror_golden.py


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from refiners_amd.build_native import build_native

    build_native()


@lru_cache(maxsize=None)
def _unet(family: str):
    unet = (SDXLUNet if family == "sdxl" else SD1UNet)(4, device="meta")
    S.load_mirror_weights(unet, S.weights(family, 0))
    return unet


def test_namespace_exports_the_mirrored_classes():
    ns = refiners_amd.namespace()
    for name in ("Tile", "Size", "DiffusionTarget", "MultiDiffusion", "SDXLTarget", "SDXLMultiDiffusion", "SD1DiffusionTarget", "SD1MultiDiffusion"):
        assert getattr(ns, name) is getattr(M, name)


def test_generate_latent_tiles_equals_the_recorded_lists():
    recorded = json.loads((S.GOLD / "multi_diffusion_tiles.json").read_text())
    assert [(*r["size"], *r["tile_size"], r["min_overlap"]) for r in recorded] == [tuple(r) for r in TILE_RECIPES]
    for r in recorded:
        got = M.MultiDiffusion.generate_latent_tiles(M.Size(*r["size"]), M.Size(*r["tile_size"]), min_overlap=r["min_overlap"])
        assert [list(t) for t in got] == r["tiles"] and all(isinstance(t, M.Tile) for t in got)
    clamped = next(r for r in recorded if r["size"] == [16, 41])["tiles"]
    assert [t[1] for t in clamped] == [0, 9, 18, 25]  # the last tile is moved back inside: the clamp branch
    with pytest.raises(AssertionError, match="Overlap"):
        M.MultiDiffusion.generate_latent_tiles(M.Size(32, 32), M.Size(16, 16), min_overlap=16)


def test_target_crop_paste_size_offset():
    t = M.DiffusionTarget(tile=M.Tile(top=2, left=3, bottom=7, right=11), solver=None)
    x = torch.arange(2 * 4 * 9 * 13, dtype=torch.float32).view(2, 4, 9, 13)
    assert t.size == M.Size(5, 8) and t.offset == (2, 3) and torch.equal(t.crop(x), x[:, :, 2:7, 3:11])
    y = t.paste(torch.zeros_like(x), crop=t.crop(x))
    assert torch.equal(y[:, :, 2:7, 3:11], x[:, :, 2:7, 3:11]) and y.sum() == x[:, :, 2:7, 3:11].sum()
    assert (t.weight, t.start_step, t.end_step, t.init_latents, t.opacity_mask) == (1, 0, M.MAX_STEPS, None, None)


@pytest.mark.parametrize("name", list(MD_CASES))
def test_mirror_call_matches_reference(name):
    case = MD_CASES[name]
    gold = S.golden("multi_diffusion")
    unet = _unet(case["family"])
    targets = build_targets(case, mirror_namespace(), mirror_solver)
    keep = DDIM(STEPS)
    if case["family"] == "sdxl":
        sd = SDXLDenoiser(unet, keep)
        md = M.SDXLMultiDiffusion(sd)
    else:
        sd = M.SD1Denoiser(unet, keep)
        md = M.SD1MultiDiffusion(sd)
    seen = {}
    inner = md.diffuse_target

    def record(x, step, target):
        y = inner(x=x, step=step, target=target)
        seen[(next(i for i, t in enumerate(targets) if t is target), step)] = y
        return y

    md.diffuse_target = record
    x, noise = canvas_inputs(case)
    x_in = x.clone()
    with torch.no_grad():
        for s in case["steps"]:
            x = md(x, noise=noise, step=s, targets=targets)
            l2, mx = S.rel_err(x, gold[f"{name}.canvas{s}"])
            print(f"{name} canvas{s}: l2 {l2:.2e} max {mx:.2e}")
            assert l2 < TOL and mx < TOL, (name, s, l2, mx)
    assert sd.solver is keep  # diffuse_target puts the denoiser's own solver back
    assert sorted(f"{name}.target{i}.step{s}" for i, s in seen) == sorted(k for k in gold if k.startswith(f"{name}.target"))
    for (i, s), y in seen.items():
        assert S.rel_err(y, gold[f"{name}.target{i}.step{s}"])[0] < TOL
    if name == "a":
        # the overlap really mixes targets: rows 8..15 x columns 11..15 lie under all four, and there the canvas is none of the four results
        g = gold["a.canvas11"]
        parts = [gold[f"a.target{i}.step11"] for i in range(4)]
        crops = [parts[0][:, :, 8:16, 11:16], parts[1][:, :, 8:16, 0:5], parts[2][:, :, 0:8, 11:16], parts[3][:, :, 0:8, 0:5]]
        assert min(S.rel_err(g[:, :, 8:16, 11:16], c)[0] for c in crops) > 5e-2
        mean = (crops[0] + 2 * crops[1] + crops[2] + crops[3]) / 5  # target 1 weighs 2
        assert S.rel_err(g[:, :, 8:16, 11:16], mean)[0] < 1e-5
        assert torch.equal(g[:, :, :8, :11], parts[0][:, :, :8, :11])  # covered once: cumulative / 1
    if name == "b":
        g = gold["b.canvas11"]
        assert torch.equal(g[:, :, 16:, :11], x_in[:, :, 16:, :11])  # uncovered: x
        assert torch.equal(g[:, :, 4:10, 3:9], x_in[:, :, 4:10, 3:9])  # num_updates == 0 inside a tile: x
        assert not torch.equal(g[:, :, :4, :11], x_in[:, :, :4, :11]) and (2, 11) not in seen


def _fake_diffuse(view, step, target):
    return view * 0.8125 + target.condition_scale * 0.03125 * view.flip(-1) + 0.001 * step  # deterministic, elementwise torch ops


@pytest.mark.parametrize("name", list(MD_CASES))
def test_kernel_model_equals_the_mirror_bit_for_bit(name):
    case = MD_CASES[name]
    targets = build_targets(case, mirror_namespace(), mirror_solver)

    class Fake(M.MultiDiffusion):
        def diffuse_target(self, x, step, target):
            return _fake_diffuse(x, step, target)

    x, noise = canvas_inputs(case)
    xm = x.clone()
    for s in case["steps"]:
        x = Fake()(x, noise=noise, step=s, targets=targets)
        xm = model_call(xm, noise, s, targets, _fake_diffuse)
        assert torch.equal(x, xm), (name, s, float((x - xm).abs().max()))


def test_kernel_model_mask_broadcast_shapes_and_many_targets():
    g = torch.Generator().manual_seed(5)
    x, noise = torch.randn(1, 4, 8, 9, generator=g), torch.randn(1, 4, 8, 9, generator=g)
    targets = []
    for k in range(64):
        top, left = k % 5, (3 * k) % 6
        mask = [None, torch.rand(4, 4, generator=g), torch.rand(1, 1, 4, 4, generator=g), torch.rand(1, 4, 4, 4, generator=g)][k % 4]
        targets.append(M.SD1DiffusionTarget(tile=M.Tile(top, left, top + 4, left + 4), solver=mirror_solver("ddim", 0), opacity_mask=mask, weight=1 + k % 3,
                                            clip_text_embedding=torch.zeros(2, 1, 1), condition_scale=float(k)))

    class Fake(M.MultiDiffusion):
        def diffuse_target(self, x, step, target):
            return _fake_diffuse(x, step, target)

    assert torch.equal(Fake()(x, noise=noise, step=3, targets=targets), model_call(x, noise, 3, targets, _fake_diffuse))


# ------------------------------------------------------------------------------------------------ the engine's plan
def test_chunk_plan_of_case_a_and_b_and_the_graph_key():
    ta = build_targets(MD_CASES["a"], mirror_namespace(), mirror_solver)
    for tile_batch, want in ((4, [(0, 1, 2, 3)]), (2, [(0, 1), (2, 3)]), (1, [(0,), (1,), (2,), (3,)]), (3, [(0, 1, 2), (3,)])):
        chunks, skipped = chunk_plan(11, ta, tile_batch)
        assert [c.indices for c in chunks] == want and skipped == [] and {c.size for c in chunks} == {(16, 16)} and not any(c.linear for c in chunks)
        assert {c.timestep for c in chunks} == {float(DDIM(STEPS).timesteps[11])}
    tb = build_targets(MD_CASES["b"], mirror_namespace(), mirror_solver)
    chunks, skipped = chunk_plan(11, tb, 4)
    assert [(c.indices, c.size) for c in chunks] == [((0, 1), (16, 16)), ((3,), (24, 16))] and skipped == [2]
    # the key moves exactly when the active set does: steps 5..10 share one (target 1 has not started), 11 adds target 1 and drops target 2, 12 equals 11
    keys = {s: graph_key(chunk_plan(s, tb, 4)[0], tb) for s in (5, 10, 11, 12, 29)}
    assert keys[5] == keys[10] and keys[11] == keys[12] == keys[29] and keys[10] != keys[11]
    assert [c.indices for c in chunk_plan(10, tb, 4)[0]] == [(0, 2), (3,)]
    # another tile_batch is another chunking and another key; another target object as well
    assert graph_key(chunk_plan(11, ta, 2)[0], ta) != graph_key(chunk_plan(11, ta, 4)[0], ta)
    other = build_targets(MD_CASES["a"], mirror_namespace(), mirror_solver)
    assert graph_key(chunk_plan(11, other, 4)[0], other) != graph_key(chunk_plan(11, ta, 4)[0], ta)
    # case d: one DDIM target and one DPM target are two timesteps and two update forms
    td = build_targets(MD_CASES["d"], mirror_namespace(), mirror_solver)
    assert [(c.indices, c.linear) for c in chunk_plan(11, td, 4)[0]] == [((0,), False), ((1,), True)]
    # a target with init latents takes part on its start step even when its window is empty (multi_diffusion.py:104)
    tb[1].end_step = 3
    assert [c.indices for c in chunk_plan(11, tb, 4)[0]][0] == (0, 1) and 1 in chunk_plan(12, tb, 4)[1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_chunk_of_case_a_and_b_lowers_without_fallback(dtype):
    """The UNet program of every chunk geometry the plans of cases a and b ask for (batch 2T of 16 x 16 and 24 x 16 tiles), dry on the meta device."""
    unet = SDXLUNet(4, device="meta", dtype=dtype)
    tokens = {("cross_attention_block", "clip_text_embedding"): (77, 2048)}
    shapes = set()
    for name in ("a", "b"):
        targets = build_targets(MD_CASES[name], mirror_namespace(), mirror_solver)
        for tile_batch in (1, 2, 4):
            shapes |= {(2 * len(c.indices), *c.size) for c in chunk_plan(11, targets, tile_batch)[0]}
    assert shapes == {(2, 16, 16), (4, 16, 16), (8, 16, 16), (2, 24, 16)}
    for B, h, w in sorted(shapes):
        low = _dry(unet, B, h, w, dtype, tokens)
        assert low.stats["fallback_nodes"] == [] and len(low.step) > 100


# ------------------------------------------------------------------------------------------------ the engine's host logic, kernels replaced by their models
def _toy_unet(x, text, timestep):
    return 0.5 * x + 0.01 * text.float().mean(dim=(1, 2)).view(-1, 1, 1, 1) + 1e-4 * float(timestep) + 0.1 * x.flip(-1)


class _ToyUNet:
    """Stands where the UNet tree stands for the denoisers of the mirror: context setters and a call."""

    dtype, device, parent = torch.float32, torch.device("cpu"), None

    def set_timestep(self, timestep):
        self.t = timestep

    def set_clip_text_embedding(self, clip_text_embedding):
        self.text = clip_text_embedding

    def set_pooled_text_embedding(self, pooled_text_embedding):
        pass

    def set_time_ids(self, time_ids):
        pass

    def get_parents(self):
        return []

    def __call__(self, x):
        return _toy_unet(x, self.text, self.t)


class _ToyEngine:
    """CompiledUNet's surface as CompiledMultiDiffusion uses it: static io buffers per geometry, a one-entry step program, a prologue flag per prompt."""

    CHECK_EVERY = 16

    def __init__(self, unet, use_graph=False, lora_mode="fused"):
        self.unet, self.lora_mode, self.cache, self.io, self.low, self.key, self.io_override, self.prologues, self.pk = unet, lora_mode, object(), None, None, None, None, 0, None

    def prepare_explicit(self, shape, dev, got):
        from types import SimpleNamespace

        if self.io is None or tuple(self.io.x.shape) != tuple(shape):
            self.io, self.pk = SimpleNamespace(x=torch.zeros(shape), out=torch.zeros(shape)), None
            self.key = ("toy", tuple(shape), id(self.io))
        self.got, io = got, self.io
        assert got["tokens"][("cross_attention_block", "clip_text_embedding")].shape[0] == shape[0] and (got["pooled"] is None or got["pooled"].shape[0] == shape[0])
        self.low = SimpleNamespace(step=[(None, lambda: io.out.copy_(_toy_unet(io.x, self.got["tokens"][("cross_attention_block", "clip_text_embedding")], self.got["timestep"])), "toy", ())])
        pk = tuple(id(v) for v in got["tokens"].values()) + (id(got["pooled"]), id(got["timesteps_all"]))
        changed, self.pk = pk != self.pk, pk
        return changed

    def run_prologue(self):
        self.prologues += 1

    def check_handovers(self, every=1):
        pass


@pytest.fixture
def modelled_kernels(monkeypatch):
    """native.md_* replaced by the torch models, reading the SAME descriptor bytes the kernels would be handed; CompiledUNet replaced by the toy engine."""
    import ctypes

    from refiners_amd import native
    from refiners_amd.engine import multi_diffusion as E

    masks, real_rows = {}, native.md_blend_rows

    def structs(t, cls):
        return (cls * (t.numel() // ctypes.sizeof(cls))).from_buffer_copy(t.contiguous().numpy().tobytes())

    def blend_rows(rows):
        masks.update({r[6].data_ptr(): r[6] for r in rows if r[6] is not None})
        return real_rows(rows)

    def gather(canvas, noise, init, desc, desc_host, view, model_in):
        assert torch.equal(desc, desc_host)
        rows = [(d.kind, d.top, d.left, d.init_row, d.a, d.b, d.s) for d in structs(desc_host, native.MdGatherDesc)][: view.shape[0]]
        v, m = gather_model(canvas, noise, init, rows, view.shape[2], view.shape[3])
        view.copy_(v), model_in.copy_(m)

    def target_step(view, unet_out, stepped, hist, coef, linear):
        s, h = target_step_model(view, unet_out, hist, coef, linear)
        stepped.copy_(s)
        if linear:
            hist.copy_(h)

    def blend(canvas, stepped, desc, desc_host, n):
        assert torch.equal(desc, desc_host)
        rows = [(d.top, d.left, d.h, d.w, d.weight, d.stepped_off, masks[d.mask] if d.mask else None) for d in structs(desc_host, native.MdBlendDesc)][:n]
        return canvas.copy_(blend_model(canvas, stepped, rows))

    for name, fn in (("md_gather", gather), ("md_target_step", target_step), ("md_blend", blend), ("md_blend_rows", blend_rows), ("stream_ptr", lambda: 0)):
        monkeypatch.setattr(native, name, fn)
    monkeypatch.setattr(E, "CompiledUNet", _ToyEngine)


@pytest.mark.parametrize("tile_batch", [1, 2, 4])
@pytest.mark.parametrize("name", list(MD_CASES))
def test_engine_host_logic_over_modelled_kernels_equals_the_mirror(modelled_kernels, name, tile_batch):
    """Everything of CompiledMultiDiffusion that is not a kernel -- plan, buffers, descriptor and coefficient rows, [negatives ; conditionals] stacks, history that moves with
    its target when the chunking changes, resident canvas -- against the mirror over the same toy UNet.  Case b runs steps 10, 11, 12: the active set changes, then stays.
    float32 with the step model in float64: 1e-5 absolute on values of order 1."""
    case = MD_CASES[name]
    unet = _ToyUNet()
    md = CompiledMultiDiffusion(unet, tile_batch=tile_batch, use_graph=False)
    targets, ref_targets = (build_targets(case, mirror_namespace(), mirror_solver) for _ in range(2))
    den = (SDXLDenoiser if case["family"] == "sdxl" else M.SD1Denoiser)(unet, DDIM(STEPS))
    ref = (M.SDXLMultiDiffusion if case["family"] == "sdxl" else M.SD1MultiDiffusion)(den)
    x, noise = canvas_inputs(case)
    xr = x.clone()
    for s in case["steps"] if name != "b" else [10, 11, 12]:
        x = md(x, noise=noise, step=s, targets=targets)
        xr = ref(xr, noise=noise, step=s, targets=ref_targets)
        assert x is md.canvas and float((x - xr).abs().max()) < 1e-5, (name, s, float((x - xr).abs().max()))
        assert max(len(c[0]) for c in md.stats["chunks"]) <= tile_batch
    assert all(e.prologues <= (2 if name == "b" else 1) for e in md.engines)  # the stacks are rebuilt only when the chunk's targets change


# ------------------------------------------------------------------------------------------------ refusals
def test_engine_refuses_what_it_does_not_batch():
    unet = SDXLUNet(4, device="meta")
    md = CompiledMultiDiffusion(unet)
    targets = build_targets(MD_CASES["a"], mirror_namespace(), mirror_solver)
    x = torch.zeros(1, 4, 24, 27)
    md.check(x, targets, 11)  # the supported call passes
    with pytest.raises(Unsupported, match="canvas batch"):
        md.check(torch.zeros(2, 4, 24, 27), targets, 11)
    lcm = build_targets(MD_CASES["a"], mirror_namespace(), lambda kind, first: LCMSolver(4))
    with pytest.raises(Unsupported, match="draws noise per step"):
        md.check(x, lcm, 1)
    with pytest.raises(Unsupported, match="draws noise per step"):
        chunk_plan(1, lcm, 4)
    many = [targets[0]] * 65
    with pytest.raises(Unsupported, match="more than 64 active targets"):
        md.check(x, many, 11)
    from refiners_amd.latent_diffusion.sag import SDXLSAGAdapter

    sag = SDXLSAGAdapter(unet, scale=0.75).inject()
    with pytest.raises(Unsupported, match="Self-Attention Guidance"):
        md.check(x, targets, 11)
    sag.eject()
    md.check(x, targets, 11)


def test_a_tree_the_lowering_refuses_is_refused_at_the_chunk_geometry():
    """The fourth refusal comes from the lowering itself: a node that reads the Chain's context store at run time (tests/test_lowering_cpu.py) raises
    Unsupported at a chunk's geometry like at any other; CompiledMultiDiffusion then takes the host loop (tests/test_multi_diffusion_gpu.py)."""
    from refiners_amd.latent_diffusion.blocks import ResidualConcatenator

    class SkipFilter(fl.Concatenate):
        def __init__(self, n: int) -> None:
            super().__init__(fl.Identity(), fl.Chain(fl.UseContext(context="unet", key="residuals").compose(lambda r: r[n]), fl.Lambda(lambda t: t * 0.5)), dim=1)

    unet = SDXLUNet(4, device="meta")
    block = unet.layer(("UpBlocks", 0), fl.Chain)
    block.replace(block.ensure_find(ResidualConcatenator), SkipFilter(-2))
    with pytest.raises(Unsupported, match="SkipFilter.*UseContext"):
        _dry(unet, 8, 16, 16, torch.float32, {("cross_attention_block", "clip_text_embedding"): (77, 2048)})
