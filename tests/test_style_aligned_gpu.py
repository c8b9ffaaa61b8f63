"""pytest -m gpu: StyleAligned shared self-attention on the MI355X -- the two kernels (mi355x_adain_stats, mi355x_style_aligned_pack) against
float32 torch, and the lowered UNet / CFG step with `StyleAlignedAdapter` injected against the REAL reference's goldens
(tests/golden/sdxl_style_aligned.safetensors) and against the unfused mirror on the GPU.

Kernel bounds are those of tests/test_sam_decoder_gpu.py, with its reasoning: float32 1e-5 relative l2 (float32 arithmetic on the same
inputs, a few roundings apart); bf16 2^-8 (a float32 result rounded once to 8 significant bits, <= 2^-9 per element, against a reference
computed from the same rounded inputs).  Engine bounds are those of tests/test_engine_gpu.py (F32_TOL, the bf16 rule)."""
import warnings

import pytest
import torch

import refiners_amd
from refiners_amd import native
from refiners_amd.engine.compiled import CompiledSDXL, CompiledUNet
from refiners_amd.latent_diffusion.sampling import DDIM
from refiners_amd.latent_diffusion.sdxl import SDXLUNet
from refiners_amd.latent_diffusion.style_aligned import StyleAlignedAdapter
from tests import support as S
from tests.style_aligned_cases import STYLE_ALIGNED_CASES, case_inputs, case_specs, pack_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
KTOL = {torch.float32: 1e-5, torch.bfloat16: 2.0**-8}
F32_TOL = 1e-3
BF16_TOL = 3e-2


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    native.load()


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
def _run_kernels(q, k, vt, n, scale, L, C, packed=None):
    """q, k: [B, L, C] views, vt: [C, B, Lp] view -> (stats q, stats k, q', k_sh, vt_sh) through the two native entry points."""
    B = q.shape[0]
    f32 = dict(device=DEV, dtype=torch.float32)
    if packed is not None:  # ONE statistics launch over the packed Q|K buffer, the two halves of its table handed to the pack kernel
        st = torch.empty(B, 2 * C, 2, **f32)
        need = native.adain_stats_ws_floats(B, L, 2 * C)
        native.adain_stats(packed, st, torch.empty(max(need, 1), **f32))
        sq, sk = st[:, :C], st[:, C:]
    else:
        need = native.adain_stats_ws_floats(B, L, C)
        ws = torch.empty(max(need, 1), **f32)
        sq, sk = native.adain_stats(q, torch.empty(B, C, 2, **f32), ws), native.adain_stats(k, torch.empty(B, C, 2, **f32), ws)
    lkp = (2 * L + 63) // 64 * 64
    k_sh, vt_sh = torch.zeros(B, lkp, C, device=DEV, dtype=q.dtype), torch.zeros(C, B, lkp, device=DEV, dtype=q.dtype)
    native.style_aligned_pack(q, k, vt, sq, sk, n, torch.tensor([scale], **f32), 1e-8, k_sh, vt_sh)
    return sq, sk, q, k_sh, vt_sh


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [640, 1280])
@pytest.mark.parametrize("L", [60, 64, 1024, 4096])
def test_kernels_match_float32_torch(L, C, dtype):
    B, n, scale = 6, 3, 0.6
    g = torch.Generator(device=DEV).manual_seed(L + C)
    # channel-dependent offsets and spreads, so that a wrong channel / sample / reference row shows
    mk = lambda: (torch.randn(B, L, C, device=DEV, generator=g) * (0.5 + torch.rand(B, 1, C, device=DEV, generator=g)) + torch.randn(B, 1, C, device=DEV, generator=g)).to(dtype)  # noqa: E731
    q0, k0, v0 = mk(), mk(), mk()
    lp = (L + 63) // 64 * 64
    vt = torch.zeros(C, B, lp, device=DEV, dtype=dtype)
    vt[:, :, :L] = v0.permute(2, 0, 1)
    # the packed [M, 2C] Q|K buffer of the merged projection launch: q and k are strided column slices of it
    qk = torch.cat((q0, k0), dim=2).contiguous()
    q, k = qk[:, :, :C], qk[:, :, C:]
    sq, sk, q1, k_sh, vt_sh = _run_kernels(q, k, vt[:, :, :L] if lp == L else vt, n, scale, L, C, packed=qk.clone())
    rq, rk, rvt = pack_model(q0.float(), k0.float(), v0.float(), n, scale)
    for name, t in (("q", q0), ("k", k0)):
        std, mean = torch.std_mean(t.float(), dim=1)
        got = sq if name == "q" else sk
        e_mean, e_std = _rel(got[..., 0], mean), _rel(got[..., 1], std)
        print(f"L {L} C {C} {dtype}: {name} mean {e_mean:.2e} std {e_std:.2e}")
        assert e_mean < 1e-5 and e_std < 1e-5  # statistics are float32 whatever the storage type
    errs = {"q'": _rel(q1.float(), rq), "k_sh": _rel(k_sh.float(), rk), "vt_sh": _rel(vt_sh.float(), rvt)}
    print(f"L {L} C {C} {dtype}: " + " ".join(f"{k_} {v:.2e}" for k_, v in errs.items()))
    assert all(v < KTOL[dtype] for v in errs.values()), errs
    assert not k_sh[:, 2 * L :].any() and not vt_sh[:, :, 2 * L :].any()  # the padding is the caller's: never written
    # the reference rows' own copies and every V^T column are moved, not recomputed
    assert torch.equal(k_sh[0::n, L : 2 * L], k0[0::n]) and torch.equal(vt_sh[:, :, :L], v0.permute(2, 0, 1))
    # separate (contiguous) q / k give the same bits as the strided slices, and so does a repeat
    again = _run_kernels(q0.clone(), k0.clone(), vt, n, scale, L, C)
    for a, b in zip((sq, sk, q1, k_sh, vt_sh), again):
        assert torch.equal(a, b)
    qk2 = torch.cat((q0, k0), dim=2).contiguous()
    third = _run_kernels(qk2[:, :, :C], qk2[:, :, C:], vt[:, :, :L] if lp == L else vt, n, scale, L, C, packed=qk2.clone())
    for a, b in zip((sq, sk, q1, k_sh, vt_sh), third):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_statistics_survive_a_dc_offset(dtype):
    """Channel means 50 x the standard deviation: a global sum of squares loses the variance to cancellation (E[x^2] - E[x]^2 at 2500 : 1),
    the per-slab (count, mean, M2) merge does not."""
    B, L, C, n = 6, 1024, 640, 3
    g = torch.Generator(device=DEV).manual_seed(5)
    sigma = 0.5 + torch.rand(B, 1, C, device=DEV, generator=g)
    mk = lambda: ((torch.randn(B, L, C, device=DEV, generator=g) + 50.0 * torch.sign(torch.randn(B, 1, C, device=DEV, generator=g))) * sigma).to(dtype)  # noqa: E731
    q0, k0, v0 = mk(), mk(), mk()
    vt = v0.permute(2, 0, 1).contiguous()
    sq, sk, q1, k_sh, vt_sh = _run_kernels(q0.clone(), k0.clone(), vt, n, 0.5, L, C)
    for got, t in ((sq, q0), (sk, k0)):
        std, mean = torch.std_mean(t.float(), dim=1)
        e_mean, e_std = _rel(got[..., 0], mean), _rel(got[..., 1], std)
        print(f"DC offset {dtype}: mean {e_mean:.2e} std {e_std:.2e}")
        assert e_mean < 1e-5 and e_std < 1e-5
    rq, rk, rvt = pack_model(q0.float(), k0.float(), v0.float(), n, 0.5)
    errs = {"q'": _rel(q1.float(), rq), "k_sh": _rel(k_sh.float(), rk), "vt_sh": _rel(vt_sh.float(), rvt)}
    print(f"DC offset {dtype}: " + " ".join(f"{k_} {v:.2e}" for k_, v in errs.items()))
    assert all(v < KTOL[dtype] for v in errs.values()), errs


def test_kernels_refuse_what_they_cannot_compute():
    x = torch.randn(2, 1, 64, device=DEV)
    with pytest.raises(native.NativeError, match="ESHAPE"):  # one token: no unbiased standard deviation
        native.adain_stats(x, torch.empty(2, 64, 2, device=DEV))
    q, k, vt = torch.randn(6, 8, 64, device=DEV), torch.randn(6, 8, 64, device=DEV), torch.randn(64, 6, 8, device=DEV)
    st, one = torch.ones(6, 64, 2, device=DEV), torch.ones(1, device=DEV)
    k_sh, vt_sh = torch.zeros(6, 64, 64, device=DEV), torch.zeros(64, 6, 64, device=DEV)
    with pytest.raises(native.NativeError, match="ESHAPE"):  # groups of 4 rows in a batch of 6
        native.style_aligned_pack(q, k, vt, st, st, 4, one, 1e-8, k_sh, vt_sh)
    both = torch.zeros(6, 64, 64, device=DEV)
    with pytest.raises(native.NativeError, match="EARG"):  # the packed keys on top of the raw ones: other rows still read those
        native.style_aligned_pack(q, both[:, :8], vt, st, st, 3, one, 1e-8, both, vt_sh)
    vboth = torch.zeros(64, 6, 64, device=DEV)
    with pytest.raises(native.NativeError, match="EARG"):
        native.style_aligned_pack(q, k, vboth[:, :, :8], st, st, 3, one, 1e-8, k_sh, vboth)
    assert not k_sh.any() and not vt_sh.any()  # nothing was launched
    native.style_aligned_pack(q, k, vt, st, st, 3, one, 1e-8, k_sh, vt_sh)  # (the same arguments, well formed)
    assert k_sh[:, :16].any() and vt_sh[:, :, :16].any()


# ---- engine -----------------------------------------------------------------------------------------------------------------------------
def _build(name, dtype):
    case = STYLE_ALIGNED_CASES[name]
    unet = SDXLUNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sdxl", case["weight_seed"]), device=DEV, dtype=dtype)
    specs = case_specs(case, S.key_shapes("sdxl"))
    handles = S.synth.apply_adapters(unet, refiners_amd.namespace(), device=DEV, dtype=dtype, **specs)
    return unet, specs, handles


@pytest.fixture(scope="module")
def bare_f32():
    """One float32 SDXL UNet on the GPU for the cases without other adapters (a, b, c): tests inject and eject their own StyleAlignedAdapter."""
    return _build("a", torch.float32)[0]


def _inputs(name):
    return {k: v.to(DEV) for k, v in case_inputs(STYLE_ALIGNED_CASES[name]).items()}


def _set_context(unet, case, inp, dtype, handles=None, specs=None):
    unet.set_timestep(DDIM(case["num_steps"]).timesteps[case["step"]].unsqueeze(0).to(DEV))
    unet.set_clip_text_embedding(inp["text"].to(dtype))
    unet.set_pooled_text_embedding(inp["pooled"].to(dtype))
    unet.set_time_ids(inp["time_ids"])
    if handles is not None and handles["ip"] is not None:
        handles["ip"].set_clip_image_embedding(specs["ip"]["tokens"].to(device=DEV, dtype=dtype))


def _step_kwargs(inp, specs=None):
    kw = dict(clip_text_embedding=inp["text"], pooled_text_embedding=inp["pooled"], time_ids=inp["time_ids"])
    if specs is not None and specs["ip"] is not None:
        kw["clip_image_embedding"] = specs["ip"]["tokens"].to(DEV)
    return kw


def _check_engine_f32(name, unet, specs=None, handles=None):
    case, gold = STYLE_ALIGNED_CASES[name], S.golden("sdxl_style_aligned")
    inp = _inputs(name)
    adapter = StyleAlignedAdapter(unet, scale=case["scale"]).inject()
    try:
        fast = CompiledUNet(unet)
        xx = torch.cat((inp["x"], inp["x"]))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)  # no whole-UNet fallback
            _set_context(unet, case, inp, torch.float32, handles, specs)
            y = fast(xx)
        assert fast.stats["fallback_nodes"] == [] and "whole_fallback" not in fast.stats and fast.stats["style_aligned_sites"] == 70
        l2, mx = S.rel_err(y, gold[f"{name}.unet_out"])
        print(f"{name} f32 CompiledUNet vs reference: l2 {l2:.2e} max {mx:.2e}; {fast.stats['step_ops']} launches")
        assert l2 < F32_TOL and mx < F32_TOL, (name, l2, mx)
        _set_context(unet, case, inp, torch.float32, handles, specs)
        y_ref = unet(xx)  # the unfused mirror on the GPU
        l2, mx = S.rel_err(y, y_ref)
        print(f"{name} f32 CompiledUNet vs unfused mirror: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < F32_TOL and mx < F32_TOL, (name, "vs unfused", l2, mx)
        for _ in range(2):  # three runs in all, the graph replays included: bit-identical
            _set_context(unet, case, inp, torch.float32, handles, specs)
            assert torch.equal(fast(xx), y)
        sd = CompiledSDXL(unet, num_inference_steps=case["num_steps"], condition_scale=case["condition_scale"])
        sd.set_inputs(inp["x"], **_step_kwargs(inp, specs))
        x1 = sd.step(case["step"]).clone()
        assert sd.engine.stats["fallback_nodes"] == [] and sd.engine.stats["style_aligned_sites"] == 70
        l2, mx = S.rel_err(x1, gold[f"{name}.x_next"])
        print(f"{name} f32 CompiledSDXL.step vs reference: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < F32_TOL and mx < F32_TOL, (name, "x_next", l2, mx)
        for _ in range(2):
            sd.set_inputs(inp["x"], **_step_kwargs(inp, specs))
            assert torch.equal(sd.step(case["step"]), x1)
        return sd, adapter, inp
    except BaseException:
        adapter.eject()
        raise


@pytest.mark.parametrize("name", ["a", "c"])
def test_engine_float32_matches_reference(bare_f32, name):
    sd, adapter, inp = _check_engine_f32(name, bare_f32)
    adapter.eject()


def test_engine_float32_on_top_of_in_launch_lora_and_ip_adapter():
    unet, specs, handles = _build("d", torch.float32)
    sd, adapter, inp = _check_engine_f32("d", unet, specs, handles)
    assert sd.engine.stats["lora_sites"] == 722 and sd.engine.stats["ip_sites"] == 70
    adapter.eject()


def test_live_scale_eject_and_split_pair(bare_f32):
    """`adapter.scale = 1.0` on the live tree: the next step is golden b (same inputs as a), with NO re-lowering -- the kernels read the scale
    from device memory.  Eject: the next step is the bare tree's (golden a's x_next_without_adapter), no stale program.  cfg_split=True (each half
    of the CFG pair its own program: every row refers to row 0) agrees with the single program."""
    unet, case, gold = bare_f32, STYLE_ALIGNED_CASES["a"], S.golden("sdxl_style_aligned")
    inp = _inputs("a")
    adapter = StyleAlignedAdapter(unet, scale=case["scale"]).inject()
    try:
        sd = CompiledSDXL(unet, num_inference_steps=case["num_steps"], condition_scale=case["condition_scale"])
        sd.set_inputs(inp["x"], **_step_kwargs(inp))
        xa = sd.step(case["step"]).clone()
        assert S.rel_err(xa, gold["a.x_next"])[0] < F32_TOL
        program = sd.engine.low
        adapter.scale = STYLE_ALIGNED_CASES["b"]["scale"]
        sd.set_inputs(inp["x"], **_step_kwargs(inp))
        xb = sd.step(case["step"]).clone()
        l2, mx = S.rel_err(xb, gold["b.x_next"])
        print(f"live scale 0.5 -> 1.0: vs golden b l2 {l2:.2e} max {mx:.2e}; a vs b {S.rel_err(xa, xb)[0]:.2e}")
        assert l2 < F32_TOL and mx < F32_TOL and sd.engine.low is program and S.rel_err(xa, xb)[0] > 1e-2
        adapter.scale = case["scale"]
        split = CompiledSDXL(unet, num_inference_steps=case["num_steps"], condition_scale=case["condition_scale"], cfg_split=True)
        split.set_inputs(inp["x"], **_step_kwargs(inp))
        xs = split.step(case["step"]).clone()
        assert split.engine_c is not None and split.engine.stats["style_aligned_sites"] == 70 and split.engine_c.stats["style_aligned_sites"] == 70
        l2, mx = S.rel_err(xs, xa)
        print(f"cfg_split vs the single program: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < 1e-4, (l2, mx)
    finally:
        adapter.eject()
    sd.set_inputs(inp["x"], **_step_kwargs(inp))
    x0 = sd.step(case["step"])
    l2, mx = S.rel_err(x0, gold["a.x_next_without_adapter"])
    print(f"after eject: vs the reference without the adapter l2 {l2:.2e} max {mx:.2e}")
    assert l2 < F32_TOL and mx < F32_TOL and sd.engine.stats["style_aligned_sites"] == 0 and sd.engine.stats["fallback_nodes"] == []


def test_odd_batch_takes_the_stock_forward_with_a_warning(bare_f32):
    """Three rows have no two CFG halves: the lowering refuses, CompiledUNet warns and runs the stock Chain forward -- whose own answer to an odd batch
    (the reference's ExtractReferenceFeatures cannot split it either) is what the caller gets."""
    unet, case = bare_f32, STYLE_ALIGNED_CASES["a"]
    inp = _inputs("a")
    adapter = StyleAlignedAdapter(unet, scale=0.5).inject()
    try:
        cut = {k: v[:3] for k, v in inp.items()}
        fast = CompiledUNet(unet)
        _set_context(unet, case, cut, torch.float32)
        with pytest.raises(Exception) as stock:
            unet(cut["x"])
        _set_context(unet, case, cut, torch.float32)
        with pytest.warns(RuntimeWarning, match="odd batch"), pytest.raises(type(stock.value)):
            fast(cut["x"])
        assert "odd batch" in fast.stats["whole_fallback"]
    finally:
        adapter.eject()


def test_scales_set_apart_by_hand_fall_back_and_come_back(bare_f32):
    """One ScaleReferenceFeatures assigned on its own AFTER the program was lowered: the live tree no longer has ONE scale, the next call warns and runs the
    stock forward (which honours the odd layer); once the adapter's setter makes them common again the lowered path is back -- although no tree epoch moved."""
    from refiners_amd.latent_diffusion.style_aligned import ScaleReferenceFeatures

    unet, case, gold = bare_f32, STYLE_ALIGNED_CASES["a"], S.golden("sdxl_style_aligned")
    inp = _inputs("a")
    xx = torch.cat((inp["x"], inp["x"]))
    adapter = StyleAlignedAdapter(unet, scale=case["scale"]).inject()
    try:
        fast = CompiledUNet(unet)
        _set_context(unet, case, inp, torch.float32)
        y = fast(xx)
        assert fast.stats["style_aligned_sites"] == 70
        odd = list(unet.layers(ScaleReferenceFeatures))[100]
        odd.scale = 0.9
        _set_context(unet, case, inp, torch.float32)
        with pytest.warns(RuntimeWarning, match="different scales"):
            y_odd = fast(xx)
        _set_context(unet, case, inp, torch.float32)
        assert "different scales" in fast.stats["whole_fallback"] and S.rel_err(y_odd, unet(xx))[0] < 1e-5  # (the same unfused forward twice)
        _set_context(unet, case, inp, torch.float32)
        assert S.rel_err(fast(xx), y_odd)[0] < 1e-5 and "different scales" in fast.stats["whole_fallback"]  # the refusal is remembered: still the stock forward
        adapter.scale = case["scale"]
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            _set_context(unet, case, inp, torch.float32)
            y_back = fast(xx)
        assert "whole_fallback" not in fast.stats and fast.stats["style_aligned_sites"] == 70
        l2, mx = S.rel_err(y_back, gold["a.unet_out"])
        assert l2 < F32_TOL and mx < F32_TOL, (l2, mx)
    finally:
        adapter.eject()


@pytest.mark.parametrize("name", ["a", "c"])
def test_engine_bfloat16_close_to_float32_reference(name):
    case, gold = STYLE_ALIGNED_CASES[name], S.golden("sdxl_style_aligned")
    unet, specs, handles = _build(name, torch.bfloat16)
    StyleAlignedAdapter(unet, scale=case["scale"]).inject()
    inp = _inputs(name)
    xx = torch.cat((inp["x"], inp["x"])).to(torch.bfloat16)
    fast = CompiledUNet(unet)
    _set_context(unet, case, inp, torch.bfloat16)
    y = fast(xx)
    assert fast.stats["fallback_nodes"] == [] and fast.stats["style_aligned_sites"] == 70
    l2, mx = S.rel_err(y.float(), gold[f"{name}.unet_out"])
    _set_context(unet, case, inp, torch.bfloat16)
    l2_t, _ = S.rel_err(unet(xx).float(), gold[f"{name}.unet_out"])  # stock torch bf16 kernels on the same tree
    print(f"{name} bf16: engine l2 {l2:.2e} max {mx:.2e}; torch-bf16 unfused l2 {l2_t:.2e}")
    assert l2 < BF16_TOL, (name, l2, mx)
    assert l2 < 1.15 * l2_t + 1e-3, "the fused path must not be less accurate than the unfused bf16 path"
