"""StyleAligned shared self-attention, host side (CPU): the mirror (refiners_amd/latent_diffusion/style_aligned.py) against the REAL
reference's step (tests/golden/sdxl_style_aligned.safetensors, tools/make_golden_style_aligned.py), the lowering's pattern matcher and
launch program (dry run on the meta device), and the torch model of the pack kernel's index arithmetic.  The kernels and the engine
are checked on the GPU in tests/test_style_aligned_gpu.py."""
import os
import sys
from collections import Counter
from pathlib import Path

import pytest
import torch

import refiners_amd
import refiners_amd.fluxion.layers as fl
from refiners_amd import synth
from refiners_amd.engine.packing import Unsupported
from refiners_amd.latent_diffusion.sampling import DDIM, SDXLDenoiser
from refiners_amd.latent_diffusion.sdxl import SDXLUNet
from refiners_amd.latent_diffusion.style_aligned import AdaIN, SharedSelfAttentionAdapter, StyleAligned, StyleAlignedAdapter
from tests import support as S
from tests.style_aligned_cases import STYLE_ALIGNED_CASES, case_inputs, case_specs, pack_model
from tests.test_lowering_cpu import _dry

TOL = 2e-4  # mirror against reference, the bar of tests/test_sag_golden.py
TOKENS = {("cross_attention_block", "clip_text_embedding"): (77, 2048)}
REF = Path(os.environ.get("REFINERS_SRC") or Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "src")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from refiners_amd.build_native import build_native

    build_native()


def _ops(low):
    return [e[2] for e in low.step]


@pytest.mark.parametrize("name", list(STYLE_ALIGNED_CASES))
def test_mirror_step_matches_reference(name):
    case = STYLE_ALIGNED_CASES[name]
    gold = S.golden("sdxl_style_aligned")
    unet = SDXLUNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sdxl", case["weight_seed"]))
    specs = case_specs(case, S.key_shapes("sdxl"))
    handles = synth.apply_adapters(unet, refiners_amd.namespace(), **specs)
    before, parent = repr(unet), unet.parent
    adapter = refiners_amd.namespace().StyleAlignedAdapter(unet, scale=case["scale"]).inject()
    assert isinstance(adapter, StyleAlignedAdapter) and len(adapter.shared_self_attention_adapters) == 70 and adapter.scale == case["scale"]
    sd = SDXLDenoiser(unet, DDIM(case["num_steps"]))
    inp = case_inputs(case)
    kw = dict(clip_text_embedding=inp["text"], pooled_text_embedding=inp["pooled"], time_ids=inp["time_ids"], condition_scale=case["condition_scale"])
    seen = []
    hook = unet.register_forward_hook(lambda _m, _a, y: seen.append(y))
    with torch.no_grad():
        if handles["ip"] is not None:
            handles["ip"].set_clip_image_embedding(specs["ip"]["tokens"])
        x1 = sd(inp["x"], case["step"], **kw)
    hook.remove()
    for got, key in ((x1, "x_next"), (seen[0], "unet_out")):
        l2, mx = S.rel_err(got, gold[f"{name}.{key}"])
        print(f"{name} {key}: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < TOL and mx < TOL, (name, key, l2, mx)
    if name != "b":
        plain = gold[f"{name}.x_next_without_adapter"]
        # the reference image attends to its own keys twice (the softmax cancels it) and is AdaIN'd with its own statistics: unchanged ...
        assert S.rel_err(x1[:1], plain[:1])[0] < 1e-4
        # ... while the others take its style: the fixture does exercise the adapter
        assert min(S.rel_err(x1[i : i + 1], plain[i : i + 1])[0] for i in range(1, case["images"])) > 5e-2
    adapter.eject()
    assert repr(unet) == before and unet.parent is parent


def test_scale_accessors_reach_every_layer():
    unet = SDXLUNet(4, device="meta")
    adapter = StyleAlignedAdapter(unet, scale=0.5).inject()
    adapter.scale = 0.25
    assert adapter.scale == 0.25 and all(m.scale == 0.25 for m in unet.layers(StyleAligned))
    assert sum(1 for _ in unet.layers(StyleAligned)) == 210 and sum(1 for _ in unet.layers(AdaIN)) == 140
    site = adapter.shared_self_attention_adapters[3]
    assert isinstance(site, SharedSelfAttentionAdapter) and site.parent is not None and site.target.parent is site


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lowering_takes_the_adapter_without_fallback(dtype):
    unet = SDXLUNet(4, device="meta", dtype=dtype)
    bare = _dry(unet, 4, 32, 32, dtype, TOKENS)
    adapter = StyleAlignedAdapter(unet, scale=0.5).inject()
    low = _dry(unet, 4, 32, 32, dtype, TOKENS)
    kinds = Counter(_ops(low))
    assert low.stats["fallback_nodes"] == [] and low.stats["style_aligned_sites"] == 70 and bare.stats["style_aligned_sites"] == 0
    assert kinds["mi355x_style_aligned_pack"] == 70 and kinds["mi355x_adain_stats"] == 70 and kinds["mi355x_attention"] == 140
    # the rest of the program is the bare tree's
    rest = [k for k in _ops(low) if k not in ("mi355x_style_aligned_pack", "mi355x_adain_stats")]
    assert rest == _ops(bare)
    packs = [e[1][0]._obj for e in low.step if e[2] == "mi355x_style_aligned_pack"]
    assert {(int(a.B), int(a.n)) for a in packs} == {(4, 2)} and {int(a.L) for a in packs} == {64, 256} and {int(a.C) for a in packs} == {640, 1280}
    att = [e[1][0]._obj for e in low.step if e[2] == "mi355x_attention"]
    assert sorted({(int(a.Lq), int(a.kv[0].Lk)) for a in att if a.kv[0].Lk > 77}) == [(64, 128), (256, 512)]
    # eject: exactly the launch sequence of a tree that never carried the adapter
    adapter.eject()
    assert _ops(_dry(unet, 4, 32, 32, dtype, TOKENS)) == _ops(bare)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sd15_heads_take_the_general_attention_kernel_over_twice_the_keys(dtype):
    """SD1.5's heads of 40 / 80 / 160 channels: the same statistics and pack launches, then mi355x_attention_general with Lq = L and Lk = 2L on the
    packed buffers (keys padded to 64)."""
    from refiners_amd.latent_diffusion.sd1 import SD1UNet

    tokens = {("cross_attention_block", "clip_text_embedding"): (77, 768)}
    unet = SD1UNet(4, device="meta", dtype=dtype)
    bare = _dry(unet, 2, 24, 24, dtype, tokens, pooled=False)
    adapter = StyleAlignedAdapter(unet, scale=0.5).inject()
    sites = len(adapter.shared_self_attention_adapters)
    low = _dry(unet, 2, 24, 24, dtype, tokens, pooled=False)
    kinds = Counter(_ops(low))
    assert sites == 16 and low.stats["style_aligned_sites"] == sites and low.stats["fallback_nodes"] == []
    assert kinds["mi355x_style_aligned_pack"] == sites and kinds["mi355x_attention"] == 0
    assert [k for k in _ops(low) if k not in ("mi355x_style_aligned_pack", "mi355x_adain_stats")] == _ops(bare)
    att = [e[1][0]._obj for e in low.step if e[2] == "mi355x_attention_general"]
    shared = sorted({(int(a.Lq), int(a.Lk), int(a.Dqk), int(a.vt_batch_stride)) for a in att if a.Lk != 77})
    # 24 x 24 latents: 576 / 144 / 36 / 9 tokens; V^T columns per sample = 2 L rounded up to 64
    assert shared == [(9, 18, 160, 64), (36, 72, 160, 128), (144, 288, 80, 320), (576, 1152, 40, 1152)]
    packs = [e[1][0]._obj for e in low.step if e[2] == "mi355x_style_aligned_pack"]
    assert {(int(a.B), int(a.n)) for a in packs} == {(2, 1)} and all(int(a.ksh_batch_stride) == int(a.vtsh_batch_stride) * int(a.C) for a in packs)
    adapter.eject()
    assert _ops(_dry(unet, 2, 24, 24, dtype, tokens, pooled=False)) == _ops(bare)


def test_lowering_refuses_what_is_not_the_adapters_pattern():
    unet = SDXLUNet(4, device="meta")
    adapter = StyleAlignedAdapter(unet, scale=0.5).inject()
    with pytest.raises(Unsupported, match="odd batch"):
        _dry(unet, 3, 32, 32, torch.float32, TOKENS)
    key_branch = adapter.shared_self_attention_adapters[5].style_aligned_layers.layer(1, StyleAligned)
    gone = key_branch.ensure_find(AdaIN)
    key_branch.remove(gone)
    with pytest.raises(Unsupported, match="StyleAligned branches differ"):
        _dry(unet, 4, 32, 32, torch.float32, TOKENS)
    key_branch.insert(1, gone)
    assert _dry(unet, 4, 32, 32, torch.float32, TOKENS).stats["style_aligned_sites"] == 70
    next(iter(unet.layers(StyleAligned))).scale = 0.75  # one layer set apart by hand: no longer ONE common scale
    with pytest.raises(Unsupported, match="different scales"):
        _dry(unet, 4, 32, 32, torch.float32, TOKENS)
    adapter.scale = 0.75
    cat = key_branch.ensure_find(fl.Concatenate)
    cat.dim = -1
    with pytest.raises(Unsupported, match="along the tokens"):
        _dry(unet, 4, 32, 32, torch.float32, TOKENS)


def test_self_attention_guidance_tap_on_a_shared_attention_is_refused():
    from refiners_amd.latent_diffusion.sag import SDXLSAGAdapter

    unet = SDXLUNet(4, device="meta")
    SDXLSAGAdapter(unet, scale=0.75).inject()
    StyleAlignedAdapter(unet, scale=0.5).inject()
    with pytest.raises(Unsupported, match="Self-Attention Guidance"):
        _dry(unet, 4, 32, 32, torch.float32, TOKENS)


@pytest.mark.parametrize("n,L,scale", [(1, 5, 0.3), (3, 37, 0.5), (2, 64, 1.0)])
def test_pack_model_agrees_with_the_adapter_layers(n, L, scale):
    """r(b), s_b, the [L, 2L) placement and the zero padding of the kernel's torch model against the mirror's own layers."""
    g = torch.Generator().manual_seed(L)
    B, C = 2 * n, 16
    q, k, v = (torch.randn(B, L, C, generator=g) * 2 + 3 for _ in range(3))
    layers = fl.Distribute(*(StyleAligned(adain=a, concatenate=c, scale=scale) for a, c in SharedSelfAttentionAdapter.BRANCHES))
    rq, rk, rv = layers(q, k, v)
    mq, k_sh, vt_sh = pack_model(q, k, v, n, scale)
    lkp = k_sh.shape[1]
    assert lkp % 64 == 0 and 2 * L <= lkp < 2 * L + 64 and tuple(vt_sh.shape) == (C, B, lkp)
    assert torch.allclose(mq, rq, rtol=1e-5, atol=1e-6) and torch.allclose(k_sh[:, : 2 * L], rk, rtol=1e-5, atol=1e-6)
    assert torch.allclose(vt_sh[:, :, : 2 * L].permute(1, 2, 0), rv, rtol=1e-6, atol=0)
    assert not k_sh[:, 2 * L :].any() and not vt_sh[:, :, 2 * L :].any()
    # one half of the CFG pair as its own program (group = rows): every row refers to row 0, as the first n rows of the whole batch do
    hq, hk, hvt = pack_model(q[:n], k[:n], v[:n], n, scale)
    assert torch.equal(hq, mq[:n]) and torch.equal(hk, k_sh[:n]) and torch.equal(hvt, vt_sh[:, :n])


@pytest.mark.skipif(not (REF / "refiners").exists(), reason="no refiners package (REFINERS_SRC / oracle/_ref, staged by build())")
def test_refiners_own_classes_lower_to_the_same_program_and_print_alike():
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "oracle" / "shim"), str(REF)]
    import refiners.fluxion.layers as rfl
    from refiners.foundationals.latent_diffusion.stable_diffusion_xl.unet import SDXLUNet as RefUNet
    from refiners.foundationals.latent_diffusion.style_aligned import StyleAligned as RefStyleAligned
    from refiners.foundationals.latent_diffusion.style_aligned import StyleAlignedAdapter as RefAdapter

    no_lambdas = lambda text: [ln for ln in text.splitlines() if "Lambda(" not in ln]  # noqa: E731  (they print their annotations, spelled differently in the mirror)
    programs, prints = [], []
    for cls, adapter_cls in ((RefUNet, RefAdapter), (SDXLUNet, StyleAlignedAdapter)):
        unet = cls(4, device="meta", dtype=torch.bfloat16)
        adapter = adapter_cls(unet, scale=0.5).inject()
        low = _dry(unet, 4, 32, 32, torch.bfloat16, TOKENS)
        programs.append((_ops(low), low.stats["style_aligned_sites"], low.stats["fallback_nodes"]))
        prints.append((repr(adapter.shared_self_attention_adapters[0]), no_lambdas(repr(unet))))
        adapter.eject()
        prints.append(no_lambdas(repr(unet)))
    assert programs[0] == programs[1] and programs[0][1] == 70
    assert prints[0] == prints[2] and prints[1] == prints[3]
    # the torch model of the kernels against the reference's own layers
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(6, 21, 8, generator=g) + 2 for _ in range(3))
    layers = rfl.Distribute(RefStyleAligned(adain=True, concatenate=False, scale=0.4), RefStyleAligned(adain=True, concatenate=True, scale=0.4),
                            RefStyleAligned(adain=False, concatenate=True, scale=0.4))
    rq, rk, rv = layers(q, k, v)
    mq, k_sh, vt_sh = pack_model(q, k, v, 3, 0.4)
    assert torch.allclose(mq, rq, rtol=1e-5, atol=1e-6) and torch.allclose(k_sh[:, :42], rk, rtol=1e-5, atol=1e-6)
    assert torch.allclose(vt_sh[:, :, :42].permute(1, 2, 0), rv, rtol=1e-6, atol=0)
