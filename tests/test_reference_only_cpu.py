"""Reference-only control without a GPU: the mirror's adapter against what the reference's own classes computed (tests/golden/reference_only*,
tools/make_golden_reference_only.py), the tree bookkeeping of the reference's tests/adapters/test_reference_only_control.py, and dry lowerings
on the meta device: what the guide part and the real pass consist of, what is refused, and that an ejected tree lowers to the bare program."""
import json
import os
import sys
from pathlib import Path

import pytest
import torch

import refiners_amd
import refiners_amd.fluxion.layers as fl
from refiners_amd import build_native, native
from refiners_amd.engine.packing import Unsupported, launches
from refiners_amd.engine.unet_lowering import UNetIO, UNetLowering
from refiners_amd.latent_diffusion import ReferenceOnlyControlAdapter, SaveLayerNormAdapter, SelfAttentionInjectionAdapter, SelfAttentionInjectionPassthrough
from refiners_amd.latent_diffusion.blocks import CrossAttentionBlock
from refiners_amd.latent_diffusion.sd1 import SD1UNet
from tests import ella_cases as E
from tests import reference_only_cases as R
from tests import support as S

ROOT = Path(__file__).resolve().parent.parent
REF = next((Path(c) for c in (os.environ.get("REFINERS_SRC"), ROOT / "oracle" / "_ref" / "src") if c and (Path(c) / "refiners").exists()), None)
CPU_TOL = 1e-5  # relative l2: both sides run the same torch arithmetic on the same machine type
TEXT = ("cross_attention_block", "clip_text_embedding")


# ------------------------------------------------------------------------------------------------ the mirror against the reference's outputs
@pytest.fixture(scope="module")
def gold():
    return S.golden("reference_only")


@pytest.fixture(scope="module")
def tree():
    unet = SD1UNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sd1", R.SEED["weight_seed"]), device="cpu", dtype=torch.float32)
    return unet, ReferenceOnlyControlAdapter(unet).inject()


def _close(got, ref, what):
    l2, mx = S.rel_err(got, ref)
    print(f"{what}: l2 {l2:.2e} max {mx:.2e}")
    assert l2 <= CPU_TOL, (what, l2, mx)


def test_mirror_matches_the_reference_on_cpu(tree, gold):
    unet, adapter = tree
    ts = R.CASES["main"]["timesteps"]
    _close(R.run(unet, adapter, "main", ts[0]), gold["main.t0"], "main t0")
    _close(R.run(unet, adapter, "main", ts[1]), gold["main.t1"], "main t1")
    for key, style in R.STYLES.items():  # style_cfg is read at forward time
        for sub in adapter.sub_adapters:
            sub.style_cfg = style
        _close(R.run(unet, adapter, "main", ts[0]), gold[f"main.{key}"], f"main {key}")
    for sub in adapter.sub_adapters:
        sub.style_cfg = 0.5
    _close(R.run(unet, adapter, "odd", R.CASES["odd"]["timesteps"][0]), gold["odd.t0"], "odd t0")
    assert not torch.allclose(gold["main.t0"], gold["main.bare"], atol=1e-3) and not torch.allclose(gold["main.t0"], gold["main.s1"], atol=1e-3)


def test_tree_shape_and_inject_eject_bookkeeping():
    unet = SD1UNet(4, device="meta")
    before = repr(unet)
    blocks = list(unet.layers(CrossAttentionBlock))
    adapter = ReferenceOnlyControlAdapter(unet)
    assert repr(unet) == before and len(adapter.sub_adapters) == len(blocks) == 16
    adapter.inject()
    assert isinstance(unet[0], SelfAttentionInjectionPassthrough) and unet.parent is adapter
    assert len(list(unet.layers(SelfAttentionInjectionAdapter))) == 16
    guide_unet = unet[0][2]
    saves = list(guide_unet.layers(SaveLayerNormAdapter))
    assert [s.context for s in saves] == [f"self_attention_context_{i}" for i in range(16)] == [a.context for a in adapter.sub_adapters]
    assert [type(m).__name__ for m in unet[0]] == ["Lambda", "UseContext", "SD1UNet", "Lambda"] and (unet[0][1].context, unet[0][1].key) == ("reference_only_control", "guide")
    # the copy shares the leaves: every Linear of the real pass's self-attentions is the guide's own
    real = [p for a in adapter.sub_adapters for p in a.target.parameters()]
    copy = [p for s in saves for p in s.target.parameters()]
    assert len(real) == len(copy) and all(a is b for a, b in zip(real, copy))
    sub = adapter.sub_adapters[0]
    assert [type(m).__name__ for m in sub] == ["Parallel", "Lambda"] and [type(m).__name__ for m in sub[0]] == ["SelfAttention", "Chain"]
    cats = list(sub[0][0][0])
    assert isinstance(cats[0], fl.Identity) and all(isinstance(c, fl.Concatenate) and c.dim == 1 for c in cats[1:])
    with pytest.raises(RuntimeError, match="cannot be copied"):
        adapter.structural_copy()
    with pytest.raises(AssertionError, match="already injected"):
        adapter.inject()
    adapter.eject()
    assert repr(unet) == before and unet.parent is None and not list(unet.layers(SelfAttentionInjectionAdapter))
    guide = torch.zeros(2, 4, 8, 8)
    adapter.set_controlnet_condition(guide)
    assert adapter.use_context("reference_only_control")["guide"] is guide


# ------------------------------------------------------------------------------------------------ dry lowerings
def _dry(unet, dtype=torch.float32, B=2, cin=4, guide=True, hw=(32, 32), guide_shape=None):
    dev = torch.device("meta")
    H, W = hw
    io = UNetIO(x=torch.empty(B, cin, H, W, device=dev, dtype=dtype), timestep=torch.empty(B, device=dev), out=torch.empty(B, 4, H, W, device=dev, dtype=dtype))
    io.tokens[TEXT] = (torch.zeros(B * 128, 768, device=dev, dtype=dtype), 77)
    if guide:
        io.guide = torch.empty(guide_shape or (B, cin, H, W), device=dev, dtype=dtype)
    low = UNetLowering(dev, dtype)
    low.lower(unet, io)
    return low


def _names(ops):
    return [e[2] for e in ops if e[0] is not None]


def _adapted(dtype=torch.float32, cin=4):
    unet = SD1UNet(cin, device="meta", dtype=dtype)
    return unet, ReferenceOnlyControlAdapter(unet).inject()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_both_passes_lower_into_one_step_program(dtype):
    bare = _dry(SD1UNet(4, device="meta", dtype=dtype), dtype, guide=False)
    unet, adapter = _adapted(dtype)
    low = _dry(unet, dtype)
    assert low.stats["fallback_nodes"] == [] and low.stats["reference_only_sites"] == 16
    n = low.stats["reference_only_guide_ops"]
    ops = [e for e in low.step if e[0] is not None]
    guide, real = ops[:n], ops[n:]
    assert _names(real).count("mi355x_attention_joint") == 16 and "mi355x_attention_joint" not in _names(guide)
    # the guide part: the self-attentions of 15 sites (Lq == Lk) and their blocks' 15 text cross-attentions (77 keys); site 16 projects K | V^T and stops
    ga = [e[1][0]._obj for e in guide if e[2] == "mi355x_attention_general"]
    assert sum(1 for a in ga if a.Lq == a.Lk) == 15 and sum(1 for a in ga if a.Lk == 77) == 15 and len(ga) == 30
    assert not any(a.Lq == a.Lk for a in (e[1][0]._obj for e in real if e[2] == "mi355x_attention_general"))
    assert guide[-1][2] == "mi355x_gemm" and {guide[-1][1][0]._obj.M, guide[-1][1][0]._obj.N} == {320, 2048} and n < launches(bare.step)  # V^T of the last site: 320 channels x 2 x 1024 tokens
    # the real pass is the bare program with the joint kernel in place of the 16 self-attention launches, minus the timestep encoder the guide part ran
    assert len(real) < launches(bare.step) and launches(low.step) == n + len(real)
    assert E.program_digest(low.prologue) == E.program_digest(bare.prologue)  # text K / V^T once for both passes
    js = [e[1][0]._obj for e in real if e[2] == "mi355x_attention_joint"]
    assert sorted({(a.D, a.Lq) for a in js}) == [(40, 1024), (80, 256), (160, 16), (160, 64)] and all(a.Lk0 == a.Lk1 == a.Lq and a.B == 2 and a.H == 8 for a in js)
    adapter.eject()
    assert E.program_digest(_dry(unet, dtype, guide=False).step) == E.program_digest(bare.step)


def test_ejected_tree_lowers_to_the_program_of_before():
    unet, adapter = _adapted()
    adapter.eject()
    want = json.loads((S.GOLD / "ella_bare_programs.json").read_text())["sd1_float32"]
    low = _dry(unet, guide=False)
    assert {"step": E.program_digest(low.step), "prologue": E.program_digest(low.prologue)} == want
    assert "reference_only_sites" not in low.stats


def test_nine_input_channels_lower():
    unet, _ = _adapted(cin=9)
    low = _dry(unet, cin=9)
    assert low.stats["reference_only_sites"] == 16 and low.stats["fallback_nodes"] == []


def test_lora_injected_before_the_adapter_is_carried_by_the_copy():
    unet = SD1UNet(4, device="meta")
    S.load_mirror_weights(unet, S.weights("sd1", 0), device="meta", dtype=torch.float32)
    R.add_lora(unet, R.lora_api(refiners_amd.namespace()), S.key_shapes("sd1"), device="meta", dtype=torch.float32)
    ReferenceOnlyControlAdapter(unet).inject()
    low = _dry(unet)
    assert low.stats["reference_only_sites"] == 16 and low.stats["lora_sites"] == 64 and low.stats["fallback_nodes"] == []


def test_refusals():
    unet, adapter = _adapted()
    with pytest.raises(Unsupported, match="batch of 4"):
        _dry(unet, B=4)
    with pytest.raises(Unsupported, match="guide of the input's shape"):
        _dry(unet, guide_shape=(2, 4, 16, 16))
    with pytest.raises(Unsupported, match="guide is unset"):
        _dry(unet, guide=False)
    adapter.sub_adapters[3].style_cfg = 0.25
    with pytest.raises(Unsupported, match="different style_cfg"):
        _dry(unet)
    adapter.sub_adapters[3].style_cfg = 0.5


def _swap_key_linear(sa):
    lin = sa.layer(("Distribute", "Linear_2"), fl.Linear)
    sa.layer("Distribute", fl.Chain).replace(lin, fl.Linear(lin.in_features, lin.out_features, bias=False, device="meta"))


def test_refusal_when_the_guide_pass_projects_keys_with_other_linears():
    """The identity the lowering rests on: Wk / Wv of the guide copy at site i are the real pass's own modules, so the guide's K / V^T are the extra keys.
    Another Wk in the GUIDE copy (the real pass untouched, its guided and plain branches still sharing theirs) must be refused by that check and no other."""
    unet, adapter = _adapted()
    saves = list(unet[0][2].layers(SaveLayerNormAdapter))
    _swap_key_linear(saves[5].target)
    with pytest.raises(Unsupported, match="of the guide pass and the real pass are not the same modules"):
        _dry(unet)


def test_refusal_when_the_guided_and_plain_branches_of_a_site_differ():
    unet, adapter = _adapted()
    _swap_key_linear(adapter.sub_adapters[5].target)  # the plain branch; the guided branch is a structural copy that keeps the old Linear
    with pytest.raises(Unsupported, match="the guided and the plain SelfAttention of one site do not share their Linears"):
        _dry(unet)


def test_refusal_of_a_head_width_no_instance_serves():
    """16 heads over 320 channels: 20 channels per head, 40 bytes in bfloat16, no multiple of the kernels' 16-byte chunks."""
    unet = SD1UNet(4, device="meta", dtype=torch.bfloat16)
    sa = next(iter(unet.layers(CrossAttentionBlock))).ensure_find(fl.SelfAttention)
    sa.num_heads = 16
    sa.ensure_find(fl.ScaledDotProductAttention).num_heads = 16
    ReferenceOnlyControlAdapter(unet).inject()
    with pytest.raises(Unsupported, match="heads of 20 channels, which no instance of the joint attention kernel serves"):
        _dry(unet, torch.bfloat16)


def test_refusal_of_a_split_pair_and_of_biased_projections():
    unet, adapter = _adapted()
    dev = torch.device("meta")
    io = UNetIO(x=torch.empty(2, 4, 32, 32, device=dev), timestep=torch.empty(2, device=dev), out=torch.empty(2, 4, 32, 32, device=dev), guide=torch.empty(2, 4, 32, 32, device=dev))
    io.tokens[TEXT] = (torch.zeros(2 * 128, 768, device=dev), 77)
    low = UNetLowering(dev, torch.float32)
    low.style_half_batch = True  # what CompiledUNet sets under io_override (CompiledSDXL's cfg_split)
    with pytest.raises(Unsupported, match="cfg_split"):
        low.lower(unet, io)
    adapter.eject()
    sa = next(iter(unet.layers(CrossAttentionBlock))).ensure_find(fl.SelfAttention)
    lin = sa.layer(("Distribute", "Linear_1"), fl.Linear)
    sa.layer("Distribute", fl.Chain).replace(lin, fl.Linear(lin.in_features, lin.out_features, bias=True, device="meta"))
    ReferenceOnlyControlAdapter(unet).inject()
    with pytest.raises(Unsupported, match="bias"):
        _dry(unet)


def test_refusal_when_a_controlnet_sits_in_front_of_the_guide_pass():
    from refiners_amd.latent_diffusion.controlnet import SD1ControlnetAdapter

    unet, _ = _adapted()
    SD1ControlnetAdapter(unet, name="canny").inject()  # injected last: the Controlnet is the first child, the guide pass the second
    with pytest.raises(Unsupported, match="SelfAttentionInjectionPassthrough is not the UNet's first child"):
        _dry(unet)


@pytest.mark.parametrize("other", ["sag", "style_aligned", "controlnet", "t2i"])
def test_refusal_together_with_other_adapters(other):
    from refiners_amd.latent_diffusion.controlnet import SD1ControlnetAdapter
    from refiners_amd.latent_diffusion.sag import SD1SAGAdapter
    from refiners_amd.latent_diffusion.style_aligned import StyleAlignedAdapter
    from refiners_amd.latent_diffusion.t2i import T2IFeatures

    unet = SD1UNet(4, device="meta")
    if other == "sag":
        ReferenceOnlyControlAdapter(unet).inject()
        SD1SAGAdapter(unet).inject()
        match = "reference-only control together with Self-Attention Guidance is not lowered"
    elif other == "style_aligned":
        ReferenceOnlyControlAdapter(unet).inject()
        StyleAlignedAdapter(unet).inject()
        match = "reference-only control together with StyleAligned is not lowered"
    elif other == "controlnet":
        SD1ControlnetAdapter(unet, name="canny").inject()
        ReferenceOnlyControlAdapter(unet).inject()
        match = "reference-only control together with a ControlNet is not lowered"
    else:
        ReferenceOnlyControlAdapter(unet).inject()
        unet.layer(("DownBlocks", "Chain_2"), fl.Chain).append(T2IFeatures(name="depth", index=0, scale=1.0))  # (where a T2I-Adapter puts its taps)
        match = "reference-only control together with a T2I-Adapter is not lowered"
    with pytest.raises(Unsupported, match=match):
        _dry(unet)


@pytest.mark.skipif(REF is None, reason="no refiners checkout (REFINERS_SRC / oracle/_ref)")
def test_reference_tree_lowers_to_the_same_program():
    sys.path[:0] = [p for p in (str(ROOT / "oracle" / "shim"), str(REF)) if p not in sys.path]
    from refiners.foundationals.latent_diffusion.reference_only_control import ReferenceOnlyControlAdapter as RefAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet as RefUNet

    ref = RefUNet(4, device="meta")
    RefAdapter(ref).inject()
    assert type(ref).__module__.startswith("refiners.")
    mine, _ = _adapted()
    a, b = _dry(ref), _dry(mine)
    assert E.program_digest(a.step) == E.program_digest(b.step) and E.program_digest(a.prologue) == E.program_digest(b.prologue)
    assert a.stats["reference_only_sites"] == b.stats["reference_only_sites"] == 16


# ------------------------------------------------------------------------------------------------ the native entry point's plumbing
def test_build_lists_and_header():
    assert "reference_only.hip" in build_native.SOURCES and "../../include/mi355x_refiners_reference_only.h" in build_native.HEADERS
    assert build_native.DEPS["reference_only.hip"] == ["attn_general_kernel.cuh", "common.cuh", "../../include/mi355x_refiners_reference_only.h"]
    assert build_native.DEPS["attention_general.hip"] == ["attn_general_kernel.cuh", "common.cuh"]  # (the two share one kernel template)
    fields = [name for name, _t in native.AttnJointArgs._fields_]
    assert fields[:7] == ["dtype", "B", "H", "Lq", "D", "Lk0", "Lk1"] and {"mix", "k1", "vt1", "scale"} <= set(fields)
