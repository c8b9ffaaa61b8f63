"""ELLA without a GPU: the mirror against the real reference (tests/golden/ella*, written by tools/make_golden_ella.py), its state-dict keys,
inject / eject, the binding of include/mi355x_refiners_ella.h, and dry lowerings on the meta device: where the resampler's launches and the
K / V^T projections of its tokens land, and that trees without ELLA lower to the programs they lowered to before."""
import json
import os
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from refiners_amd import native  # noqa: E402
from refiners_amd.engine.ella import ELLA_TOKENS, LLM_TOKENS  # noqa: E402
from refiners_amd.engine.unet_lowering import UNetIO, UNetLowering  # noqa: E402
from refiners_amd.latent_diffusion import ELLA, ELLAAdapter, SD1ELLAAdapter  # noqa: E402
from refiners_amd.latent_diffusion.sd1 import SD1UNet  # noqa: E402
from tests import ella_cases as E  # noqa: E402
from tests import support as S  # noqa: E402

REF = next((Path(c) for c in (os.environ.get("REFINERS_SRC"), ROOT / "oracle" / "_ref" / "src") if c and (Path(c) / "refiners").exists()), None)


@pytest.fixture(scope="module")
def gold():
    return S.golden("ella")


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("case", list(E.ELLA_CASES))
def test_mirror_matches_the_reference(case, gold):
    model = E.mirror(case)
    assert list(model.state_dict()) == list(E.key_shapes(case)) and {k: tuple(v.shape) for k, v in model.state_dict().items()} == E.key_shapes(case)
    llm = E.llm_embedding(case)
    for i, ts in enumerate(E.ELLA_CASES[case]["timesteps"]):
        l2, mx = S.rel_err(E.run_tree(model, ts, llm), gold[f"{case}.t{i}"])
        print(f"{case} t{i}: l2 {l2:.2e} max {mx:.2e}")
        assert l2 < 1e-5 and mx < 1e-5  # the same float32 torch operators in the same order


def test_adapter_keys_inject_and_eject():
    unet = SD1UNet(4, device="meta")
    bare = repr(unet)
    adapter = SD1ELLAAdapter(unet)
    assert isinstance(adapter, ELLAAdapter) and isinstance(adapter.latents_encoder, ELLA)
    assert list(adapter.latents_encoder.state_dict()) == list(E.key_shapes("sd1_full"))
    assert {k: tuple(v.shape) for k, v in adapter.latents_encoder.state_dict().items()} == E.key_shapes("sd1_full")
    assert len(adapter.sub_adapters) == 32
    assert adapter.init_context() == {"ella": {"timestep_embedding": None, "latents": None}}
    assert adapter.latents_encoder.layer("PerceiverResampler", torch.nn.Module).init_context() == {"perceiver_resampler": {"x": None}}
    adapted = None
    for _ in range(2):
        adapter.inject()
        assert list(unet._modules.values())[0] is adapter.latents_encoder and unet.parent is adapter
        readers = [r for sub in adapter.sub_adapters for r in sub._modules.values()]
        assert len(readers) == 32 and all((r.context, r.key) == ELLA_TOKENS for r in readers)
        assert all(sub.parent is not None for sub in adapter.sub_adapters)
        adapted = adapted or repr(unet)
        assert repr(unet) == adapted != bare
        adapter.eject()
        assert repr(unet) == bare and unet.parent is None
    llm = torch.zeros(2, 5, 2048)
    adapter.inject()
    adapter.set_llm_text_embedding(llm)
    assert list(unet._modules.values())[1].provider.contexts["adapted_cross_attention_block"]["llm_text_embedding"] is llm


def test_zero_initialised_modulation_is_the_identity():
    """The reference's initial state: every AdaLayerNorm Linear is zero, so AdaLayerNorm is LayerNorm without affine."""
    from refiners_amd.latent_diffusion.ella import AdaLayerNorm

    ada = AdaLayerNorm(64, 32)
    ada.set_context("ella", {"timestep_embedding": torch.randn(2, 1, 32)})
    x = torch.randn(2, 7, 64)
    assert torch.allclose(ada(x), torch.nn.functional.layer_norm(x, (64,), eps=1e-6), atol=1e-6)


# ------------------------------------------------------------------------------------------------ the header
def test_ella_header_is_bound_and_exported():
    """The ELLA header's prototype written out by hand (its names, layout and exports: tests/test_abi_header_cpu.py)."""
    import ctypes as C

    from refiners_amd.build_native import build_native

    build_native()
    lib = native.load()
    assert hasattr(lib, "mi355x_ella_adaln") and lib.mi355x_ella_adaln.argtypes == [C.POINTER(native.EllaAdaLnArgs), C.c_void_p]


# ------------------------------------------------------------------------------------------------ dry lowerings
def _dry(unet, table=False, dtype=torch.float32, B=2, T=77, steps=30):
    dev, H, W = torch.device("meta"), 32, 32
    io = UNetIO(x=torch.empty(B, 4, H, W, device=dev, dtype=dtype), timestep=torch.empty(B, device=dev), out=torch.empty(B, 4, H, W, device=dev, dtype=dtype))
    io.tokens[LLM_TOKENS] = (torch.zeros(B * ((T + 63) // 64 * 64), 2048, device=dev, dtype=dtype), T)
    if table:
        io.timesteps = torch.empty(B * steps, device=dev)
        io.step_rows = torch.zeros(B, device=dev, dtype=torch.int32)
    low = UNetLowering(dev, dtype)
    low.lower(unet, io)
    return low


def _names(ops):
    return [e[2] for e in ops if e[0] is not None]


def _gemms(ops):
    return [e[1][0]._obj for e in ops if e[2] == "mi355x_gemm"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adapted_sd1_tree_lowers_into_the_step(dtype):
    unet = SD1UNet(4, device="meta", dtype=dtype)
    adapter = SD1ELLAAdapter(unet).inject()
    layers = 6
    low = _dry(unet, dtype=dtype)
    step, pro = _names(low.step), _names(low.prologue)
    assert low.stats["fallback_nodes"] == [] and low.stats["ella_sites"] == 16 and low.stats["ella_layers"] == layers
    assert step.count("mi355x_ella_adaln") == 2 * layers and "mi355x_ella_adaln" not in pro
    assert "mi355x_gather_rows" not in step
    # prompt side: the input Linear over the LLM's tokens and nothing else -- no GEMM that reads ELLA's tokens (K = 768 from 128 rows) sits there
    assert pro == ["mi355x_gemm"] and (_gemms(low.prologue)[0].N, _gemms(low.prologue)[0].seg[0].k) == (768, 2048)
    # the time table: one launch of 18 x 1536 + 768 columns; the squared-ReLU epilogue once per layer
    width = 3 * layers * 1536 + 768
    assert sum(1 for a in _gemms(low.step) if (a.M, a.N) == (2, width)) == 1
    assert sum(1 for a in _gemms(low.step) if a.geglu == 5) == layers and not any(a.geglu == 5 for a in _gemms(low.prologue))
    # 16 cross-attentions x (K, V^T) over the 2 x 64 latent rows, in the step
    bare = _dry_bare(dtype)
    kv = [a for a in _gemms(low.step) if a.seg[0].k == 768 and (a.M == 128 or a.N == 128) and a.geglu == 0 and not a.out_t]
    assert len(_gemms(low.step)) - len(_gemms(bare.step)) == 32 + 2 + 1 + 1 + 4 * layers  # K, V^T of 16 sites | RangeEncoder | time table | latents | Q|K|V^T, out-projection, FF1, FF2 per layer
    assert len(kv) >= 32
    # the attention over [latents ; text]: Lq = 64, Lk = 64 + 77, batch strides over 192 rows
    att = [e[1][0]._obj for e in low.step if e[2] == "mi355x_attention_general" and e[1][0]._obj.Dqk == 96]
    assert len(att) == layers and all((a.Lq, a.Lk, a.H, a.causal) == (64, 141, 8, 0) and a.k_batch_stride == 192 * 1536 for a in att)
    adapter.eject()
    assert E.program_digest(_dry_bare(dtype, unet).step) == E.program_digest(bare.step)


def _dry_bare(dtype, unet=None):
    dev, B, H, W = torch.device("meta"), 2, 32, 32
    unet = unet if unet is not None else SD1UNet(4, device="meta", dtype=dtype)
    io = UNetIO(x=torch.empty(B, 4, H, W, device=dev, dtype=dtype), timestep=torch.empty(B, device=dev), out=torch.empty(B, 4, H, W, device=dev, dtype=dtype))
    io.tokens[("cross_attention_block", "clip_text_embedding")] = (torch.zeros(B * 128, 768, device=dev, dtype=dtype), 77)
    low = UNetLowering(dev, dtype)
    low.lower(unet, io)
    return low


def test_table_mode_moves_the_time_table_into_the_prologue():
    unet = SD1UNet(4, device="meta")
    SD1ELLAAdapter(unet).inject()
    low = _dry(unet, table=True)
    width = 18 * 1536 + 768
    assert [(a.M, a.N) for a in _gemms(low.prologue) if a.N == width] == [(2 * 30, width)]
    assert not any(a.N == width for a in _gemms(low.step))
    assert _names(low.step).count("mi355x_gather_rows") == 1 and _names(low.step).count("mi355x_ella_adaln") == 12
    assert _names(low.prologue).count("mi355x_sinusoidal") == 1


def test_missing_llm_embedding_and_unknown_children_are_refused():
    from refiners_amd.engine.packing import Unsupported

    import refiners_amd.fluxion.layers as fl

    unet = SD1UNet(4, device="meta")
    adapter = SD1ELLAAdapter(unet).inject()
    dev = torch.device("meta")
    io = UNetIO(x=torch.empty(2, 4, 32, 32, device=dev), timestep=torch.empty(2, device=dev), out=torch.empty(2, 4, 32, 32, device=dev))
    with pytest.raises(Unsupported, match="llm_text_embedding"):
        UNetLowering(dev, torch.float32).lower(unet, io)
    layer = adapter.latents_encoder.layer(("PerceiverResampler", "Transformer", "TransformerLayer_1"), fl.Chain)
    layer.append(fl.Identity())
    with pytest.raises(Unsupported, match="TransformerLayer"):
        _dry(unet)


@pytest.mark.parametrize("name", [f"{f}_{d}" for f, d in E.BARE_PROGRAMS])
def test_bare_programs_are_what_they_were(name):
    """The bare SD1 and SDXL trees lower op for op to the programs of the commit before ELLA (tests/golden/ella_bare_programs.json, written there by
    tools/make_golden_ella.py --bare-programs)."""
    family, dtype = name.split("_")
    want = json.loads((S.GOLD / "ella_bare_programs.json").read_text())[name]
    assert E.bare_program(family, getattr(torch, dtype)) == want


@pytest.mark.skipif(REF is None, reason="no refiners checkout (REFINERS_SRC / oracle/_ref)")
def test_reference_tree_lowers_to_the_same_program():
    sys.path[:0] = [p for p in (str(ROOT / "oracle" / "shim"), str(REF)) if p not in sys.path]
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.ella_adapter import SD1ELLAAdapter as RefAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet as RefUNet

    ref = RefUNet(4, device="meta")
    RefAdapter(ref).inject()
    assert type(ref).__module__.startswith("refiners.")
    mine = SD1UNet(4, device="meta")
    SD1ELLAAdapter(mine).inject()
    a, b = _dry(ref), _dry(mine)
    assert E.program_digest(a.step) == E.program_digest(b.step) and E.program_digest(a.prologue) == E.program_digest(b.prologue)
    assert a.stats["ella_sites"] == b.stats["ella_sites"] == 16
