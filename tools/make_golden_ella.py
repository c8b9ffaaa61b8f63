"""Golden vectors of the ELLA text connector: the REAL reference's foundationals.latent_diffusion.ella_adapter classes on CPU float32 with the
synthetic per-key weights of tests/ella_cases.py (AdaLayerNorm Linears drawn non-zero: the reference zero-initialises them, which would hide
the modulation) and seeded inputs.  Run where refiners' sources are (REFINERS_SRC, else the copy __graft_entry__.build() stages under
oracle/_ref/src); not on a GPU box:
    python tools/make_golden_ella.py
Writes tests/golden/ella_keys.json (per case, and for SD1ELLAAdapter's own 6-layer encoder "sd1_full", the state-dict keys, in order, with
their shapes) and tests/golden/ella.safetensors, ella.1.safetensors, ... (outputs only; shards as tests/support.golden reads them, each below
the size of the largest fixture already committed):
    <case>.t<i>     ella.latents [B, Nl, width'] of ELLA_CASES[case] at its i-th timestep
    unet.t<i>       SD1UNet + SD1ELLAAdapter of UNET_CASE at its i-th timestep, [B, 4, H, W]
    unet.llm2       the same at timestep 0 with another LLM embedding
    unet.lora       the same at timestep 0 with a LoRA on the cross-attention K / V Linears
`--bare-programs` writes tests/golden/ella_bare_programs.json instead: the digests of the bare SD1 / SDXL programs (dry lowerings) of the
commit it runs on -- run it on the commit whose programs are to be pinned."""
from __future__ import annotations

import json
import os
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")
GOLD = ROOT / "tests" / "golden"
SHARD_BYTES = 700_000


def bare_programs() -> None:
    sys.path[:0] = [str(ROOT)]
    import torch

    from tests.ella_cases import BARE_PROGRAMS, bare_program

    out = {f"{family}_{dtype}": bare_program(family, getattr(torch, dtype)) for family, dtype in BARE_PROGRAMS}
    (GOLD / "ella_bare_programs.json").write_text(json.dumps(out, indent=1))
    print({k: (v["step"]["launches"], v["prologue"]["launches"]) for k, v in out.items()})


def main() -> None:
    sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF), str(ROOT)]
    import torch
    from safetensors.torch import save_file

    import refiners.fluxion.layers as rfl
    from refiners.fluxion.adapters.lora import Conv2dLora, LinearLora, LoraAdapter
    from refiners.foundationals.latent_diffusion.ella_adapter import ELLA
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.ella_adapter import SD1ELLAAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet

    from refiners_amd import synth
    from tests import support as S
    from tests.ella_cases import ELLA_CASES, UNET_CASE, draw_weights, llm_embedding, run_tree, timestep, unet_inputs, unet_lora_targets

    t0 = time.time()
    keys, out = {}, {}
    for name, case in ELLA_CASES.items():
        model = ELLA(**case["model"])
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        keys[name] = {k: list(v) for k, v in shapes.items()}
        model.load_state_dict(draw_weights(shapes, name))
        llm = llm_embedding(name)
        for i, ts in enumerate(case["timesteps"]):
            y = run_tree(model, ts, llm)
            m = case["model"]
            assert tuple(y.shape) == (case["batch"], m["num_latents"], m.get("out_dim") or m["width"]) and torch.isfinite(y).all()
            out[f"{name}.t{i}"] = y.contiguous()
            print(name, i, tuple(y.shape), f"rms {float(y.pow(2).mean().sqrt()):.3f}")

    c = UNET_CASE
    unet = SD1UNet(4, device="meta")
    unet.load_state_dict({k: v.clone() for k, v in S.weights("sd1", c["unet_weight_seed"]).items()}, assign=True)
    adapter = SD1ELLAAdapter(unet)
    shapes = {k: tuple(v.shape) for k, v in adapter.latents_encoder.state_dict().items()}
    keys["sd1_full"] = {k: list(v) for k, v in shapes.items()}
    adapter.latents_encoder.load_state_dict(draw_weights(shapes, "sd1_full"))
    adapter.inject()
    inp = unet_inputs()

    def run(ts: float, llm: "torch.Tensor") -> "torch.Tensor":
        adapter.set_llm_text_embedding(llm)
        unet.set_timestep(timestep(ts))
        with torch.no_grad():
            return unet(inp["x"]).contiguous()

    for i, ts in enumerate(c["timesteps"]):
        out[f"unet.t{i}"] = run(ts, inp["llm"])
        print("unet", i, f"rms {float(out[f'unet.t{i}'].pow(2).mean().sqrt()):.3f}")
    out["unet.llm2"] = run(c["timesteps"][0], unet_inputs(shift=1)["llm"])
    ushapes = S.key_shapes("sd1")
    spec = synth.lora_spec(ushapes, "ella_kv", c["lora_scale"], rank=c["lora_rank"], seed=3, targets=unet_lora_targets(ushapes))
    assert len(spec["pairs"]) == 32
    synth.apply_adapters(unet, SimpleNamespace(fl=rfl, LinearLora=LinearLora, Conv2dLora=Conv2dLora, LoraAdapter=LoraAdapter), loras=[spec])
    out["unet.lora"] = run(c["timesteps"][0], inp["llm"])
    for a, b in (("unet.t0", "unet.t1"), ("unet.t0", "unet.llm2"), ("unet.t0", "unet.lora")):
        print(a, b, "relative difference %.3e %.3e" % S.rel_err(out[b], out[a]))

    (GOLD / "ella_keys.json").write_text(json.dumps(keys))
    for old in GOLD.glob("ella*.safetensors"):
        old.unlink()
    shards: list[dict] = [{}]
    size = 0
    for k, v in out.items():
        n = v.numel() * v.element_size()
        if size + n > SHARD_BYTES and shards[-1]:
            shards.append({})
            size = 0
        shards[-1][k] = v
        size += n
    for i, sh in enumerate(shards):
        path = GOLD / ("ella.safetensors" if i == 0 else f"ella.{i}.safetensors")
        save_file(sh, str(path))
        print(path.name, path.stat().st_size, "bytes")
    print(f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    bare_programs() if "--bare-programs" in sys.argv else main()
