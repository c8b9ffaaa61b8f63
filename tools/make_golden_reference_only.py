"""Golden vectors of reference-only control: the REAL reference's SD1UNet + ReferenceOnlyControlAdapter on CPU float32 with the synthetic
weights of refiners_amd.synth (tests/support.weights("sd1", 0)) and the seeded inputs of tests/reference_only_cases.py.  Run where refiners'
sources are (REFINERS_SRC, else the copy __graft_entry__.build() stages under oracle/_ref/src); not on a GPU box:
    python tools/make_golden_reference_only.py
Writes tests/golden/reference_only.safetensors, reference_only.1.safetensors, ... (outputs only, [2, 4, H, W] each; shards as
tests/support.golden reads them); the keys are listed in tests/reference_only_cases.py."""
from __future__ import annotations

import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")
GOLD = ROOT / "tests" / "golden"
SHARD_BYTES = 700_000


def main() -> None:
    sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF), str(ROOT)]
    import torch
    from safetensors.torch import save_file

    import refiners.fluxion.layers as rfl
    from refiners.fluxion.adapters.lora import Conv2dLora, LinearLora, LoraAdapter
    from refiners.foundationals.latent_diffusion.reference_only_control import ReferenceOnlyControlAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet

    from tests import reference_only_cases as R
    from tests import support as S

    t0 = time.time()
    out = {}

    def tree(lora: bool = False):
        unet = SD1UNet(4, device="meta")
        unet.load_state_dict({k: v.clone() for k, v in S.weights("sd1", R.SEED["weight_seed"]).items()}, assign=True)
        if lora:  # before the adapter is built: its structural copies then carry the LoRAs
            from types import SimpleNamespace

            R.add_lora(unet, SimpleNamespace(fl=rfl, LinearLora=LinearLora, Conv2dLora=Conv2dLora, LoraAdapter=LoraAdapter), S.key_shapes("sd1"))
        return unet, ReferenceOnlyControlAdapter(unet).inject()

    unet, adapter = tree()
    for case, cfg in R.CASES.items():
        for i, ts in enumerate(cfg["timesteps"]):
            out[f"{case}.t{i}"] = R.run(unet, adapter, case, ts)
    ts = R.CASES["main"]["timesteps"][0]
    for key, style in R.STYLES.items():
        for sub in adapter.sub_adapters:
            sub.style_cfg = style
        out[f"main.{key}"] = R.run(unet, adapter, "main", ts)
    adapter.eject()
    out["main.bare"] = R.run(unet, None, "main", ts)
    unet, adapter = tree(lora=True)
    out["main.lora"] = R.run(unet, adapter, "main", ts)

    for k, v in out.items():
        assert torch.isfinite(v).all()
        print(k, tuple(v.shape), f"rms {float(v.pow(2).mean().sqrt()):.3f}")
    for a, b in (("main.t0", "main.t1"), ("main.t0", "main.s1"), ("main.t0", "main.s0"), ("main.t0", "main.bare"), ("main.t0", "main.lora")):
        print(a, b, "relative difference %.3e %.3e" % S.rel_err(out[b], out[a]))
    print("rows of main.t0 differ by %.3e" % float((out["main.t0"][0] - out["main.t0"][1]).abs().max()))

    for old in GOLD.glob("reference_only*.safetensors"):
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
        path = GOLD / ("reference_only.safetensors" if i == 0 else f"reference_only.{i}.safetensors")
        save_file(sh, str(path))
        print(path.name, path.stat().st_size, "bytes")
    print(f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
