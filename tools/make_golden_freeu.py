"""Golden vectors of FreeU: the REAL reference's SD1UNet / SDXLUNet and latent_diffusion.freeu.SDFreeUAdapter on CPU float32, at the cases of
tests/freeu_cases.py (bare weights as `sd1_bare` / `sdxl_bare` draw them, seeded inputs).  Run where refiners' sources are (REFINERS_SRC, else the
copy __graft_entry__.build() stages under oracle/_ref/src); not on a GPU box:
    python tools/make_golden_freeu.py
Writes tests/golden/freeu.safetensors
    <case>.unet_out.t<i>   the UNet's output [2, 4, H, W] at the case's i-th timestep (SDXL: at DDIM step `step`)
    sdxl.x_next            that DDIM step from the case's latents, the CFG pair combined at the case's condition scale
and tests/golden/freeu_keys.json: per family the digest of the injected adapter's repr on the meta device and its state-dict keys."""
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


def main() -> None:
    sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF), str(ROOT)]
    import torch
    from safetensors.torch import save_file

    import refiners.fluxion.layers as rfl
    from refiners.fluxion.adapters.lora import Conv2dLora, LinearLora, LoraAdapter
    from refiners.foundationals.latent_diffusion.freeu import SDFreeUAdapter
    from refiners.foundationals.latent_diffusion.solvers.ddim import DDIM
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet
    from refiners.foundationals.latent_diffusion.stable_diffusion_xl.unet import SDXLUNet

    from tests import freeu_cases as P
    from tests import support as S

    t0 = time.time()
    api = SimpleNamespace(fl=rfl, LinearLora=LinearLora, Conv2dLora=Conv2dLora, LoraAdapter=LoraAdapter, SDFreeUAdapter=SDFreeUAdapter)
    unets = {"sd1": SD1UNet, "sdxl": SDXLUNet}
    out, keys = {}, {}
    for case, c in P.CASES.items():
        fam = c["family"]
        unet = unets[fam](4, device="meta")
        unet.load_state_dict({k: v.clone() for k, v in S.weights(fam, c["weight_seed"]).items()}, assign=True)
        adapter = P.inject(unet, api, case, S.key_shapes(fam))
        assert type(adapter).__module__.startswith("refiners.")
        if fam == "sdxl":
            solver = DDIM(num_inference_steps=c["num_steps"])
            y = P.run_chain(unet, case, float(solver.timesteps[c["step"]]))
            u, cnd = y.chunk(2)
            out[f"{case}.unet_out.t0"] = y.contiguous()
            out[f"{case}.x_next"] = solver(P.inputs(case)["x"], predicted_noise=u + c["condition_scale"] * (cnd - u), step=c["step"]).contiguous()
        else:
            for i, ts in enumerate(c["timesteps"]):
                out[f"{case}.unet_out.t{i}"] = P.run_chain(unet, case, ts).contiguous()
        print(case, f"rms {float(out[f'{case}.unet_out.t0'].pow(2).mean().sqrt()):.3f}")
        if "lora_rank" not in c:
            meta = P.inject(unets[fam](4, device="meta"), api, case, S.key_shapes(fam), device="meta")
            keys[fam] = {"repr_sha256": P.repr_digest(meta), "state_dict": list(adapter.state_dict())}
            adapter.eject()
            ts = float(solver.timesteps[c["step"]]) if fam == "sdxl" else c["timesteps"][0]
            print(case, "against the ejected tree: relative difference %.3e %.3e" % S.rel_err(out[f"{case}.unet_out.t0"], P.run_chain(unet, case, ts)))
        del unet
    (GOLD / "freeu_keys.json").write_text(json.dumps(keys))
    save_file(out, str(GOLD / "freeu.safetensors"))
    print("freeu.safetensors", (GOLD / "freeu.safetensors").stat().st_size, "bytes,", f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
