"""Golden vectors of IP-Adapter on SD1.5: the REAL reference's SD1UNet and stable_diffusion_1.image_prompt.SD1IPAdapter on CPU float32, at the
cases of tests/sd1_ip_cases.py (bare weights as `sd1_bare` draws them, seeded inputs and image tokens).  Run where refiners' sources are
(REFINERS_SRC, else the copy __graft_entry__.build() stages under oracle/_ref/src); not on a GPU box:
    python tools/make_golden_sd1_ip.py
Writes tests/golden/sd1_ip.safetensors
    <case>.tokens        the image tokens [2, n, 768] the adapter's context held ([negative ; conditional])
    <case>.unet_out.t<i> the UNet's output [2, 4, 32, 32] at the case's i-th timestep
    lora.unet_out.rescaled   case "lora" after `adapter.scale = rescale`
    plain.x_next         one DPM-Solver++ step (SOLVER) from the shared latents: the CFG pair combined, then the solver's update
    x, text              the inputs every case shares
and tests/golden/sd1_ip_keys.json: per variant ("plain", "plus") the digest of the adapter's repr on the meta device, the state-dict keys of the injected adapter and of its image projection."""
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
    from refiners.foundationals.clip.image_encoder import CLIPImageEncoderH
    from refiners.foundationals.latent_diffusion.solvers import DPMSolver
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.image_prompt import SD1IPAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet

    from tests import sd1_ip_cases as P
    from tests import support as S

    t0 = time.time()
    api = SimpleNamespace(fl=rfl, LinearLora=LinearLora, Conv2dLora=Conv2dLora, LoraAdapter=LoraAdapter, SD1IPAdapter=SD1IPAdapter)
    shapes = S.key_shapes("sd1")
    inp = P.inputs("plain")
    out, keys = {"x": inp["x"], "text": inp["text"]}, {}
    for case, c in P.CASES.items():
        unet = SD1UNet(4, device="meta")
        unet.load_state_dict({k: v.clone() for k, v in S.weights("sd1", P.UNET["weight_seed"]).items()}, assign=True)
        adapter = P.inject(unet, api, case, shapes, encoder=CLIPImageEncoderH(device="meta"))  # (the encoder is only asked for its widths)
        assert type(adapter).__module__.startswith("refiners.")
        out[f"{case}.tokens"] = P.inputs(case)["tokens"]
        for i, ts in enumerate(c["timesteps"]):
            out[f"{case}.unet_out.t{i}"] = P.run_chain(unet, case, ts).contiguous()
            print(case, i, f"rms {float(out[f'{case}.unet_out.t{i}'].pow(2).mean().sqrt()):.3f}")
        if "rescale" in c:
            adapter.scale = c["rescale"]
            out[f"{case}.unet_out.rescaled"] = P.run_chain(unet, case, c["timesteps"][0]).contiguous()
            print(case, "rescaled: relative difference %.3e %.3e" % S.rel_err(out[f"{case}.unet_out.rescaled"], out[f"{case}.unet_out.t0"]))
        if case == "plain":
            solver = DPMSolver(P.SOLVER["num_steps"])
            s, cs = P.SOLVER["step"], P.SOLVER["condition_scale"]
            u, cnd = P.run_chain(unet, case, float(solver.timesteps[s])).chunk(2)
            out["plain.x_next"] = solver(inp["x"], predicted_noise=u + cs * (cnd - u), step=s).contiguous()
        if case in ("plain", "plus"):
            meta = P.inject(SD1UNet(4, device="meta"), api, case, shapes, device="meta", encoder=CLIPImageEncoderH(device="meta"))
            keys[case] = {"repr_sha256": P.repr_digest(meta), "state_dict": list(adapter.state_dict()), "image_proj": list(adapter.image_proj.state_dict())}
            adapter.eject()
            bare = P.run_chain(unet, case, c["timesteps"][0])
            print(case, "against the ejected tree: relative difference %.3e %.3e" % S.rel_err(out[f"{case}.unet_out.t0"], bare))
    (GOLD / "sd1_ip_keys.json").write_text(json.dumps(keys))
    save_file(out, str(GOLD / "sd1_ip.safetensors"))
    print("sd1_ip.safetensors", (GOLD / "sd1_ip.safetensors").stat().st_size, "bytes,", f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
