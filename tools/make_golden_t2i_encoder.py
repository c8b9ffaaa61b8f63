"""Golden vectors of the T2I-Adapter's condition encoder: the REAL reference's ConditionEncoder / ConditionEncoderXL and one SD1UNet +
SD1T2IAdapter step on CPU float32, at the cases of tests/t2i_encoder_cases.py (weights drawn per key, seeded pictures).  Run where refiners'
sources are (REFINERS_SRC, else the copy __graft_entry__.build() stages under oracle/_ref/src); not on a GPU box:
    python tools/make_golden_t2i_encoder.py
Writes tests/golden/t2i_encoder.safetensors
    <case>.f<i>      feature map i of the case's encoder
    sd1_step.f<i>    the default-width SD1 encoder's features of the step's picture
    sd1_step.out     SD1UNet + SD1T2IAdapter at the step's timestep on those features, [1, 4, 16, 16]
Prints the distance of the float32 features to the reference's own float64 forward."""
from __future__ import annotations

import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")
GOLD = ROOT / "tests" / "golden"


def main() -> None:
    sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF), str(ROOT)]
    import torch
    from safetensors.torch import save_file

    import refiners.foundationals.latent_diffusion.t2i_adapter as ref_t2i
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.t2i_adapter import SD1T2IAdapter
    from refiners.foundationals.latent_diffusion.stable_diffusion_1.unet import SD1UNet

    from tests import support as S
    from tests import t2i_encoder_cases as TC

    out = {}
    for case in TC.ENCODER_CASES:
        enc = TC.encoder(case, ref_t2i)
        assert type(enc).__module__.startswith("refiners.")
        x = TC.picture(case)
        with torch.no_grad():
            feats = enc(x)
            feats64 = enc.to(dtype=torch.float64)(x.double())
        for i, (f, f64) in enumerate(zip(feats, feats64)):
            out[f"{case}.f{i}"] = f.contiguous()
            print(case, i, tuple(f.shape), f"rms {float(f.pow(2).mean().sqrt()):.3f}; float32 against float64: %.2e %.2e" % S.rel_err(f, f64))
    unet = SD1UNet(4, device="meta")
    unet.load_state_dict({k: v.clone() for k, v in S.weights("sd1", TC.SD1_STEP["unet_seed"]).items()}, assign=True)
    adapter = TC.sd1_adapter(unet, SD1T2IAdapter)
    with torch.no_grad():
        feats = adapter.compute_condition_features(TC.sd1_inputs()["picture"])
    for i, f in enumerate(feats):
        out[f"sd1_step.f{i}"] = f.contiguous()
    out["sd1_step.out"] = TC.sd1_run(unet, tuple(feats)).contiguous()
    adapter.eject()
    print("sd1_step against the ejected tree: relative difference %.3e %.3e" % S.rel_err(out["sd1_step.out"], TC.sd1_run(unet, None)))
    save_file(out, str(GOLD / "t2i_encoder.safetensors"))
    print("t2i_encoder.safetensors", (GOLD / "t2i_encoder.safetensors").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
