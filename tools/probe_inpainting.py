"""SD1.5 inpainting timing at 512 x 512 (64 x 64 latents), classifier-free-guidance pair, bfloat16, 77 CLIP tokens, DPM-Solver++, synthetic weights
(refiners_amd.synth).  In ONE process:
    native_step    CompiledSDXL.step on SD1UNet(9) with `input_condition` (mask + masked-picture latents, 5 channels): one HIP-graph replay whose last
                   launch is mi355x_cond_step
    bare_step      the same engine class on SD1UNet(4) without input_condition (last launch: mi355x_cfg_linear_step): what the step cost before
    stock_chain    the mirror pipeline's stock Chain forward (StableDiffusion_1_Inpainting.__call__ in torch) on the 9-channel tree
the three alternating, three repeats each, every path warmed first; times are a host clock around work that ends in a device synchronise; the
spread of the repeats is written beside every median.  Then the conditions of a run, picture and mask already on the device as uint8:
    compiled_conditions   CompiledInpaintConditions (mi355x_inpaint_conditions + the lowered VAE encoder)
    torch_conditions      the reference's sequence of torch operations + lda.encode through the stock Chain forward
Needs a GPU (no fallback).
    python tools/probe_inpainting.py --json profiles/inpainting_probe.json"""
import argparse
import json
import sys
import time
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import synth  # noqa: E402
from refiners_amd.engine.compiled import CompiledSDXL  # noqa: E402
from refiners_amd.engine.image_conditioned import CompiledInpaintConditions  # noqa: E402
from refiners_amd.latent_diffusion import SD1Autoencoder, StableDiffusion_1_Inpainting  # noqa: E402
from refiners_amd.latent_diffusion.sd1 import SD1UNet  # noqa: E402
from refiners_amd.latent_diffusion.solvers import DPMSolver  # noqa: E402


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def build(channels, dev, dt):
    unet = SD1UNet(channels, device="meta")
    sd = synth.synth_state_dict(synth.model_shapes(unet), 0)
    unet.load_state_dict({k: v.to(device=dev, dtype=dt) for k, v in sd.items()}, assign=True)
    return unet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_inpainting needs a GPU"
    dev, dt, L = torch.device("cuda"), torch.bfloat16, a.latent
    g = torch.Generator().manual_seed(1)
    unet9, unet4 = build(9, dev, dt), build(4, dev, dt)
    x = torch.randn((1, 4, L, L), generator=g).to(dev, dt)
    clip = torch.randn((2, 77, 768), generator=g).to(dev, dt)
    mask_latents = (torch.rand((1, 1, L, L), generator=g) > 0.6).to(dev, dt)
    target_latents = (torch.randn((1, 4, L, L), generator=g) * 0.8).to(dev, dt)
    cond = torch.cat((mask_latents, target_latents), dim=1)
    steps = 30
    native = CompiledSDXL(unet9, solver=DPMSolver(steps, device=dev), condition_scale=7.5)
    bare = CompiledSDXL(unet4, solver=DPMSolver(steps, device=dev), condition_scale=7.5)
    native.set_inputs(x, clip_text_embedding=clip, input_condition=cond)
    bare.set_inputs(x, clip_text_embedding=clip)
    pipe = StableDiffusion_1_Inpainting(unet=unet9, solver=DPMSolver(steps, device=dev, dtype=dt))
    pipe.mask_latents, pipe.target_image_latents = mask_latents, target_latents

    def stock():
        with torch.no_grad():
            return pipe(x, step=3, clip_text_embedding=clip, condition_scale=7.5)

    x_native = native.step(0).clone()
    bare.step(0)
    with torch.no_grad():
        x_stock = pipe(x, step=0, clip_text_embedding=clip, condition_scale=7.5)
    apart = float((x_native.float() - x_stock.float()).norm() / x_stock.float().norm())
    assert native.engine.stats["fallback_nodes"] == [] and bare.engine.stats["fallback_nodes"] == [], "the native path did not run"
    for _ in range(3):  # warm every path: the second step captures the graph
        native.step(3), bare.step(3), stock()
    runs = []
    for _ in range(3):
        runs.append((timeit(lambda: native.step(3), a.iters), timeit(lambda: bare.step(3), a.iters), timeit(stock, max(a.iters // 5, 3))))
    med = lambda r, i: sorted(v[i] for v in r)[1]  # noqa: E731
    span = lambda r, i: [round(min(v[i] for v in r), 3), round(max(v[i] for v in r), 3)]  # noqa: E731
    kn = Counter(op[2] for op in native.engine.low.step if op[0] is not None)
    kb = Counter(op[2] for op in bare.engine.low.step if op[0] is not None)

    # the conditions of a run: a 512 x 512 picture and mask, uint8, on the device
    H = 8 * L
    lda = SD1Autoencoder(device="meta")
    lda.load_state_dict({k: v.to(device=dev, dtype=dt) for k, v in synth.synth_state_dict(synth.model_shapes(lda), 0).items()}, assign=True)
    image = torch.randint(0, 256, (H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    mask = (torch.randint(0, 2, (H, H), generator=g, dtype=torch.uint8) * 255).to(dev)
    compiled = CompiledInpaintConditions(lda)

    def compiled_conditions():
        return compiled(image, mask, latents_size=(L, L))

    def torch_conditions():  # stable_diffusion_1/model.py:259-286 behind the PIL conversion
        with torch.no_grad():
            m = ((mask.float() / 255.0) > 0.5)[None, None].to(dt)
            ml = torch.nn.functional.interpolate(m, size=(L, L), mode="nearest")
            t = (image.float() / 255.0).to(dt).permute(2, 0, 1)[None] * 2 - 1
            return ml, lda.encode(t * (1 - m))

    (ml_c, tl_c), (ml_t, tl_t) = compiled_conditions(), torch_conditions()
    assert torch.equal(ml_c, ml_t)
    cond_apart = float((tl_c.float() - tl_t.float()).norm() / tl_t.float().norm())
    for _ in range(2):
        compiled_conditions(), torch_conditions()
    cruns = [(timeit(compiled_conditions, max(a.iters // 3, 5)), timeit(torch_conditions, max(a.iters // 3, 5))) for _ in range(3)]
    res = {
        "device": torch.cuda.get_device_name(0), "shape": {"images": 1, "cfg_pair": True, "latent": L, "clip_tokens": 77, "dtype": "bfloat16", "solver": "DPMSolver(30)"},
        "iters": a.iters,
        "native_step_ms": round(med(runs, 0), 3), "native_step_ms_min_max": span(runs, 0),
        "bare_step_ms": round(med(runs, 1), 3), "bare_step_ms_min_max": span(runs, 1),
        "stock_chain_ms": round(med(runs, 2), 3), "stock_chain_ms_min_max": span(runs, 2),
        "native_over_bare": round(med(runs, 0) / med(runs, 1), 4), "speedup_over_stock_chain": round(med(runs, 2) / med(runs, 0), 2),
        "step_launches": {"native": native.engine.stats["step_ops"] + 1, "bare": bare.engine.stats["step_ops"] + 1},  # (+ the solver update)
        "native_by_kernel": dict(sorted(kn.items())), "bare_by_kernel": dict(sorted(kb.items())),
        "native_vs_stock_relative_l2_step0": round(apart, 5),
        "compiled_conditions_ms": round(med(cruns, 0), 3), "compiled_conditions_ms_min_max": span(cruns, 0),
        "torch_conditions_ms": round(med(cruns, 1), 3), "torch_conditions_ms_min_max": span(cruns, 1),
        "conditions_speedup": round(med(cruns, 1) / med(cruns, 0), 2), "conditions_relative_l2": round(cond_apart, 5),
    }
    print(json.dumps(res, indent=1))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
