"""What FreeU costs on the MI355X.  SDXL at 1024 x 1024 (128 x 128 latents), bfloat16, CFG pair, DDIM(30), synthetic weights, ONE process, the
variants alternating, every variant warmed first, device events around the timed calls:
    bare        CompiledSDXL.step of the UNet without the adapter
    freeu_on    ... with SDFreeUAdapter(backbone_scales=[1.2, 1.4], skip_scales=[0.9, 0.2]) lowered under REFINERS_AMD_FREEU=1
    freeu_off   ... the same tree lowered without the switch: refused, the stock Chain forward (what ran before the adapter was lowered)
    launch      mi355x_freeu_filter alone at a site's shape (2 images x 32 x 32 pixels, 1280 skip and 1280 backbone channels; both sites have it), as
                captured graphs of REPS calls, for each slab width (16 / 32 / 64 channels per workgroup) and as the library picks it
Every figure is the median of three repeats, with their minimum and maximum beside it.  Needs a GPU (no fallback).
    python tools/probe_freeu.py --json profiles/freeu_probe.json"""
import argparse
import json
import os
import sys
import warnings
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import native, synth  # noqa: E402
from refiners_amd.engine import freeu  # noqa: E402
from refiners_amd.engine.compiled import CompiledSDXL  # noqa: E402
from refiners_amd.latent_diffusion.freeu import SDFreeUAdapter  # noqa: E402
from refiners_amd.latent_diffusion.sdxl import SDXLUNet  # noqa: E402

REPS = 20
stat = lambda v: {"median": round(sorted(v)[len(v) // 2], 3), "min_max": [round(min(v), 3), round(max(v), 3)]}  # noqa: E731


def events_us(fn, iters, per):
    """Microseconds per unit of work: `fn` holds `per` units and runs `iters` times between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (iters * per)


def launch_point(dev, iters, dt):
    B, H, W, C = 2, 32, 32, 1280
    g = torch.Generator().manual_seed(1)
    skip, bb = torch.randn(B * H * W, C, generator=g).to(dev, dt), torch.randn(B * H * W, C, generator=g).to(dev, dt)
    out = torch.empty_like(skip)
    A, S, R = freeu.tables(H, W, 0.2, device=dev)
    lib, forms = native.load(), {}
    for slab in (0, 16, 32, 64):  # (the width is read when the call is made, i.e. when the graph is captured)
        lib.mi355x_freeu_set_slab(slab)
        ops = []
        with native.recording(ops):
            for _ in range(REPS):
                native.freeu_filter(skip, out, bb, B, A, S, R, 1.0)  # (scale 1: the timed replays leave the backbone's values alone)
        native.replay(ops)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            native.replay(ops)
        forms[f"slab_{slab or 'auto'}"] = graph.replay
    lib.mi355x_freeu_set_slab(0)
    runs = {name: [] for name in forms}
    for _ in range(3):
        for name, fn in forms.items():
            runs[name].append(events_us(fn, iters, REPS))
    moved = 3 * skip.numel() * skip.element_size() + 2 * (bb.numel() // 2) * bb.element_size()  # skip read twice and written, the backbone's half read and written
    row = {"shape": [B, H, W, C, C], "dtype": str(dt).split(".")[1], "bytes_moved": moved, "workgroups": {s: B * -(-C // s) for s in (16, 32, 64)},
           "us_per_launch": {name: stat(v) for name, v in runs.items()}}
    print(json.dumps(row), flush=True)
    return row


def step_point(dev, iters, latent):
    dt, steps = torch.bfloat16, 30
    bare, adapted = SDXLUNet(4, device="meta"), SDXLUNet(4, device="meta")
    sd = {k: v.to(device=dev, dtype=dt) for k, v in synth.synth_state_dict(synth.model_shapes(bare), 0).items()}
    bare.load_state_dict(sd, assign=True)
    adapted.load_state_dict(sd, assign=True)  # (the same storage)
    SDFreeUAdapter(target=adapted, backbone_scales=[1.2, 1.4], skip_scales=[0.9, 0.2]).inject()
    inp = {k: v.to(dev) for k, v in synth.sdxl_inputs(1, (latent, latent), 3).items()}
    pipes, outs = {}, {}
    for which, unet, flag in (("bare", bare, "0"), ("freeu_on", adapted, "1"), ("freeu_off", adapted, "0")):
        os.environ["REFINERS_AMD_FREEU"] = flag  # read while the tree is lowered; a program keeps the form it was lowered with
        p = pipes[which] = CompiledSDXL(unet, num_inference_steps=steps, condition_scale=5.0)
        p.set_inputs(inp["x"].to(dt), clip_text_embedding=inp["text"].to(dt), pooled_text_embedding=inp["pooled"].to(dt), time_ids=inp["time_ids"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for _ in range(3):
                outs[which] = p.step(3).float().clone()
    os.environ.pop("REFINERS_AMD_FREEU")
    st = {w: p.engine.stats for w, p in pipes.items()}
    assert st["freeu_on"].get("freeu_sites") == 2 and st["freeu_on"]["fallback_nodes"] == [] and st["freeu_off"].get("whole_fallback"), "the path asked for did not run"
    runs = {which: [] for which in pipes}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for _ in range(3):
            for which, p in pipes.items():
                runs[which].append(events_us(lambda p=p: p.step(3), iters, 1) / 1e3)
    names = lambda p: [e[2] for e in p.engine.low.step if e[0] is not None]  # noqa: E731
    count = lambda p: {n: names(p).count(n) for n in sorted(set(names(p))) if "groupnorm" in n or "freeu" in n}  # noqa: E731
    diff = outs["freeu_on"] - outs["freeu_off"]
    row = {"latent": latent, "dtype": "bfloat16", "solver": f"DDIM({steps})", "step_ms": {w: stat(v) for w, v in runs.items()},
           "step_launches": {w: st[w]["step_ops"] for w in ("bare", "freeu_on")}, "groupnorm_and_freeu_launches": {w: count(pipes[w]) for w in ("bare", "freeu_on")},
           "gn_from_producer": {w: st[w].get("gn_from_producer", 0) for w in ("bare", "freeu_on")},
           "on_vs_off_x_next": {"rel_l2": float(diff.norm() / outs["freeu_off"].norm()), "max_rel": float(diff.abs().max() / outs["freeu_off"].abs().max())}}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_freeu needs a GPU"
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "launch": [launch_point(dev, a.iters, dt) for dt in (torch.bfloat16, torch.float32)]}
    if not a.no_step:
        res["sdxl_step"] = step_point(dev, max(3, a.iters // 2), a.latent)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
