"""What IP-Adapter on SD1.5 costs per step, and what mi355x_attention_streams changes: SD1.5 at 512 x 512 (64 x 64 latents), classifier-free-guidance
pair, bfloat16, 77 CLIP tokens, DPMSolver(30), synthetic weights (refiners_amd.synth), SD1IPAdapter plain (4 image tokens) and plus (16).  In ONE
process, per adapter variant:
    fused       CompiledSDXL.step with every cross-attention site as one mi355x_attention_streams launch
    unfused     the same tree lowered with the switch off (REFINERS_AMD_ATTN_STREAMS=0's form): two mi355x_attention_general launches + mi355x_axpby per site
    bare        the UNet without the adapter
    chain       the stock Chain forward of the adapted tree on torch (one UNet call on the pair; no solver update)
the engine paths alternating, three repeats each, every path warmed first (the second step captures the graph); times are a host clock around work
that ends in a device synchronise; the spread of the repeats is written beside every median.
Then per kernel, at SD1.5's cross-attention shapes (B = 2, 8 heads), each side as a captured graph of REPS launches (or launch triples) replayed:
    streams     mi355x_attention_streams over text + image keys
    general     mi355x_attention_general (text), mi355x_attention_general (image, into scratch), mi355x_axpby
and, for information, the one-stream 77-key shapes: mi355x_attention_streams against mi355x_attention_general.
Needs a GPU (no fallback).
    python tools/probe_sd1_ip.py --json profiles/sd1_ip_probe.json"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import refiners_amd  # noqa: E402
from refiners_amd import native, synth  # noqa: E402
from refiners_amd.engine import lowering_blocks  # noqa: E402
from refiners_amd.engine.compiled import CompiledSDXL  # noqa: E402
from refiners_amd.latent_diffusion.adapters import SD1IPAdapter  # noqa: E402
from refiners_amd.latent_diffusion.sd1 import SD1UNet  # noqa: E402
from refiners_amd.latent_diffusion.solvers import DPMSolver  # noqa: E402

REPS = 50
med = lambda r, i: sorted(v[i] for v in r)[len(r) // 2]  # noqa: E731
span = lambda r, i: [round(min(v[i] for v in r), 4), round(max(v[i] for v in r), 4)]  # noqa: E731


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def graph_of(emit):
    """REPS times what `emit` launches, recorded and captured: a callable that replays the graph."""
    ops = []
    with native.recording(ops):
        for _ in range(REPS):
            emit()
    native.replay(ops)  # warm: code objects, attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        native.replay(ops)
    return g.replay


def kernel_points(dev, dt, iters):
    out = []
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    for D, Lq in ((40, 4096), (80, 1024), (160, 256), (160, 64)):
        for img in (4, 16, 0):
            B, H = 2, 8
            C_ = H * D
            q, o, scratch = rnd(B, Lq, C_), torch.empty(B, Lq, C_, device=dev, dtype=dt), torch.empty(B, Lq, C_, device=dev, dtype=dt)
            streams = [(rnd(B, 128, C_), rnd(C_, B, 128), 77, 1.0)] + ([(rnd(B, 64, C_), rnd(C_, B, 64), img, 0.6)] if img else [])

            def general():
                for i, (k, vt, Lk, osc) in enumerate(streams):
                    native.attention_general(q, k, vt, scratch if i else o, H, Lk, out_scale=osc)
                    if i:
                        native.axpby(o.view(-1, C_), 1.0, scratch.view(-1, C_), 1.0, o.view(-1, C_))

            fused, parent = graph_of(lambda: native.attention_streams(q, o, H, streams)), graph_of(general)
            runs = [(timeit(fused, iters) / REPS * 1e3, timeit(parent, iters) / REPS * 1e3) for _ in range(3)]
            out.append({"D": D, "Lq": Lq, "keys": [77, img] if img else [77], "streams_us": round(med(runs, 0), 3), "streams_us_min_max": span(runs, 0),
                        "general_us": round(med(runs, 1), 3), "general_us_min_max": span(runs, 1), "general_over_streams": round(med(runs, 1) / med(runs, 0), 3)})
            print(out[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_sd1_ip needs a GPU"
    dev, dt, L, steps = torch.device("cuda"), torch.bfloat16, a.latent, 30
    g = torch.Generator().manual_seed(1)
    x = torch.randn((1, 4, L, L), generator=g).to(dev, dt)
    clip = torch.randn((2, 77, 768), generator=g).to(dev, dt)

    def make_unet():
        unet = SD1UNet(4, device="meta")
        shapes = synth.model_shapes(unet)
        unet.load_state_dict({k: v.to(device=dev, dtype=dt) for k, v in synth.synth_state_dict(shapes, 0).items()}, assign=True)
        return unet, shapes

    bare_unet, shapes = make_unet()
    bare = CompiledSDXL(bare_unet, solver=DPMSolver(steps), condition_scale=7.5)
    bare.set_inputs(x, clip_text_embedding=clip)
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "kernel_reps_per_graph": REPS,
           "shape": {"images": 1, "cfg_pair": True, "latent": L, "clip_tokens": 77, "dtype": "bfloat16", "solver": f"DPMSolver({steps})"}}
    for name, fine, nt in (("plain", False, 4), ("plus", True, 16)):
        unet, _ = make_unet()
        ad = SD1IPAdapter(target=unet, clip_image_encoder=synth._NoImageEncoder(), scale=0.6, fine_grained=fine)
        for sub, (wk, wv) in zip(ad.sub_adapters, synth.ip_spec(shapes, 0.6, batch=2, num_tokens=nt, seed=5)["kv"].values()):
            sub.image_key_projection.weight = torch.nn.Parameter(wk.to(dev, dt))
            sub.image_value_projection.weight = torch.nn.Parameter(wv.to(dev, dt))
        ad.inject()
        tokens = torch.randn((2, nt, 768), generator=g).to(dev, dt)
        pipes, first = {}, {}
        for which, on in (("fused", True), ("unfused", False)):
            lowering_blocks.ATTN_STREAMS = on  # the switch the environment variable sets at import; a program keeps the form it was lowered with
            p = pipes[which] = CompiledSDXL(unet, solver=DPMSolver(steps), condition_scale=7.5)
            p.set_inputs(x, clip_text_embedding=clip, clip_image_embedding=tokens)
            p.step(0)
            first[which] = p.engine.io.out.float().clone()  # the UNet's output of the same first step in both forms
            assert p.engine.stats["fallback_nodes"] == [] and (p.engine.stats.get("attn_streams_sites", 0) > 0) == on, "the path asked for did not run"
        lowering_blocks.ATTN_STREAMS = True
        paths = (pipes["fused"], pipes["unfused"], bare)
        bare.step(0)
        for _ in range(3):
            for p in paths:
                p.step(3)
        assert all(p.graph is not None for p in paths)
        runs = [tuple(timeit(lambda p=p: p.step(3), a.iters) for p in paths) for _ in range(3)]
        x2, ts = torch.cat((x, x)), torch.tensor([500.0], device=dev)

        def forward():  # (a Chain forward resets the context store when it returns)
            ad.set_clip_image_embedding(tokens)
            unet.set_clip_text_embedding(clip)
            unet.set_timestep(ts)
            unet(x2)

        with torch.no_grad():
            forward()
            chain = [(timeit(forward, max(3, a.iters // 6)),) for _ in range(3)]
        diff = (first["fused"] - first["unfused"]).norm() / first["unfused"].norm()
        res[name] = {
            "image_tokens": nt,
            "fused_step_ms": round(med(runs, 0), 4), "fused_step_ms_min_max": span(runs, 0),
            "unfused_step_ms": round(med(runs, 1), 4), "unfused_step_ms_min_max": span(runs, 1),
            "bare_step_ms": round(med(runs, 2), 4), "bare_step_ms_min_max": span(runs, 2),
            "chain_forward_ms": round(med(chain, 0), 3), "chain_forward_ms_min_max": span(chain, 0),
            "unfused_over_fused": round(med(runs, 1) / med(runs, 0), 4), "fused_over_bare": round(med(runs, 0) / med(runs, 2), 4),
            "step_launches": {k: p.engine.stats["step_ops"] for k, p in pipes.items()} | {"bare": bare.engine.stats["step_ops"]},
            "fused_vs_unfused_unet_out_rel_l2": float(diff),
        }
        print(name, json.dumps(res[name]), flush=True)
        del pipes, unet, ad
        torch.cuda.empty_cache()
    res["kernels"] = kernel_points(dev, dt, a.iters)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
