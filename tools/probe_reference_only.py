"""Reference-only control timing on SD1.5 at 512 x 512 (64 x 64 latents), classifier-free-guidance pair (B = 2), bfloat16, 77 CLIP tokens, synthetic
weights (refiners_amd.synth).  In ONE process:
    adapted_step   the lowered step of SD1UNet + ReferenceOnlyControlAdapter (guide part + real pass): one HIP-graph replay (CompiledUNet.run_step),
                   and the whole call (staging of x and the guide + replay + copy out)
    bare_step      the lowered step of the same UNet without the adapter, the same two ways
    stock_chain    the stock Chain forward of the adapted tree in torch: what CompiledUNet fell back to before the adapter was lowered
the three alternating, three repeats each, every path warmed first; times are a host clock around work that ends in a device synchronise.
Then mi355x_attention_joint at SD1.5's four self-attention shapes (L = 4096 / 1024 / 256 / 64 keys per segment, 8 heads of 40 / 80 / 160 / 160)
against the three launches it replaces: mi355x_attention_general over a packed 2L-key buffer, mi355x_attention_general for row 0 over L keys,
mi355x_axpby for the blend -- the packing of the 2L buffer (two copies per site) is NOT counted against the three-launch form.  Each form is
replayed from a captured graph of `reps` launches, alternating, three repeats.  Needs a GPU (no fallback).
    python tools/probe_reference_only.py --json profiles/reference_only_probe.json"""
import argparse
import json
import sys
import time
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import native, synth  # noqa: E402
from refiners_amd.engine.compiled import CompiledUNet  # noqa: E402
from refiners_amd.latent_diffusion import ReferenceOnlyControlAdapter  # noqa: E402
from refiners_amd.latent_diffusion.sd1 import SD1UNet  # noqa: E402


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def build(dev, dt, sd):
    unet = SD1UNet(4, device="meta")
    unet.load_state_dict({k: v.to(device=dev, dtype=dt) for k, v in sd.items()}, assign=True)
    return unet


def graphed(fn, reps):
    """`reps` launches of fn as one captured graph: (replay, reps)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    return g.replay


def kernel_shapes(dev, dt, reps, iters):
    out = []
    gen = torch.Generator().manual_seed(3)
    H, B = 8, 2
    for L, D in ((4096, 40), (1024, 80), (256, 160), (64, 160)):
        C = H * D
        r = lambda *s: torch.randn(s, generator=gen).to(dev, dt)  # noqa: E731
        q, k0, k1 = r(B, L, C), r(B, L, C), r(B, L, C)
        vt0, vt1 = r(C, B, L), r(C, B, L)
        kk, vv = torch.cat([k0, k1], 1).contiguous(), torch.cat([vt0, vt1], 2).contiguous()
        mix = torch.tensor([0.5, 1.0], device=dev)
        o, o2, o0 = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q[:1])

        def joint():
            native.attention_joint(q, k0, vt0, L, k1, vt1, L, o, H, mix=mix)

        def three():
            native.attention_general(q, kk, vv, o2, H, 2 * L)
            native.attention_general(q[:1], k0[:1], vt0[:, :1], o0, H, L)
            native.axpby(o2[0], 0.5, o0[0], 0.5, o2[0])

        joint(), three()
        torch.cuda.synchronize()
        apart = float((o.float() - o2.float()).abs().max() / o2.float().abs().max())
        gj, g3 = graphed(joint, reps), graphed(three, reps)
        runs = [(timeit(gj, iters) / reps * 1e3, timeit(g3, iters) / reps * 1e3) for _ in range(3)]
        med = lambda i: sorted(x[i] for x in runs)[1]  # noqa: E731
        span = lambda i: [round(min(x[i] for x in runs), 2), round(max(x[i] for x in runs), 2)]  # noqa: E731
        out.append({"L": L, "D": D, "joint_us": round(med(0), 2), "joint_us_min_max": span(0), "three_launch_us": round(med(1), 2), "three_launch_us_min_max": span(1),
                    "joint_vs_three_launch_max_abs_rel": round(apart, 5)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_reference_only needs a GPU"
    dev, dt, B = torch.device("cuda"), torch.bfloat16, 2
    g = torch.Generator().manual_seed(1)
    sd = synth.synth_state_dict(synth.model_shapes(SD1UNet(4, device="meta")), 0)
    adapted, bare = build(dev, dt, sd), build(dev, dt, sd)
    del sd
    adapter = ReferenceOnlyControlAdapter(adapted).inject()
    x = torch.randn((B, 4, a.latent, a.latent), generator=g).to(dev, dt)
    guide = torch.randn((B, 4, a.latent, a.latent), generator=g).to(dev, dt)
    clip = torch.randn((B, 77, 768), generator=g).to(dev, dt)
    ts = torch.tensor([500.0], device=dev)
    fast_a, fast_b = CompiledUNet(adapted), CompiledUNet(bare)

    def adapted_call():
        adapter.set_controlnet_condition(guide)
        adapted.set_clip_text_embedding(clip)
        adapted.set_timestep(ts)
        return fast_a(x)

    def bare_call():
        bare.set_clip_text_embedding(clip)
        bare.set_timestep(ts)
        return fast_b(x)

    def stock():
        adapter.set_controlnet_condition(guide)
        adapted.set_clip_text_embedding(clip)
        adapted.set_timestep(ts)
        with torch.no_grad():
            return adapted(x.clone())

    ya = adapted_call()
    bare_call()
    ys = stock()
    assert fast_a.stats["fallback_nodes"] == [] and fast_a.stats.get("reference_only_sites") == 16 and fast_b.stats["fallback_nodes"] == [], "the native path did not run"
    apart = float((ya.float() - ys.float()).norm() / ys.float().norm())
    for _ in range(3):  # warm every path: the second engine call captures the graph
        adapted_call()
        bare_call()
        stock()
    runs = []
    for _ in range(3):
        runs.append((timeit(fast_a.run_step, a.iters), timeit(fast_b.run_step, a.iters), timeit(adapted_call, a.iters), timeit(bare_call, a.iters), timeit(stock, max(a.iters // 5, 3))))
    med = lambda i: sorted(r[i] for r in runs)[1]  # noqa: E731
    span = lambda i: [round(min(r[i] for r in runs), 3), round(max(r[i] for r in runs), 3)]  # noqa: E731
    ka, kb = Counter(op[2] for op in fast_a.low.step if op[0] is not None), Counter(op[2] for op in fast_b.low.step if op[0] is not None)
    res = {
        "device": torch.cuda.get_device_name(0), "shape": {"batch": B, "latent": a.latent, "clip_tokens": 77, "dtype": "bfloat16"}, "iters": a.iters,
        "adapted_step_replay_ms": round(med(0), 3), "adapted_step_replay_ms_min_max": span(0),
        "bare_step_replay_ms": round(med(1), 3), "bare_step_replay_ms_min_max": span(1),
        "adapted_call_ms": round(med(2), 3), "adapted_call_ms_min_max": span(2),
        "bare_call_ms": round(med(3), 3), "bare_call_ms_min_max": span(3),
        "stock_chain_ms": round(med(4), 3), "stock_chain_ms_min_max": span(4),
        "adapted_over_bare": round(med(0) / med(1), 3), "speedup_over_stock_chain": round(med(4) / med(2), 2),
        "step_launches": {"adapted": fast_a.stats["step_ops"], "guide_part": fast_a.stats["reference_only_guide_ops"], "bare": fast_b.stats["step_ops"]},
        "adapted_by_kernel": dict(sorted(ka.items())), "bare_by_kernel": dict(sorted(kb.items())),
        "prologue_launches": {"adapted": fast_a.stats["prologue_ops"], "bare": fast_b.stats["prologue_ops"]},
        "lowered_vs_stock_relative_l2": round(apart, 5), "prologue_runs": fast_a.prologue_runs, "lowerings": fast_a.lowerings,
        "joint_kernel": kernel_shapes(dev, dt, reps=20, iters=max(a.iters // 3, 5)),
    }
    print(json.dumps(res, indent=1))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
