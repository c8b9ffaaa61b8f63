"""ELLA timing on SD1.5 at 512 x 512 (64 x 64 latents), classifier-free-guidance pair (B = 2), bfloat16, T = 128 LLM tokens, synthetic weights
(refiners_amd.synth; the encoder's drawn as the fixtures draw them, AdaLayerNorm Linears non-zero).  In ONE process:
    ella_step      the lowered step of SD1UNet + SD1ELLAAdapter: one HIP-graph replay (CompiledUNet.run_step), and the whole call (staging + replay + copy out)
    bare_step      the lowered step of the same UNet without the adapter (77 CLIP tokens, K / V^T in the prologue), the same two ways
    stock_chain    the stock Chain forward of the adapted tree in torch: what CompiledUNet fell back to before ELLA was lowered
the three alternating, three repeats each, every path warmed first; times are a host clock around work that ends in a device synchronise.
Also reports the launches ELLA adds to the step (by kernel) and how far the lowered and the stock outputs are apart.  Needs a GPU (no fallback).
    python tools/probe_ella.py --json profiles/ella_probe.json"""
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
from refiners_amd.engine.compiled import CompiledUNet  # noqa: E402
from refiners_amd.latent_diffusion import SD1ELLAAdapter  # noqa: E402
from refiners_amd.latent_diffusion.sd1 import SD1UNet  # noqa: E402
from tests.ella_cases import draw_weights  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_ella needs a GPU"
    dev, dt, B = torch.device("cuda"), torch.bfloat16, 2
    g = torch.Generator().manual_seed(1)
    shapes = synth.model_shapes(SD1UNet(4, device="meta"))
    sd = synth.synth_state_dict(shapes, 0)
    with_ella, bare = build(dev, dt, sd), build(dev, dt, sd)
    del sd
    adapter = SD1ELLAAdapter(with_ella)
    enc = adapter.latents_encoder
    enc.load_state_dict({k: v.to(device=dev, dtype=dt) for k, v in draw_weights(synth.model_shapes(enc), "probe").items()}, assign=True)
    adapter.inject()
    x = torch.randn((B, 4, a.latent, a.latent), generator=g).to(dev, dt)
    llm = torch.randn((B, a.tokens, 2048), generator=g).to(dev, dt)
    clip = torch.randn((B, 77, 768), generator=g).to(dev, dt)
    ts = torch.tensor([500.0], device=dev)
    fast_e, fast_b = CompiledUNet(with_ella), CompiledUNet(bare)

    def ella_call():
        adapter.set_llm_text_embedding(llm)
        with_ella.set_timestep(ts)
        return fast_e(x)

    def bare_call():
        bare.set_clip_text_embedding(clip)
        bare.set_timestep(ts)
        return fast_b(x)

    def stock():
        adapter.set_llm_text_embedding(llm)
        with_ella.set_timestep(ts)
        with torch.no_grad():
            return with_ella(x)

    ye = ella_call()
    bare_call()
    ys = stock()
    assert fast_e.stats["fallback_nodes"] == [] and fast_e.stats.get("ella_sites") == 16 and fast_b.stats["fallback_nodes"] == [], "the native path did not run"
    apart = float((ye.float() - ys.float()).norm() / ys.float().norm())
    for _ in range(3):  # warm every path: the second engine call captures the graph
        ella_call()
        bare_call()
        stock()
    runs = []
    for _ in range(3):
        runs.append((timeit(fast_e.run_step, a.iters), timeit(fast_b.run_step, a.iters), timeit(ella_call, a.iters), timeit(bare_call, a.iters), timeit(stock, max(a.iters // 5, 3))))
    med = lambda i: sorted(r[i] for r in runs)[1]  # noqa: E731
    span = lambda i: [round(min(r[i] for r in runs), 3), round(max(r[i] for r in runs), 3)]  # noqa: E731
    ke, kb = Counter(op[2] for op in fast_e.low.step if op[0] is not None), Counter(op[2] for op in fast_b.low.step if op[0] is not None)
    res = {
        "device": torch.cuda.get_device_name(0), "shape": {"batch": B, "latent": a.latent, "llm_tokens": a.tokens, "dtype": "bfloat16"}, "iters": a.iters,
        "ella_step_replay_ms": round(med(0), 3), "ella_step_replay_ms_min_max": span(0),
        "bare_step_replay_ms": round(med(1), 3), "bare_step_replay_ms_min_max": span(1),
        "ella_call_ms": round(med(2), 3), "ella_call_ms_min_max": span(2),
        "bare_call_ms": round(med(3), 3), "bare_call_ms_min_max": span(3),
        "stock_chain_ms": round(med(4), 3), "stock_chain_ms_min_max": span(4),
        "ella_cost_ms": round(med(0) - med(1), 3), "speedup_over_stock_chain": round(med(4) / med(2), 2),
        "step_launches": {"ella": fast_e.stats["step_ops"], "bare": fast_b.stats["step_ops"], "added": fast_e.stats["step_ops"] - fast_b.stats["step_ops"]},
        "added_by_kernel": {k: ke[k] - kb.get(k, 0) for k in sorted(ke) if ke[k] != kb.get(k, 0)},
        "prologue_launches": {"ella": fast_e.stats["prologue_ops"], "bare": fast_b.stats["prologue_ops"]},
        "lowered_vs_stock_relative_l2": round(apart, 5), "prologue_runs": fast_e.prologue_runs, "lowerings": fast_e.lowerings,
    }
    print(json.dumps(res, indent=1))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
