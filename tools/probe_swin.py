"""Swin-B timing as MVANet builds it: embedding_dim 128, depths [2, 2, 18, 2], heads [4, 8, 16, 32], window 12, on MVANet's five views of
3 x 512 x 512, bfloat16, synthetic weights (refiners_amd.synth; canonical relative_position_index).  In ONE process: CompiledSwinTransformer
(one HIP-graph replay per call) against the unfused torch forward of the same mirror tree on the same GPU, alternating the two, three
repeats each, every shape warmed first; times are a host clock around work that ends in a device synchronise.  Also reports how far the
two paths' outputs are apart.  Needs a GPU (no fallback).
    python tools/probe_swin.py --json profiles/swin_probe.json"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import synth  # noqa: E402
from refiners_amd.engine.swin import CompiledSwinTransformer  # noqa: E402
from refiners_amd.swin import SwinTransformer, canonical_relative_position_index  # noqa: E402

SWIN_B = dict(embedding_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=12)


def build(device, dtype, seed=0):
    model = SwinTransformer(**SWIN_B, device="meta")
    shapes = synth.model_shapes(model)
    sd = synth.synth_state_dict(shapes, seed)
    for k, s in shapes.items():
        if k.endswith("relative_position_index"):
            sd[k] = canonical_relative_position_index(SWIN_B["window_size"])
        elif k.endswith("relative_position_bias_table"):
            sd[k] = synth.synth_tensor(k, s, seed, gain=0.5 * s[1] ** 0.5)
    model.load_state_dict({k: v.to(device=device, dtype=dtype if v.is_floating_point() else None) for k, v in sd.items()}, assign=True)
    return model


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_swin.py measures on the GPU; there is no CPU fallback"
    dev, dt = torch.device("cuda"), torch.bfloat16
    model = build(dev, dt)
    fast = CompiledSwinTransformer(model)
    x = torch.randn((args.views, 3, args.side, args.side), generator=torch.Generator().manual_seed(1)).to(dev, dt)

    def engine():
        return fast(x)

    def unfused():
        with torch.no_grad():
            return model(x)

    t0 = time.perf_counter()
    a = engine()
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    assert fast.stats.get("fallback_nodes") == [] and fast.key is not None, "the native path did not run"
    b = unfused()
    apart = [float((p.float() - q.float()).norm() / q.float().norm()) for p, q in zip(a, b)]
    for _ in range(3):  # warm both paths: the second engine call captures the graph
        engine()
        unfused()
    runs = [(timeit(engine, args.iters), timeit(unfused, max(args.iters // 3, 3))) for _ in range(3)]
    e, u = sorted(r[0] for r in runs), sorted(r[1] for r in runs)
    res = {"workload": "swin_b_mvanet_backbone", "config": SWIN_B, "input": [args.views, 3, args.side, args.side], "dtype": "bfloat16",
           "engine_ms": round(e[1], 3), "engine_ms_min_max": [round(e[0], 3), round(e[2], 3)],
           "unfused_torch_ms": round(u[1], 3), "unfused_torch_ms_min_max": [round(u[0], 3), round(u[2], 3)], "speedup": round(u[1] / e[1], 2),
           "launches": fast.stats["step_ops"], "pool_bytes": fast.stats["pool_bytes"], "first_call_ms_with_lowering": round(first_ms, 1),
           "rel_l2_engine_vs_unfused_per_output": [round(v, 5) for v in apart], "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
