"""DINOv2 timing at three points, bfloat16, synthetic weights (refiners_amd.synth; LayerScale weights, position table, class token and
registers drawn as the fixtures draw them):
    DINOv2_large_reg   1 x 3 x 518 x 518   (1 374 tokens, the native grid)
    DINOv2_small      64 x 3 x 224 x 224   (the feature-extraction / FID shape)
    DINOv2_giant_reg   8 x 3 x 224 x 224
In ONE process per run: CompiledDINOv2 (one HIP-graph replay per call) against the unfused torch forward of the same mirror tree on the same
GPU, alternating the two, three repeats each, every shape warmed first; times are a host clock around work that ends in a device
synchronise.  Also reports how far the two paths' outputs are apart and which kernels the step launches.  Needs a GPU (no fallback).
    python tools/probe_dinov2.py --json profiles/dinov2_probe.json"""
import argparse
import json
import sys
import time
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import dinov2 as DV  # noqa: E402
from refiners_amd import synth  # noqa: E402
from refiners_amd.engine.dinov2 import CompiledDINOv2  # noqa: E402
from tests.dinov2_cases import draw_weights  # noqa: E402

POINTS = {
    "large_reg_1x518": ("DINOv2_large_reg", 1, 518),
    "small_64x224": ("DINOv2_small", 64, 224),
    "giant_reg_8x224": ("DINOv2_giant_reg", 8, 224),
}


def build(name, device, dtype):
    model = getattr(DV, name)(device="meta")
    sd = draw_weights(synth.model_shapes(model), "probe")
    model.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in sd.items()}, assign=True)
    return model


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def measure(point, iters):
    name, batch, side = POINTS[point]
    dev, dt = torch.device("cuda"), torch.bfloat16
    model = build(name, dev, dt)
    fast = CompiledDINOv2(model)
    x = torch.randn((batch, 3, side, side), generator=torch.Generator().manual_seed(1)).to(dev, dt)

    def engine():
        return fast(x)

    def unfused():
        with torch.no_grad():
            return model(x)

    t0 = time.perf_counter()
    a = engine()
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    assert fast.stats.get("fallback_nodes") == [] and fast.lowerings == 1, "the native path did not run"
    b = unfused()
    apart = float((a.float() - b.float()).norm() / b.float().norm())
    for _ in range(3):  # warm both paths: the second engine call captures the graph
        engine()
        unfused()
    runs = [(timeit(engine, iters), timeit(unfused, max(iters // 3, 3))) for _ in range(3)]
    e, u = sorted(r[0] for r in runs), sorted(r[1] for r in runs)
    low = next(iter(fast.entries.values())).low
    return {"model": name, "input": [batch, 3, side, side], "tokens": fast.stats["tokens"], "token_rows": fast.stats["token_rows"],
            "engine_ms": round(e[1], 3), "engine_ms_min_max": [round(e[0], 3), round(e[2], 3)],
            "unfused_torch_ms": round(u[1], 3), "unfused_torch_ms_min_max": [round(u[0], 3), round(u[2], 3)], "speedup": round(u[1] / e[1], 2),
            "launches": fast.stats["step_ops"], "launches_by_kernel": dict(Counter(op[2] for op in low.step if op[0] is not None)),
            "prologue_launches": fast.stats["prologue_ops"], "pool_bytes": fast.stats["pool_bytes"], "first_call_ms_with_lowering": round(first_ms, 1),
            "rel_l2_engine_vs_unfused": round(apart, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="*", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_dinov2.py measures on the GPU; there is no CPU fallback"
    res = {"workload": "dinov2_encoder", "dtype": "bfloat16", "device": torch.cuda.get_device_name(0), "points": {}}
    for point in args.points:
        res["points"][point] = measure(point, args.iters)
        print(json.dumps({point: res["points"][point]}), flush=True)
        torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
