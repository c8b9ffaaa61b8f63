"""InformativeDrawings (the lineart preprocessor) timing, bfloat16, synthetic weights (tests/lineart_cases.draw_weights), default 3 residual blocks:
    1 x 3 x 512 x 512 and 1 x 3 x 1024 x 1024
In ONE process: CompiledInformativeDrawings (one HIP-graph replay per call) against the unfused torch forward of the same mirror tree on the same
GPU, alternating the two, three repeats each, every shape warmed first; times are a host clock around work that ends in a device synchronise.
Then the native program launch by launch: every recorded launch replayed alone, back to back, between device events (its operands are then as
warm as the caches can hold them: a 33.5 MB tensor fits the Infinity Cache), with the bytes it has to move computed from its shapes, and the
achieved GB/s against the 6.3 TB/s copy rate.  Needs a GPU (no fallback).
    python tools/probe_lineart.py --json profiles/lineart_probe.json"""
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
from refiners_amd.engine.lineart import CompiledInformativeDrawings  # noqa: E402
from refiners_amd.latent_diffusion.preprocessors import InformativeDrawings  # noqa: E402
from tests.lineart_cases import draw_weights  # noqa: E402

POINTS = {"1x512": (1, 512), "1x1024": (1, 1024)}
COPY_GBS = 6300.0  # MI355X_MICROARCH.md: the measured device copy rate


def build(device, dtype):
    model = InformativeDrawings(device="meta")
    sd = draw_weights(synth.model_shapes(model))
    model.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in sd.items()}, assign=True)
    return model.eval()


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def launch_bytes(name, a, es):
    """(bytes a launch must read, bytes it must write, what it is), from the fields of its argument struct."""
    if name == "mi355x_lineart_stem":
        return a.B * a.Cin * a.H * a.W * es, a.B * a.H * a.W * 64 * es, f"stem {a.H}x{a.W}"
    if name == "mi355x_lineart_in_stats":
        return a.B * a.H * a.W * a.C * es, a.B * a.C * 8, f"stats {a.H}x{a.W}x{a.C} layout {a.layout}"
    if name == "mi355x_lineart_in_apply":
        n = a.B * a.H * a.W * a.C * es
        out = a.B * (a.H + 2 * a.ring) * (a.W + 2 * a.ring) * a.C * es
        return n * (2 if a.ldr else 1), out, f"apply {a.H}x{a.W}x{a.C} layout {a.layout} ring {a.ring}"
    if name == "mi355x_lineart_head":
        return a.B * a.H * a.W * 64 * es, a.B * a.H * a.W * es, f"head {a.H}x{a.W}"
    sg = a.seg[0]  # mi355x_gemm(conv): the input image once, the weights once, the output once
    return (a.B * sg.H * sg.W * sg.k + a.N * sg.ksize * sg.ksize * sg.k) * es, a.M * a.N * es, f"conv{sg.ksize}x{sg.ksize}/{sg.stride} {sg.H}x{sg.W}x{sg.k} -> {a.N}"


def per_launch(low, es, reps=20):
    rows = []
    stream = native.stream_ptr()
    for fn, args, name, _keep in low.step:
        if fn is None:
            continue
        for _ in range(3):
            native.check(fn(*args, stream), name)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn(*args, stream)
        end.record()
        end.synchronize()
        us = start.elapsed_time(end) / reps * 1e3
        rd, wr, what = launch_bytes(name, args[0]._obj, es)
        rows.append({"launch": name, "what": what, "us": round(us, 2), "read_bytes": int(rd), "write_bytes": int(wr), "gb_per_s": round((rd + wr) / us / 1e3, 1),
                     "share_of_copy_rate": round((rd + wr) / us / 1e3 / COPY_GBS, 3)})
    return rows


def measure(point, iters):
    batch, side = POINTS[point]
    dev, dt = torch.device("cuda"), torch.bfloat16
    model = build(dev, dt)
    fast = CompiledInformativeDrawings(model)
    x = torch.rand((batch, 3, side, side), generator=torch.Generator().manual_seed(1)).to(dev, dt)

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
    apart = float((a.float() - b.float()).abs().max())
    for _ in range(3):  # warm both paths: the second engine call captures the graph
        engine()
        unfused()
    runs = [(timeit(engine, iters), timeit(unfused, iters)) for _ in range(3)]
    e, u = sorted(r[0] for r in runs), sorted(r[1] for r in runs)
    low = next(iter(fast.entries.values())).low
    rows = per_launch(low, 2)
    return {"input": [batch, 3, side, side], "engine_ms": round(e[1], 3), "engine_ms_min_max": [round(e[0], 3), round(e[2], 3)],
            "unfused_torch_ms": round(u[1], 3), "unfused_torch_ms_min_max": [round(u[0], 3), round(u[2], 3)], "speedup": round(u[1] / e[1], 2),
            "launches": fast.stats["step_ops"], "launches_by_kernel": dict(Counter(op[2] for op in low.step if op[0] is not None)),
            "pool_bytes": fast.stats["pool_bytes"], "first_call_ms_with_lowering": round(first_ms, 1), "max_abs_engine_vs_unfused": round(apart, 5),
            "sum_of_launches_us": round(sum(r["us"] for r in rows), 1), "per_launch": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="*", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_lineart.py measures on the GPU; there is no CPU fallback"
    res = {"workload": "informative_drawings", "dtype": "bfloat16", "device": torch.cuda.get_device_name(0), "copy_rate_gb_per_s": COPY_GBS, "points": {}}
    for point in args.points:
        res["points"][point] = measure(point, args.iters)
        p = res["points"][point]
        print(json.dumps({point: {k: v for k, v in p.items() if k != "per_launch"}}), flush=True)
        for r in p["per_launch"]:
            print(f"  {r['us']:9.2f} us  {r['gb_per_s']:8.1f} GB/s  {r['launch']}  {r['what']}", flush=True)
        torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
