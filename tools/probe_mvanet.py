"""MVANet timing as `solutions.BoxSegmenter` builds it: MVANet() with its default depths [2, 2, 18, 2] in eval mode, one 1 x 3 x 1024 x 1024
image, bfloat16, the synthetic weights of tests/mvanet_cases.py.  In ONE process: CompiledMVANet (one HIP-graph replay per call) against the
unfused torch forward of the same mirror tree on the same GPU, alternating the two, three repeats each, both warmed first; times are a host
clock around work that ends in a device synchronise.  Also reports how far the two paths' logits are apart, and a breakdown of the native
program by kernel family: every launch of the recorded program replayed on its own between two device events (so the sum exceeds the graph
replay by the launch gaps; it ranks the families, it is not a trace).  Needs a GPU (no fallback).
    python tools/probe_mvanet.py --json profiles/mvanet_probe.json"""
import argparse
import json
import sys
import time
from collections import defaultdict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import native  # noqa: E402
from refiners_amd.engine.mvanet import CompiledMVANet  # noqa: E402
from refiners_amd.mvanet import MVANet  # noqa: E402
from tests.mvanet_cases import draw_weights  # noqa: E402


def build(device, dtype, depths):
    model = MVANet(depths=depths, device="meta")
    sd = draw_weights({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: v.to(device=device, dtype=dtype if v.is_floating_point() else None) for k, v in sd.items()}, assign=True)
    return model.eval()


def timeit(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def families(ops, repeats=3):
    """ms per kernel family: backbone = every launch between the view split and the shallow convolution's input transpose."""
    names = [e[2] for e in ops]
    lo, hi = names.index("mi355x_mvanet_split_views") + 1, names.index("mi355x_nchw_to_nhwc")

    def family(i, name):
        if lo <= i < hi:
            return "backbone"
        if name == "mi355x_attention_general":
            return "attention"
        if name == "mi355x_gemm(conv)":
            return "convolutions"
        if name in ("mi355x_gemm", "mi355x_layernorm"):
            return "decoder_gemm_layernorm"
        return "streaming"

    total, count = defaultdict(float), defaultdict(int)
    for r in range(repeats + 1):
        for i, op in enumerate(ops):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            native.replay([op])
            b.record()
            b.synchronize()
            if r:  # (the first pass warms)
                total[family(i, op[2])] += a.elapsed_time(b) / repeats
                count[family(i, op[2])] += 1
    return {k: {"ms": round(v, 3), "launches": count[k] // repeats} for k, v in sorted(total.items(), key=lambda kv: -kv[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", type=int, nargs=4, default=[2, 2, 18, 2])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "probe_mvanet.py measures on the GPU; there is no CPU fallback"
    dev, dt = torch.device("cuda"), torch.bfloat16
    model = build(dev, dt, args.depths)
    fast = CompiledMVANet(model)
    x = torch.randn((1, 3, 1024, 1024), generator=torch.Generator().manual_seed(1)).to(dev, dt)

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
    apart = float((a.float() - b.float()).norm() / b.float().norm())
    for _ in range(3):  # warm both paths: the second engine call captures the graph
        engine()
        unfused()
    runs = [(timeit(engine, args.iters), timeit(unfused, max(args.iters // 2, 3))) for _ in range(3)]
    e, u = sorted(r[0] for r in runs), sorted(r[1] for r in runs)
    res = {"workload": "mvanet_box_segmenter", "depths": args.depths, "input": [1, 3, 1024, 1024], "dtype": "bfloat16",
           "engine_ms": round(e[1], 3), "engine_ms_min_max": [round(e[0], 3), round(e[2], 3)],
           "unfused_torch_ms": round(u[1], 3), "unfused_torch_ms_min_max": [round(u[0], 3), round(u[2], 3)], "speedup": round(u[1] / e[1], 2),
           "launches": fast.stats["step_ops"], "pool_bytes": fast.stats["pool_bytes"], "first_call_ms_with_lowering": round(first_ms, 1),
           "rel_l2_engine_vs_unfused_logits": round(apart, 5), "families_ms_launch_by_launch": families(fast.low.step), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
