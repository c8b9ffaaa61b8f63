"""What the T2I-Adapter's condition encoder costs on the MI355X.  bfloat16, synthetic weights, ONE process, the variants alternating, every
variant warmed first, device events around the timed calls.  Two geometries: SDXL (ConditionEncoderXL, a 1024 x 1024 picture, r = 16) and SD1.5
(ConditionEncoder, 512 x 512, r = 8), both with the default widths (320, 640, 1280, 1280):
    encoder   CompiledT2IConditionEncoder (graph replay, its input copy and output clones included) against the stock torch forward of the same tree
    stem      mi355x_t2i_stem alone, as captured graphs of REPS calls, at every (strip, chunk) of the lever and as the library picks them
    unfused   for the record: torch's pixel_unshuffle, mi355x_nchw_to_nhwc and the existing implicit-GEMM 3 x 3 convolution on the unshuffled tensor
Every figure is the median of three repeats, with their minimum and maximum beside it.  Needs a GPU (no fallback).
    python tools/probe_t2i.py --json profiles/t2i_probe.json"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from refiners_amd import native, synth  # noqa: E402
from refiners_amd.engine import CompiledT2IConditionEncoder  # noqa: E402
from refiners_amd.latent_diffusion import t2i as M  # noqa: E402

REPS = 10
GEOMETRIES = {"sdxl_1024": ("ConditionEncoderXL", 16, 1024), "sd1_512": ("ConditionEncoder", 8, 512)}
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


def alternate(forms, iters, per):
    runs = {name: [] for name in forms}
    for _ in range(3):
        for name, fn in forms.items():
            runs[name].append(events_us(fn, iters, per))
    return {name: stat(v) for name, v in runs.items()}


def stem_point(dev, iters, r, side, C0=320):
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, side, side, generator=g).to(dev, dt)
    w = (torch.randn(C0, 3 * r * r, 3, 3, generator=g) / (3 * r * 3 ** 0.5)).to(dt)
    h = side // r
    out = torch.empty(h * h, C0, device=dev, dtype=dt)
    wp = native.t2i_pack_stem(w, r, dt).to(dev)
    lib, forms = native.load(), {}
    for strip, chunk in ((0, 0), (32, 64), (32, 128), (64, 64), (64, 128)):  # (the lever is read when the call is made, i.e. when the graph is captured)
        lib.mi355x_t2i_set_strip(strip, chunk)
        ops = []
        with native.recording(ops):
            for _ in range(REPS):
                native.t2i_stem(x, wp, None, out, r)
        native.replay(ops)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            native.replay(ops)
        forms[f"strip_{strip}_chunk_{chunk}" if strip else "auto"] = graph.replay
    lib.mi355x_t2i_set_strip(0, 0)
    # the route the stem replaces: unshuffle (torch), to channels-last rows, the existing 3 x 3 implicit-GEMM convolution
    rows, w9 = torch.empty(h * h, 3 * r * r, device=dev, dtype=dt), native.pack_conv_weight(w.to(dev))
    out2 = torch.empty_like(out)

    def unfused():
        native.nchw_to_nhwc(F.pixel_unshuffle(x, r), rows.view(1, h * h, -1))
        native.conv_gemm([(rows.view(1, h, h, -1), w9, 3, 1, 1, 0)], out2, 1, h, h)

    unfused()
    graph.replay()
    torch.cuda.synchronize()
    diff = float((out.float() - out2.float()).abs().max() / out2.float().abs().max())
    res = alternate(forms, iters, REPS)
    res["unfused_route"] = alternate({"u": unfused}, iters, 1)["u"]
    row = {"r": r, "picture": [1, 3, side, side], "C0": C0, "dtype": "bfloat16", "flop": 2 * h * h * C0 * 27 * r * r, "us_per_launch": res, "stem_vs_unfused_max_rel": diff}
    print(json.dumps(row), flush=True)
    return row


def encoder_point(dev, iters, cls, side):
    dt = torch.bfloat16
    enc = getattr(M, cls)(device="meta")
    enc.load_state_dict({k: v.to(dev, dt) for k, v in synth.synth_state_dict({k: tuple(v.shape) for k, v in enc.state_dict().items()}, 0).items()}, assign=True)
    x = torch.rand(1, 3, side, side, generator=torch.Generator().manual_seed(2)).to(dev, dt)
    fast = CompiledT2IConditionEncoder(enc)
    with torch.no_grad():
        for _ in range(3):
            got, want = fast(x), enc(x)
    assert not fast.stats["whole_fallback"], "the path asked for did not run"
    err = max(float((a.float() - b.float()).norm() / b.float().norm()) for a, b in zip(got, want))

    def stock():
        with torch.no_grad():
            enc(x)

    row = {"encoder": cls, "picture": [1, 3, side, side], "dtype": "bfloat16", "launches": fast.stats["step_ops"],
           "ms_per_call": {k: {kk: (round(vv / 1e3, 4) if kk == "median" else [round(t / 1e3, 4) for t in vv]) for kk, vv in v.items()}
                           for k, v in alternate({"compiled": lambda: fast(x), "stock_torch": stock}, iters, 1).items()},
           "compiled_vs_stock_rel_l2": err}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_t2i needs a GPU"
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "stem": [stem_point(dev, a.iters, r, side) for _cls, r, side in GEOMETRIES.values()],
           "encoder": [encoder_point(dev, a.iters, cls, side) for cls, _r, side in GEOMETRIES.values()]}
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
