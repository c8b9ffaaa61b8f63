"""StyleAligned shared self-attention at the two full-size SDXL shapes with 4 images (CFG batch B = 8: L = 1024 tokens x C = 1280, 20 heads; L = 4096 x
C = 640, 10 heads), bf16:
  * mi355x_adain_stats (over the packed Q|K buffer) and mi355x_style_aligned_pack, in GB/s against the bytes the algorithm needs,
  * the 2L-key attention launch beside today's L-key launch,
  * the configs[1] step at 4 images per GPU (bench.py's bare workload) with and without the adapter, alternated in ONE process.
Kernel times: N launches over rotating buffer sets inside a HIP graph, best of 3 windows.  `python tools/probe_style_aligned.py [--no-step] [--json FILE]`"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import native  # noqa: E402

dev, dt = "cuda", torch.bfloat16
N_REP, N_SETS = 8, 4  # (4 sets x ~0.3-0.7 GB per shape: larger than the 256 MB Infinity Cache, so every launch streams from HBM)


def graph_time_us(fn, iters=5):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            g.replay()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) / iters / N_REP * 1e3)
    return best


def kernels(B, L, C, heads):
    n, es = B // 2, 2
    sets = []
    for _ in range(N_SETS):
        qk = torch.randn(B * L, 2 * C, device=dev).to(dt)
        vt = torch.randn(C, B * L, device=dev).to(dt)
        sets.append((qk, vt, torch.empty(B * 2 * L, C, device=dev, dtype=dt), torch.empty(C, B * 2 * L, device=dev, dtype=dt), torch.empty(B * L, C, device=dev, dtype=dt)))
    st = torch.empty(B, 2 * C, 2, device=dev, dtype=torch.float32)
    ws = torch.empty(max(native.adain_stats_ws_floats(B, L, 2 * C), 1), device=dev, dtype=torch.float32)
    scale = torch.full((1,), 0.5, device=dev)
    v3 = lambda t, rows: t.as_strided((B, rows, C), (rows * t.stride(0), t.stride(0), 1))  # noqa: E731

    def stats():
        for i in range(N_REP):
            native.adain_stats(sets[i % N_SETS][0].view(B, L, 2 * C), st, ws)

    def pack():
        for i in range(N_REP):
            qk, vt, ksh, vtsh, _ = sets[i % N_SETS]
            native.style_aligned_pack(v3(qk[:, :C], L), v3(qk[:, C:], L), vt.view(C, B, L), st[:, :C], st[:, C:], n, scale, 1e-8, ksh.view(B, 2 * L, C), vtsh.view(C, B, 2 * L))

    def attn(shared):
        def fn():
            for i in range(N_REP):
                qk, vt, ksh, vtsh, out = sets[i % N_SETS]
                kv = (ksh.view(B, 2 * L, C), vtsh.view(C, B, 2 * L), 2 * L, 1.0) if shared else (v3(qk[:, C:], L), vt.view(C, B, L), L, 1.0)
                native.attention(v3(qk[:, :C], L), out.view(B, L, C), heads, [kv])
        return fn

    stats()  # (the pack launches read a valid table)
    unit = B * L * C * es
    r = {"B": B, "L": L, "C": C, "heads": heads,
         "stats_us": graph_time_us(stats), "stats_bytes": 2 * unit,            # reads Q and K once
         "pack_us": graph_time_us(pack), "pack_bytes": 8 * unit,               # reads Q, K, V^T; writes Q', 2 x K rows, 2 x V^T columns
         "attention_L_us": graph_time_us(attn(False)), "attention_2L_us": graph_time_us(attn(True))}
    for k in ("stats", "pack"):
        r[f"{k}_GBps"] = round(r[f"{k}_bytes"] / r[f"{k}_us"] / 1e3, 1)
    r["attention_ratio"] = round(r["attention_2L_us"] / r["attention_L_us"], 3)
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def step(images=4, steps=20, rounds=2):
    import bench
    from refiners_amd.latent_diffusion.style_aligned import StyleAlignedAdapter

    unet, specs, _sd, pipe, _ = bench.build_pipeline("bare", images, 0, torch.device(dev), dt, "fused", use_graph=True, broadcast=False)
    adapter = StyleAlignedAdapter(unet, scale=0.5)
    res = {"without": [], "with": []}
    for _ in range(rounds):  # alternated: box drift shows as a difference between the rounds, not between the variants
        for name in ("without", "with"):
            if name == "with":
                adapter.inject()
            res[name].append(round(bench.timed_steps(pipe, steps, 3, 1, torch.device(dev)) / steps * 1e3, 3))
            if name == "with":
                assert pipe.engine.stats["style_aligned_sites"] == 70 and pipe.engine.stats["fallback_nodes"] == []
                adapter.eject()
    out = {"workload": f"configs[1] (bare), {images} images per GPU, bf16", "ms_per_step": res}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    native.load()
    out = {"kernels": [kernels(8, 1024, 1280, 20), kernels(8, 4096, 640, 10)]}
    if not args.no_step:
        out["step"] = step()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
