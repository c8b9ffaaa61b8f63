"""What the Self-Attention Guidance tap costs, fused (mi355x_attention_key_mass: two launches, no score matrix in memory) against the chain it
replaces (per sample and head: mi355x_gemm into an L x L float32 scratch, mi355x_softmax_rows, mi355x_colsum_rows).  In ONE process, the two forms
alternating, every form warmed first, device events around captured graphs of REPS calls:
    tap alone   SDXL's middle block (L = 1024, 20 heads of 64, n = 1 and 4) in bfloat16 and float32, with pass B's key tile forced to 16 / 32 / 64
                keys and as the library picks it; SD1.5's middle block (L = 64, 8 heads of 160, n = 1): the chain takes that width in float32 only
    whole step  SDXL at 1024 x 1024 (128 x 128 latents), CFG pair + the guidance's second UNet pass, bfloat16, DDIM(30), synthetic weights:
                CompiledSDXL.step lowered with the lever on and off (REFINERS_AMD_SAG_MASS's two forms)
Every figure is the median of three repeats, with their minimum and maximum beside it.  Needs a GPU (no fallback).
    python tools/probe_sag_mass.py --json profiles/sag_mass_probe.json"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import native, synth  # noqa: E402
from refiners_amd.engine import lowering_blocks  # noqa: E402
from refiners_amd.engine.compiled import CompiledSDXL  # noqa: E402
from refiners_amd.latent_diffusion.sag import SDXLSAGAdapter  # noqa: E402
from refiners_amd.latent_diffusion.sdxl import SDXLUNet  # noqa: E402

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


def graph_of(emit, reps):
    ops = []
    with native.recording(ops):
        for _ in range(reps):
            emit()
    native.replay(ops)  # warm: code objects, attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        native.replay(ops)
    return g.replay


def tap_points(dev, iters):
    out = []
    lib = native.load()
    for L, H, D, n in ((1024, 20, 64, 1), (1024, 20, 64, 4), (64, 8, 160, 1)):
        for dt in (torch.bfloat16, torch.float32):
            C_ = H * D
            qk = torch.randn(n * L, 2 * C_, generator=torch.Generator().manual_seed(L + n)).to(dev, dt)
            q, k = qk[:, :C_], qk[:, C_:]
            lse, mass = torch.empty(n, H, L, device=dev), torch.empty(n, L, device=dev)
            sc, pr, cmass = torch.empty(L, L, device=dev), torch.empty(L, L, device=dev, dtype=dt), torch.empty(n, L, device=dev)

            def fused():
                native.attention_key_mass(q.view(n, L, C_), k.view(n, L, C_), H, D ** -0.5, lse, mass)

            def chain():
                for b in range(n):
                    for h in range(H):
                        native.gemm([(q[b * L : (b + 1) * L, h * D : (h + 1) * D], k[b * L : (b + 1) * L, h * D : (h + 1) * D])], sc, out_f32=dt != torch.float32)
                        native.softmax_rows(sc, pr, L, D ** -0.5)
                        native.colsum_rows(pr, cmass[b], accumulate=h > 0, scale=1.0 / H)

            forms = {}
            for tile in (0, 16, 32, 64):  # (the height is read when the call is made, i.e. when the graph is captured)
                lib.mi355x_key_mass_set_tile(tile)
                forms[f"fused_tile_{tile or 'auto'}"] = (graph_of(fused, 20), 20)
            lib.mi355x_key_mass_set_tile(0)
            has_chain = D % (128 // q.element_size()) == 0
            if has_chain:
                forms["chain"] = (graph_of(chain, 2), 2)
            runs = {name: [] for name in forms}
            for _ in range(3):
                for name, (g, per) in forms.items():
                    runs[name].append(events_us(g, iters, per))
            row = {"L": L, "H": H, "D": D, "n": n, "dtype": str(dt).split(".")[1], "launches": {"fused": 2, "chain": 3 * n * H if has_chain else None},
                   "us_per_call": {name: stat(v) for name, v in runs.items()}}
            if has_chain:
                g, _ = forms["chain"]
                g()
                forms["fused_tile_auto"][0]()
                torch.cuda.synchronize()
                row["fused_vs_chain_max_rel"] = float((mass - cmass).abs().max() / cmass.abs().max())
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def step_point(dev, iters, latent):
    dt, steps = torch.bfloat16, 30
    unet = SDXLUNet(4, device="meta")
    unet.load_state_dict({k: v.to(device=dev, dtype=dt) for k, v in synth.synth_state_dict(synth.model_shapes(unet), 0).items()}, assign=True)
    SDXLSAGAdapter(target=unet, scale=0.75).inject()
    inp = {k: v.to(dev) for k, v in synth.sdxl_inputs(1, (latent, latent), 3).items()}
    pipes = {}
    for which, on in (("fused", True), ("chain", False)):
        lowering_blocks.SAG_MASS = on  # the switch the environment variable sets at import; a program keeps the form it was lowered with
        p = pipes[which] = CompiledSDXL(unet, num_inference_steps=steps, condition_scale=5.0)
        p.set_inputs(inp["x"].to(dt), clip_text_embedding=inp["text"].to(dt), pooled_text_embedding=inp["pooled"].to(dt), time_ids=inp["time_ids"])
        for _ in range(3):
            p.step(3)
        assert p.engine.stats["fallback_nodes"] == [] and p.engine.stats.get("sag_mass_fused", False) is on, "the path asked for did not run"
    lowering_blocks.SAG_MASS = True
    runs = {which: [] for which in pipes}
    for _ in range(3):
        for which, p in pipes.items():
            runs[which].append(events_us(lambda p=p: p.step(3), iters, 1) / 1e3)
    row = {"latent": latent, "dtype": "bfloat16", "solver": f"DDIM({steps})", "step_ms": {w: stat(v) for w, v in runs.items()},
           "step_launches": {w: p.engine.stats["step_ops"] for w, p in pipes.items()}}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_sag_mass needs a GPU"
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "taps": tap_points(dev, a.iters)}
    if not a.no_step:
        res["sdxl_step"] = step_point(dev, max(3, a.iters // 2), a.latent)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
