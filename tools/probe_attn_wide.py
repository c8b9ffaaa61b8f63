"""The autoencoder's single 512-wide attention head (bf16): ONE mi355x_attention_general launch (csrc/attn_wide_kernel.cuh) against the sequence it
replaced -- V transpose, then per sample float32 scores GEMM, row softmax, P V GEMM -- alternating in one process, several rounds each, so that the
spread between rounds of the same code stands next to the difference.  Prints one JSON line per shape."""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import native  # noqa: E402

C = 512
#: name, samples, tokens, launches per timed window
SHAPES = (("decode_1024x1024", 1, 16384, 20), ("tile_batch_4_of_512x512", 4, 4096, 40), ("edge_tiles_4_of_8x7", 4, 56, 200))


def time_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def replaced_sequence(q, k, v, out, B, L):
    """What BlockLowering.sdpa / TiledVAELowering.sdpa launched for this head before the fused kernel: the key axis padded to the GEMM's K block of 64."""
    lp = (L + 63) // 64 * 64
    vt = torch.zeros(B, C, lp, device="cuda", dtype=q.dtype)
    sc = torch.zeros(L, lp, device="cuda", dtype=torch.float32)
    pr = torch.empty(L, lp, device="cuda", dtype=q.dtype)

    def run():
        if lp == L:
            native.nhwc_to_nchw(v.view(B, L, C), vt.view(B, C, L, 1), C)
        else:  # (the tiled override gathered V into the zero-padded V^T in one launch; a strided copy stands in for it here)
            vt[:, :, :L].copy_(v.view(B, L, C).transpose(1, 2))
        for b in range(B):
            native.gemm([(q[b], k[b])], sc[:, :L], out_f32=True)
            native.softmax_rows(sc, pr, L, C ** -0.5)
            native.gemm([(pr, vt[b])], out[b])

    return run


def main():
    native.load()
    dt = torch.bfloat16
    for name, B, L, n in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(L)
        q, k, v = ((torch.randn(B, L, C, generator=g) * s).to("cuda", dt) for s in (1.0, 1.0, 1.0))
        lp = (L + 63) // 64 * 64
        vt = torch.zeros(C, B, lp, device="cuda", dtype=dt)
        vt[:, :, :L] = v.permute(2, 0, 1)
        out_new, out_old = torch.empty(B, L, C, device="cuda", dtype=dt), torch.empty(B, L, C, device="cuda", dtype=dt)
        fused = lambda: native.attention_general(q, k, vt, out_new, 1, L)  # noqa: E731
        old = replaced_sequence(q, k, v, out_old, B, L)
        for _ in range(2):  # warm-up: both paths, this shape
            fused()
            old()
        torch.cuda.synchronize()
        t_new, t_old = [], []
        for _ in range(7):  # alternating rounds
            t_new.append(time_ms(fused, n))
            t_old.append(time_ms(old, n))
        flop = 4.0 * B * L * L * C
        med_new, med_old = statistics.median(t_new), statistics.median(t_old)
        print(json.dumps({
            "shape": name, "samples": B, "tokens": L,
            "fused_ms": round(med_new, 4), "fused_min_max_ms": [round(min(t_new), 4), round(max(t_new), 4)], "fused_tflops": round(flop / med_new / 1e9, 1),
            "replaced_ms": round(med_old, 4), "replaced_min_max_ms": [round(min(t_old), 4), round(max(t_old), 4)],
            "max_abs_fused_vs_replaced": round((out_new.float() - out_old.float()).abs().max().item(), 5), "out_max_abs": round(out_old.float().abs().max().item(), 4),
        }), flush=True)


if __name__ == "__main__":
    main()
