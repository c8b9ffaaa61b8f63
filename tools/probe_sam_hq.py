"""HQ-SAM mask prediction timing: one 1024 x 1024 image embedding + early ViT embedding, P = 1 / 16 / 64 prompt sets of one foreground point,
float32 and bfloat16: CompiledHQSegmentAnything.predict_batch (point encoder in torch, one graph replay, hq + base, the postprocess_masks
kernel) against the unfused torch forward of the same adapted tree on the same GPU (the embedding repeated P times), alternating the two,
with the spread of three repeats.  Prints one JSON line per (dtype, P): milliseconds per batch, host clock around a device synchronise.
    python tools/probe_sam_hq.py > profiles/sam_hq_probe.log"""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd.engine.sam_hq import CompiledHQSegmentAnything  # noqa: E402
from refiners_amd.segment_anything import PointType, postprocess_masks  # noqa: E402
from tests.sam_hq_cases import early_embedding, embedding, hq_sam  # noqa: E402


def timeit(fn, n):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def main():
    dev, size = torch.device("cuda"), (1024, 1024)
    for dt in (torch.float32, torch.bfloat16):
        sam, adapter = hq_sam(dev, dt)
        adapter.set_context("hq_sam", {"early_vit_embedding": early_embedding().to(dev, dt)})
        fast = CompiledHQSegmentAnything(sam)
        emb = embedding().to(dev, dt)
        dec = sam.mask_decoder
        for P in (1, 16, 64):
            g = torch.Generator().manual_seed(P)
            pts = torch.rand(P, 1, 2, generator=g) * 1024
            types = torch.full((P, 1), PointType.FOREGROUND.value)

            def engine():
                return fast.predict_batch(emb, pts, types, original_size=size)

            def unfused():
                with torch.no_grad():
                    # (the tree's own PointTypeEmbedding cannot run in bfloat16: the point rows come from the engine's float32 copy of it)
                    point_embedding = torch.stack([fast._sparse(pts[p], types[p], size)[6:] for p in range(P)])
                    dec.set_image_embedding(image_embedding=emb.expand(P, -1, -1, -1).contiguous())
                    dec.set_mask_embedding(mask_embedding=sam.mask_encoder.get_no_mask_dense_embedding((64, 64), batch_size=P))
                    dec.set_point_embedding(point_embedding=point_embedding.to(dt))
                    dec.set_dense_positional_embedding(dense_positional_embedding=sam.point_encoder.get_dense_positional_embedding(image_embedding_size=(64, 64)).to(dt))
                    low, _iou = dec()
                    return postprocess_masks(low, size, 1024) > 0

            a, b = engine()[0], unfused()
            assert fast.stats["whole_fallback"] is None
            agree = float((a == b).float().mean())
            n = 20 if P < 64 else 5
            runs = [(timeit(engine, n), timeit(unfused, max(n // 4, 2))) for _ in range(3)]
            e, u = sorted(r[0] for r in runs), sorted(r[1] for r in runs)
            print(json.dumps({"workload": "hq_sam_mask_prediction", "dtype": str(dt).split(".")[-1], "P": P, "engine_ms": round(e[1], 3), "engine_ms_min_max": [round(e[0], 3), round(e[2], 3)],
                              "unfused_ms": round(u[1], 3), "unfused_ms_min_max": [round(u[0], 3), round(u[2], 3)], "speedup": round(u[1] / e[1], 2),
                              "binary_masks_equal": round(agree, 5), "step_ops": fast.stats.get("step_ops")}), flush=True)


if __name__ == "__main__":
    main()
