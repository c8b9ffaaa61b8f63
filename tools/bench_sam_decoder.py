"""SAM mask decoder timing, bf16, one 1024 x 1024 image embedding, P = 1 / 16 / 64 prompt sets of one foreground point each: the MI355X
engine (CompiledSegmentAnything.predict_batch: point encoder in torch, one graph replay, postprocess_masks kernel) against the mirror's
unfused torch forward on the same GPU with the embedding repeated P times.  Prints one JSON line (milliseconds per batch)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from refiners_amd import synth  # noqa: E402
from refiners_amd.engine.sam_decoder import CompiledSegmentAnything  # noqa: E402
from refiners_amd.segment_anything import PointType, SegmentAnythingH, postprocess_masks  # noqa: E402


def timeit(fn, n=10):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def main():
    dt, dev = torch.bfloat16, torch.device("cuda")
    sam = SegmentAnythingH(device=dev, dtype=dt)
    shapes = {k: tuple(v.shape) for k, v in sam.state_dict().items() if not k.startswith("SAMViTH.")}
    sam.load_state_dict({k: v.to(dev, dt) for k, v in synth.synth_state_dict(shapes, 0).items()}, strict=False)
    fast = CompiledSegmentAnything(sam)
    emb = torch.randn(1, 256, 64, 64, device=dev).to(dt)
    size = (1024, 1024)
    out = {"workload": "sam_h_mask_decoder", "dtype": "bf16", "image": list(size), "multimask": True}
    dec = sam.mask_decoder
    pe = sam.point_encoder.get_dense_positional_embedding(image_embedding_size=(64, 64))
    for P in (1, 16, 64):
        g = torch.Generator().manual_seed(P)
        pts = torch.rand(P, 1, 2, generator=g) * 1024
        types = torch.full((P, 1), PointType.FOREGROUND.value)
        engine = timeit(lambda: fast.predict_batch(emb, pts, types, original_size=size))

        def unfused():
            with torch.no_grad():
                # (the tree's own PointTypeEmbedding cannot run in bfloat16: the point rows come from the engine's float32 copy of it)
                point_embedding = torch.stack([fast._sparse(pts[p], types[p], size)[5:] for p in range(P)])
                dec.set_image_embedding(image_embedding=emb.expand(P, -1, -1, -1).contiguous())
                dec.set_mask_embedding(mask_embedding=sam.mask_encoder.get_no_mask_dense_embedding((64, 64), batch_size=P))
                dec.set_point_embedding(point_embedding=point_embedding.to(dt))
                dec.set_dense_positional_embedding(dense_positional_embedding=pe)
                low, _iou = dec()
                return postprocess_masks(low, size, 1024) > 0

        out[f"P{P}_engine_ms"] = round(engine, 3)
        out[f"P{P}_unfused_ms"] = round(timeit(unfused, n=3), 3)
        out[f"P{P}_speedup"] = round(out[f"P{P}_unfused_ms"] / engine, 2)
    out["step_ops"] = fast.stats.get("step_ops")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
