"""Golden vectors of the SAM mask decoder: the REAL reference's SegmentAnythingH.predict on CPU float32 with the synthetic per-key
weights of refiners_amd/synth.py and a seeded [1, 256, 64, 64] image embedding (the ViT does not run).  Run where refiners' sources
are (REFINERS_SRC, else the copy __graft_entry__.build() stages under oracle/_ref/src); not on a GPU box:
    python tools/make_golden_sam_decoder.py
Writes tests/golden/sam_h_decoder_keys.json (every state-dict key of SegmentAnythingH, in order, with its shape) and
tests/golden/sam_h_decoder.safetensors (per case: iou, strided samples and statistics of the masks; tests/sam_decoder_cases.py)."""
from __future__ import annotations

import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")
sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF), str(ROOT)]

import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

from refiners.foundationals.segment_anything.mask_decoder import MaskDecoder  # noqa: E402
from refiners.foundationals.segment_anything.model import ImageEmbedding, SegmentAnythingH  # noqa: E402

from refiners_amd import synth  # noqa: E402
from tests.sam_decoder_cases import SAM_DECODER_CASE, SAM_DECODER_CASES, decoder_sample, embedding, low_res_mask  # noqa: E402

GOLD = ROOT / "tests" / "golden"


def decoder_weights(shapes: dict) -> dict:
    """Synthetic weights of everything but the image encoder (which the fixtures never run)."""
    return synth.synth_state_dict({k: v for k, v in shapes.items() if not k.startswith("SAMViTH.")}, SAM_DECODER_CASE["weight_seed"])


def main() -> None:
    t0 = time.time()
    # (SegmentAnything.__init__ moves the whole model to "cpu" whatever its parts were built on: the ViT-H's random init is paid per case)
    shapes = synth.model_shapes(SegmentAnythingH())
    (GOLD / "sam_h_decoder_keys.json").write_text(json.dumps({k: list(v) for k, v in shapes.items()}))
    sd = decoder_weights(shapes)
    out = {}
    for name, case in SAM_DECODER_CASES.items():
        sam = SegmentAnythingH(mask_decoder=MaskDecoder(multimask_output=case["multimask"]))
        sam.load_state_dict(sd, strict=False)
        kw = {k: case[k] for k in ("foreground_points", "background_points", "box_points") if k in case}
        if case.get("low_res_mask"):
            kw["low_res_mask"] = low_res_mask()
        masks, iou, low = sam.predict(ImageEmbedding(embedding(), case["original_size"]), binarize=False, **kw)
        frac = float((masks > 0).double().mean())
        assert 0.05 <= frac <= 0.95, f"{name}: degenerate masks ({frac:.3f} positive): choose another seed"
        for k, v in decoder_sample(masks, iou, low).items():
            out[f"{name}.{k}"] = v.contiguous()
        print(name, tuple(masks.shape), tuple(iou.shape), tuple(low.shape), f"positive {frac:.3f}", iou.flatten().tolist())
    save_file(out, str(GOLD / "sam_h_decoder.safetensors"))
    print(f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
