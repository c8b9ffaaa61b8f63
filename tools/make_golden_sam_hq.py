"""Golden vectors of HQ-SAM mask prediction: the REAL reference's SegmentAnythingH(multimask_output=False) with its HQSAMAdapter injected,
predict() on CPU float32 with the synthetic per-key weights of refiners_amd/synth.py, the seeded image embedding of the SAM decoder fixtures
and a seeded early ViT embedding (the ViT does not run).  Run where refiners' sources are (REFINERS_SRC, else the copy
__graft_entry__.build() stages under oracle/_ref/src); not on a GPU box:
    python tools/make_golden_sam_hq.py
Writes tests/golden/sam_hq_keys.json (the adapter's weight keys, in order, with their shapes) and tests/golden/sam_hq_decoder.safetensors
(per case of tests/sam_hq_cases.py what decoder_sample keeps: iou, strided samples and statistics of the masks)."""
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

from refiners.foundationals.segment_anything.hq_sam import HQSAMAdapter  # noqa: E402
from refiners.foundationals.segment_anything.model import ImageEmbedding, SegmentAnythingH  # noqa: E402

from refiners_amd import synth  # noqa: E402
from tests.sam_hq_cases import SAM_HQ_CASE, SAM_HQ_CASES, decoder_sample, early_embedding, embedding, low_res_mask, prompt_kwargs  # noqa: E402

GOLD = ROOT / "tests" / "golden"


def main() -> None:
    t0 = time.time()
    base = {k: tuple(v) for k, v in json.loads((GOLD / "sam_h_decoder_keys.json").read_text()).items() if not k.startswith("SAMViTH.")}
    sd = synth.synth_state_dict(base, SAM_HQ_CASE["weight_seed"])
    sam = SegmentAnythingH(multimask_output=False)
    sam.load_state_dict(sd, strict=False)
    adapter = HQSAMAdapter(sam)
    shapes = {k: tuple(v.shape) for k, v in adapter.weights.items()}
    (GOLD / "sam_hq_keys.json").write_text(json.dumps({k: list(v) for k, v in shapes.items()}))
    adapter.load_weights(synth.synth_state_dict(shapes, SAM_HQ_CASE["hq_weight_seed"]))
    adapter.inject()
    out = {}
    for name, case in SAM_HQ_CASES.items():
        adapter.hq_mask_only = case["hq_mask_only"]
        adapter.set_context("hq_sam", {"early_vit_embedding": early_embedding()})
        kw = prompt_kwargs(case)
        if case.get("low_res_mask"):
            kw["low_res_mask"] = low_res_mask()
        t1 = time.time()
        masks, iou, low = sam.predict(ImageEmbedding(embedding(), case["original_size"]), binarize=False, **kw)
        frac = float((masks > 0).double().mean())
        assert 0.05 <= frac <= 0.95, f"{name}: degenerate masks ({frac:.3f} positive): choose another seed"
        for k, v in decoder_sample(masks, iou, low).items():
            out[f"{name}.{k}"] = v.contiguous()
        print(name, tuple(masks.shape), tuple(iou.shape), tuple(low.shape), f"positive {frac:.3f}", iou.flatten().tolist(), f"{time.time() - t1:.2f}s")
    save_file(out, str(GOLD / "sam_hq_decoder.safetensors"))
    print(f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
