"""Golden vectors of the DINOv2 encoder: the REAL reference's foundationals.dinov2.vit.ViT on CPU float32 with the synthetic per-key weights
of tests/dinov2_cases.py (LayerScale weights uniform in +-[0.05, 1.5]; position table, class token and registers of standard deviation
0.5) and a seeded image.  Run where refiners' sources are (REFINERS_SRC, else the copy __graft_entry__.build() stages under
oracle/_ref/src); not on a GPU box:
    python tools/make_golden_dinov2.py
Writes tests/golden/dinov2_keys.json (per case, and per named model, the state-dict keys, in order, with their shapes; a named model's
identical layers are stored once, dinov2_cases.fold_layers) and
tests/golden/dinov2.safetensors, dinov2.1.safetensors, ... (per case what dinov2_cases.output_sample keeps of the output; shards as
tests/support.golden reads them, each below the size of the largest fixture already committed)."""
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

import refiners.fluxion.layers as rfl  # noqa: E402
import refiners.foundationals.dinov2.dinov2 as ref_models  # noqa: E402
from refiners.foundationals.dinov2.vit import ViT  # noqa: E402

from tests.dinov2_cases import DINOV2_CASES, draw_weights, expand_layers, fold_layers, image, model_kwargs, output_sample, tokens  # noqa: E402

GOLD = ROOT / "tests" / "golden"
SHARD_BYTES = 700_000
NAMED = [f"DINOv2_{size}{reg}" for size in ("small", "base", "large", "giant") for reg in ("", "_reg")]


def main() -> None:
    t0 = time.time()
    keys, out = {}, {}
    for name, case in DINOV2_CASES.items():
        model = ViT(**model_kwargs(name, rfl))
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        keys[name] = {k: list(v) for k, v in shapes.items()}
        model.load_state_dict(draw_weights(shapes, name))
        t1 = time.time()
        with torch.no_grad():
            y = model(image(name))
        dt = time.time() - t1
        assert tuple(y.shape) == (case["batch"], tokens(name), case["model"]["embedding_dim"]) and torch.isfinite(y).all()
        for k, v in output_sample(y).items():
            out[f"{name}.{k}"] = v
        print(name, tuple(y.shape), f"{dt:.2f}s")
    for name in NAMED:
        model = getattr(ref_models, name)(device="meta")
        full = {k: list(v.shape) for k, v in model.state_dict().items()}
        keys[name] = fold_layers(full)  # 12 to 40 identical layers: one is stored
        assert list(expand_layers(keys[name]).items()) == list(full.items()), name
    (GOLD / "dinov2_keys.json").write_text(json.dumps(keys))
    for old in GOLD.glob("dinov2*.safetensors"):
        old.unlink()
    shards: list[dict] = [{}]
    size = 0
    for k, v in out.items():
        n = v.numel() * v.element_size()
        if size + n > SHARD_BYTES and shards[-1]:
            shards.append({})
            size = 0
        shards[-1][k] = v
        size += n
    for i, sh in enumerate(shards):
        path = GOLD / ("dinov2.safetensors" if i == 0 else f"dinov2.{i}.safetensors")
        save_file(sh, str(path))
        print(path.name, path.stat().st_size, "bytes")
    print(f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
