"""Golden vectors of the Swin Transformer backbone: the REAL reference's foundationals.swin.SwinTransformer on CPU float32 with the
synthetic per-key weights of tests/swin_cases.py (canonical relative_position_index, bias tables of standard deviation 0.5) and a seeded
image.  Run where refiners' sources are (REFINERS_SRC, else the copy __graft_entry__.build() stages under oracle/_ref/src); not on
a GPU box:
    python tools/make_golden_swin.py
Writes tests/golden/swin_keys.json (per case the model's state-dict keys, in order, with their shapes) and
tests/golden/swin.safetensors, swin.1.safetensors, ... (per case and output what swin_cases.output_sample keeps; shards as
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

from refiners.foundationals.swin.swin_transformer import SwinTransformer  # noqa: E402

from tests.swin_cases import SWIN_CASES, draw_weights, image, output_names, output_sample  # noqa: E402

GOLD = ROOT / "tests" / "golden"
SHARD_BYTES = 700_000


def main() -> None:
    t0 = time.time()
    keys, out = {}, {}
    for name, case in SWIN_CASES.items():
        model = SwinTransformer(**case["model"])
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        keys[name] = {k: list(v) for k, v in shapes.items()}
        model.load_state_dict(draw_weights(shapes, name))
        t1 = time.time()
        with torch.no_grad():
            ys = model(image(name))
        dt = time.time() - t1
        assert len(ys) == len(output_names(name))
        for oname, y in zip(output_names(name), ys):
            assert torch.isfinite(y).all()
            for k, v in output_sample(y).items():
                out[f"{name}.{oname}.{k}"] = v
        print(name, [tuple(y.shape) for y in ys], f"{dt:.2f}s")
    (GOLD / "swin_keys.json").write_text(json.dumps(keys))
    for old in GOLD.glob("swin*.safetensors"):
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
        path = GOLD / ("swin.safetensors" if i == 0 else f"swin.{i}.safetensors")
        save_file(sh, str(path))
        print(path.name, path.stat().st_size, "bytes")
    print(f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
