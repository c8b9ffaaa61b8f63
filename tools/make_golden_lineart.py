"""Golden vectors of the lineart preprocessor: the REAL reference's InformativeDrawings on CPU float32 with the synthetic per-key weights of
tests/lineart_cases.py and seeded `torch.rand` images.  Run where refiners' sources are (REFINERS_SRC, else the copy
__graft_entry__.build() stages under oracle/_ref/src); not on a GPU box:
    python tools/make_golden_lineart.py
Writes tests/golden/lineart_keys.json (for 0, 1 and 3 residual blocks the reference's repr on the meta device and its state-dict keys, in
order, with their shapes) and tests/golden/lineart.safetensors ("{case}.out": the whole output of every case; 75 KB in all).  Prints the
distance of the float32 output to the reference's own float64 forward."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")
sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF), str(ROOT)]

import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

from refiners.foundationals.latent_diffusion.preprocessors.informative_drawings import InformativeDrawings  # noqa: E402

from tests.lineart_cases import BLOCK_COUNTS, LINEART_CASES, draw_weights, image, out_shape  # noqa: E402

GOLD = ROOT / "tests" / "golden"


def main() -> None:
    keys = {}
    for n in BLOCK_COUNTS:
        model = InformativeDrawings(n_residual_blocks=n, device="meta")
        keys[str(n)] = {"repr": repr(model), "keys": {k: list(v.shape) for k, v in model.state_dict().items()}}
    (GOLD / "lineart_keys.json").write_text(json.dumps(keys))
    out = {}
    for name, case in LINEART_CASES.items():
        model = InformativeDrawings(n_residual_blocks=case["n_residual_blocks"])
        sd = draw_weights({k: tuple(v.shape) for k, v in model.state_dict().items()})
        model.load_state_dict(sd)
        x = image(name)
        with torch.no_grad():
            y = model(x)
            y64 = model.to(dtype=torch.float64)(x.double())
        assert tuple(y.shape) == out_shape(name) and torch.isfinite(y).all()
        out[f"{name}.out"] = y.contiguous()
        print(name, tuple(y.shape), f"range {float(y.min()):.3f} .. {float(y.max()):.3f}; float32 against float64: max abs {float((y.double() - y64).abs().max()):.2e}")
    path = GOLD / "lineart.safetensors"
    save_file(out, str(path))
    print(path.name, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
