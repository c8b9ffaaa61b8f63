"""Cases of the InformativeDrawings fixtures (tests/golden/lineart_keys.json and lineart.safetensors, written by tools/make_golden_lineart.py
from the reference's own class): model configurations, the synthetic weight draw and seeded inputs.  The 17 MB of weights are not stored: they
are drawn per key from a seeded CPU generator over the reference's key / shape list."""
from __future__ import annotations

import json
from functools import lru_cache
from pathlib import Path

LINEART_SEED = dict(weight_seed=17, input_seed=71)

#: name -> residual blocks + input geometry (in_channels 3, out_channels 1 throughout)
#:   A  the default model, even at every stage
#:   B  batch 2; odd at every stage (37 -> 19 -> 10, 50 -> 25 -> 13); output 40 x 52 != input
#:   C  2 x 3 residual maps: the reflected ring is most of the image
#:   D  more than one workgroup tile per image in every kernel
#:   E  the smallest size the reference accepts; no residual block
LINEART_CASES = {
    "A": dict(n_residual_blocks=3, shape=(1, 3, 40, 56)),
    "B": dict(n_residual_blocks=3, shape=(2, 3, 37, 50)),
    "C": dict(n_residual_blocks=1, shape=(1, 3, 8, 12)),
    "D": dict(n_residual_blocks=3, shape=(1, 3, 128, 96)),
    "E": dict(n_residual_blocks=0, shape=(1, 3, 5, 5)),
}
BLOCK_COUNTS = (0, 1, 3)  # the key lists the fixture stores


def out_shape(case: str) -> tuple[int, int, int, int]:
    b, _c, h, w = LINEART_CASES[case]["shape"]
    q = lambda n: ((n + 1) // 2 + 1) // 2  # noqa: E731
    return (b, 1, 4 * q(h), 4 * q(w))


def image(case: str, shift: int = 0):
    import torch

    g = torch.Generator().manual_seed(LINEART_SEED["input_seed"] + sum(map(ord, case)) + 1000 * shift)
    return torch.rand(LINEART_CASES[case]["shape"], generator=g)


@lru_cache(maxsize=None)
def reference_tree(n_residual_blocks: int) -> dict:
    """{"repr": the reference's repr on the meta device, "keys": {state-dict key: shape}, in the reference's order}."""
    entry = json.loads((Path(__file__).resolve().parent / "golden" / "lineart_keys.json").read_text())[str(n_residual_blocks)]
    return {"repr": entry["repr"], "keys": {k: tuple(v) for k, v in entry["keys"].items()}}


def key_shapes(n_residual_blocks: int) -> dict[str, tuple[int, ...]]:
    return reference_tree(n_residual_blocks)["keys"]


def draw_weights(shapes: dict) -> dict:
    from refiners_amd import synth

    return synth.synth_state_dict(shapes, LINEART_SEED["weight_seed"])


def weights(case: str) -> dict:
    return draw_weights(key_shapes(LINEART_CASES[case]["n_residual_blocks"]))


def mirror(case: str, device="cpu", dtype=None, **overrides):
    """The mirror's InformativeDrawings of a case with the fixture's weights loaded (a variant -- other channels, say -- draws over its own keys)."""
    import torch

    from refiners_amd.latent_diffusion.preprocessors import InformativeDrawings

    dtype = dtype or torch.float32
    model = InformativeDrawings(**{"n_residual_blocks": LINEART_CASES[case]["n_residual_blocks"], **overrides}, device="meta")
    drawn = draw_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}) if overrides else weights(case)
    model.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in drawn.items()}, assign=True)
    return model
