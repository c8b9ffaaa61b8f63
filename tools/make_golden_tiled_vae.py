"""Golden vectors of the tiled VAE: the REAL reference's SDXLAutoencoder inside `with lda.tiled_inference(image, tile_size, blending):`, synthetic
weights (tests/golden/vae_keys.json, seed 0), CPU float32, per case of tests/tiled_vae_cases.py:
    <case>.calibration     the tensor _add_fixed_group_norm feeds to encode (captured by wrapping encode), so that no GPU test needs PIL
    <case>.gn_mean / .gn_var   every FixedGroupNorm's statistics, [nodes, 32], in walk order
    <case>.image_u8        the image as uint8 (H, W, 3); tests/tiled_vae_cases.image_tensor() turns it into the tensor _tiled_encode is given
    <case>.encoded         _tiled_encode's result
    <case>.latents / .decoded  the latents given to _tiled_decode and its result
and tiled_vae.json: per case the tile list of _generate_latent_tiles, plus the blending masks of one interior and one corner tile of GEOMETRY_C.
Before writing, the reference's `weights` tensor of every multi-tile case and of GEOMETRY_C is checked to be strictly positive.
Run where refiners' sources are (the build container), not on a GPU box:
    python tools/make_golden_tiled_vae.py
-> tests/golden/tiled_vae.safetensors, tests/golden/tiled_vae.json"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

import torch  # noqa: E402
from PIL import Image  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

import oracle.make_golden  # noqa: E402,F401  (puts the reference package and the jaxtyping shim on sys.path)

from refiners.foundationals.latent_diffusion.auto_encoder import FixedGroupNorm, _create_blending_mask, _ImageSize  # noqa: E402
from refiners.foundationals.latent_diffusion.stable_diffusion_xl.model import SDXLAutoencoder  # noqa: E402

from refiners_amd import synth  # noqa: E402
from tests.tiled_vae_cases import GEOMETRY_C, TILE, TILED_VAE_CASES, WEIGHT_SEED, case_image_u8, case_latents, image_tensor  # noqa: E402

GOLD = ROOT / "tests" / "golden"


def weights_of(tiles: list, size: _ImageSize, blending: int, scale: int) -> torch.Tensor:
    """The `weights` tensor of _tiled_encode (scale 1, blending in latents) / _tiled_decode (scale 8, blending in pixels), one channel."""
    w = torch.zeros(size.height * scale, size.width * scale)
    for t in tiles:
        edge = (t.top == 0, t.bottom == size.height, t.left == 0, t.right == size.width)
        m = _create_blending_mask(_ImageSize((t.bottom - t.top) * scale, (t.right - t.left) * scale), blending, 1, is_edge=edge)
        w[t.top * scale : t.bottom * scale, t.left * scale : t.right * scale] += m[0, 0]
    return w


def checked_tiles(lda, name: str, case: dict) -> list:
    size = _ImageSize(height=case["latent_wh"][1], width=case["latent_wh"][0])
    tiles = lda._generate_latent_tiles(size, _ImageSize(height=TILE[1] // 8, width=TILE[0] // 8), overlap=case["blending"] // 8)
    nx, ny = case["grid"]
    assert len(tiles) == nx * ny, (name, len(tiles))
    if len(tiles) > 1:
        for blending, scale in ((case["blending"] // 8, 1), (case["blending"], 8)):
            assert bool((weights_of(tiles, size, blending, scale) > 0).all()), f"case {name}: an element of weight zero at scale {scale}; change the sizes"
    return tiles


def main() -> None:
    shapes = {k: tuple(v) for k, v in json.loads((GOLD / "vae_keys.json").read_text()).items()}
    lda = SDXLAutoencoder(device="meta")
    lda.load_state_dict(synth.synth_state_dict(shapes, WEIGHT_SEED), assign=True)
    out, meta = {}, {}
    for name, case in TILED_VAE_CASES.items():
        t0 = time.time()
        tiles = checked_tiles(lda, name, case)
        u8 = case_image_u8(case)
        image = Image.fromarray(u8.numpy())
        seen: list = []
        plain_encode = lda.encode

        def recording_encode(x, plain_encode=plain_encode, seen=seen):
            seen.append(x.clone())
            return plain_encode(x)

        lda.encode = recording_encode  # type: ignore[method-assign]
        try:
            with lda.tiled_inference(image, tile_size=TILE, blending=case["blending"]):
                del lda.encode  # only the calibration call is recorded
                fixed = [f for f, _ in lda.walk(FixedGroupNorm)]
                out[f"{name}.gn_mean"] = torch.stack([f.mean for f in fixed]).contiguous()
                out[f"{name}.gn_var"] = torch.stack([f.var for f in fixed]).contiguous()
                x = image_tensor(u8)
                assert torch.equal(x, 2 * torch.tensor(__import__("numpy").array(image).astype("float32") / 255.0).permute(2, 0, 1)[None] - 1)
                out[f"{name}.encoded"] = lda._tiled_encode(x, lda._tile_size, case["blending"]).contiguous()
                z = case_latents(case)
                out[f"{name}.latents"] = z
                out[f"{name}.decoded"] = lda._tiled_decode(z, lda._tile_size, case["blending"]).contiguous()
        finally:
            lda.__dict__.pop("encode", None)
        assert len(seen) == 1 and tuple(seen[0].shape) == (1, 3, TILE[1], TILE[0])
        out[f"{name}.calibration"] = seen[0].contiguous()
        out[f"{name}.image_u8"] = u8
        meta[name] = {"tiles": [list(t) for t in tiles]}
        print(name, len(tiles), "tiles", f"{time.time() - t0:.1f}s", flush=True)
    ctiles = checked_tiles(lda, "c", GEOMETRY_C)
    b = GEOMETRY_C["blending"] // 8
    meta["c"] = {"tiles": [list(t) for t in ctiles],
                 "mask_interior": _create_blending_mask(_ImageSize(8, 8), b, 1)[0, 0].tolist(),
                 "mask_corner_6x7": _create_blending_mask(_ImageSize(6, 7), b, 1, is_edge=(False, True, False, True))[0, 0].tolist()}
    (GOLD / "tiled_vae.json").write_text(json.dumps(meta, indent=None, separators=(",", ":")) + "\n")
    save_file(out, str(GOLD / "tiled_vae.safetensors"))
    print((GOLD / "tiled_vae.safetensors").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
