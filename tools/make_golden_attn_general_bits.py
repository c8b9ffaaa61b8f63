"""Records what mi355x_attention_general and mi355x_attention_joint compute, bit for bit, per case of tests/attn_general_bits_cases.py:
    python tools/make_golden_attn_general_bits.py [--out PATH]        (on the GPU; default tests/golden/attn_general_bits.safetensors)
It calls only native.attention_general, native.attention_joint and mi355x_attention_general_set_fast, so it runs unchanged on either side of a
change to the kernels behind them.  The committed file was written by the library of the commit before the two kernels moved onto one tile loop
(csrc/attn_general_kernel.cuh); tests/test_reference_only_kernels_gpu.py::test_bits_are_the_parent_commits holds every later library to it."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

from safetensors.torch import save_file  # noqa: E402

from refiners_amd import native  # noqa: E402
from tests import attn_general_bits_cases as AC  # noqa: E402


SHARD_BYTES = 900 * 1024  # (a committed file stays under 1 MiB)


def save_sharded(out: dict, path: Path) -> list[Path]:
    """Whole records, in order, into `<name>.safetensors`, `<name>.1.safetensors`, ... (what tests/support.golden reads back as one dict)."""
    shards: list[dict] = [{}]
    for k, v in out.items():
        if shards[-1] and sum(t.numel() * t.element_size() for t in shards[-1].values()) + v.numel() * v.element_size() > SHARD_BYTES:
            shards.append({})
        shards[-1][k] = v
    paths = [path if i == 0 else path.with_suffix(f".{i}.safetensors") for i in range(len(shards))]
    for p, s in zip(paths, shards):
        save_file(s, str(p))
    return paths


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / f"{AC.NAME}.safetensors"))
    args = ap.parse_args()
    native.load()
    out = {case: AC.run(native, case).contiguous() for case in AC.CASES}
    written = sum(int((AC.bits(v) != AC.bits(v.new_full((), AC.NAN))).sum()) for v in out.values())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    paths = save_sharded(out, Path(args.out))
    print(f"{len(out)} records, {written} elements written by a kernel -> " + ", ".join(f"{p} ({p.stat().st_size} bytes)" for p in paths))


if __name__ == "__main__":
    main()
