"""Records what the six solver-step entry points compute, bit for bit, per case of tests/solver_step_cases.py:
    python tools/make_golden_step_bits.py [--out PATH]        (on the GPU; default tests/golden/solver_step_bits.safetensors)
It calls only the public wrappers native.cfg_ddim_step, cfg_linear_step, ddim_step, linear_step, cfg_sde_step and sde_step, so it runs unchanged
on either side of a change to the kernels behind them.  The committed file was written by the library of the commit before those entry points moved
onto one kernel (csrc/solver_step.hip); tests/test_solver_step_kernels_gpu.py::test_bits_are_the_parent_commits holds every later library to it."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]

import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

from refiners_amd import native  # noqa: E402
from tests import solver_step_cases as SC  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(SC.GOLD))
    args = ap.parse_args()
    native.load()
    coefs = SC.coefficient_rows()
    out = dict(coefs)
    records = 0
    for tname, dtype in SC.DTYPES.items():
        for layout in SC.LAYOUTS:
            inp = SC.inputs(dtype, layout)
            out.update({f"{tname}.{layout}.in.{k}": v for k, v in inp.items()})
            for entry in SC.ENTRIES:
                got = SC.run(native, entry, layout, inp, coefs)
                out.update({f"{tname}.{layout}.{entry}.{k}": v for k, v in got.items()})
                records += 1
    torch.cuda.synchronize()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    save_file({k: v.contiguous() for k, v in out.items()}, args.out)
    print(f"{records} records, {len(out)} tensors, {Path(args.out).stat().st_size} bytes -> {args.out}")


if __name__ == "__main__":
    main()
