"""pytest -m gpu: the glue kernels of csrc/elementwise.hip (relpos_pack, pointwise_nchw, colsum_rows, sag_degrade, silu, axpby, concat2,
cfg_ddim_step) and the LayerNorm / GroupNorm edges of csrc/norm.hip against float64 references of the same operation (tests/glue_cases.py).

Pure data movement must be bit-equal; arithmetic is held to kernel_cases._tol (1e-3 float32, 1.6e-2 bfloat16, relative to the reference's
max-abs), colsum_rows to its derived per-column bound.  Every case prints its observed error.

The sag_*_nearest_* cases are the ones the integer cell formula (py * ah / h) failed: at 122 rows from 16 cells and 198 from 50, row 61 / 99
read the neighbouring cell, and with a mass alternating per cell that turns a blurred pixel into an untouched one.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from refiners_amd import native  # noqa: E402
from tests import glue_cases  # noqa: E402

CASES = glue_cases.all_cases()


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from refiners_amd.build_native import build_native

    build_native()
    native.load()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_glue_parity(name):
    err, scale, tol = dict(CASES)[name]()
    torch.cuda.synchronize()
    print(f"{name}: max|err| {err:.3e}, reference max {scale:.3e}, bar {tol:g} relative")
    assert err <= tol * scale, f"{name}: max|err|={err:.3e} vs ref max {scale:.3e} (tol {tol:g} relative)"
