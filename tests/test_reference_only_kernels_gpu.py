"""mi355x_attention_joint (include/mi355x_refiners_reference_only.h, csrc/reference_only.hip) against a float32 torch model on the device:
  out[b] = mix[b] * SDPA(q, [k0 ; k1], [v0 ; v1]) + (1 - mix[b]) * SDPA(q, k0, v0)
at SD1.5's head widths 40 / 80 / 160, float32 and bfloat16, at the smallest shapes that reach each branch: both segments a fraction of one
64-key tile (16, 16), exactly one tile each (64, 64), odd lengths with two masked tail tiles (100, 37), and four tiles each with two workgroups
per head (256, 256).  Inputs are rounded to the tested dtype first; the model works in float32 from the rounded values.

The bars are tests/kernel_cases._tol: max |err| <= 1e-3 (float32) / 1.6e-2 (bfloat16) of the reference's max-abs.  Every V^T padding column (up to
the next 64 keys of its segment) holds a finite non-zero value, so a tail tile that is not masked by its own segment's Lk shows."""
import math

import pytest
import torch

from refiners_amd import native
from tests.attn_general_bits_cases import _vt  # ([B, Lk, C] -> V^T [C, B, Lkp] whose padding columns are finite and NOT zero)
from tests.kernel_cases import _cmp, _rand

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
H = 2
LENGTHS = [(16, 16), (64, 64), (100, 37), (256, 256)]
MIXES = [(0.5, 1.0), (0.0, 1.0), (1.0, 1.0), (0.3, 0.7)]


def _sdpa(q, k, v, D):
    B, Lq, C = q.shape
    qh, kh, vh = (t.float().reshape(B, -1, C // D, D).transpose(1, 2) for t in (q, k, v))
    att = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(D), dim=-1)
    return (att @ vh).transpose(1, 2).reshape(B, Lq, C)


def _model(q, k0, v0, k1, v1, mix, D):
    m = torch.tensor(mix, device=q.device, dtype=torch.float32).reshape(-1, 1, 1)
    return m * _sdpa(q, torch.cat([k0, k1], 1), torch.cat([v0, v1], 1), D) + (1 - m) * _sdpa(q, k0, v0, D)


def _inputs(D, L0, L1, dtype, seed, B=2):
    C = H * D
    q = _rand(B, L0, C, dtype=dtype, seed=seed)
    k0, v0 = _rand(B, L0, C, dtype=dtype, seed=seed + 1), _rand(B, L0, C, dtype=dtype, seed=seed + 2)
    k1, v1 = _rand(B, L1, C, dtype=dtype, seed=seed + 3), _rand(B, L1, C, dtype=dtype, seed=seed + 4, scale=2.0)  # (the guide's values stand out)
    return q, k0, v0, k1, v1


def _run(q, k0, v0, k1, v1, mix, out=None):
    """Launch into a NaN-filled buffer with one guard row per sample: (out, guard rows)."""
    B, Lq, C = q.shape
    buf = torch.full((B, Lq + 1, C), NAN, dtype=q.dtype, device=DEV)
    m = None if mix is None else torch.tensor(mix, device=DEV, dtype=torch.float32)
    native.attention_joint(q, k0, _vt(v0), k0.shape[1], k1, _vt(v1), k1.shape[1], buf[:, :Lq], H, mix=m)
    torch.cuda.synchronize()
    return buf[:, :Lq], buf[:, Lq]


def _assert_close(out, ref, dtype, what):
    err, mag, tol = _cmp(out, ref, dtype)
    print(f"{what}: max |err| = {err:.3e}, max |ref| = {mag:.3e}, err / (tol * max |ref|) = {err / (tol * mag):.3f}")
    assert err <= tol * mag, (what, err, mag)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L0,L1", LENGTHS)
@pytest.mark.parametrize("D", [40, 80, 160])
def test_joint_attention_against_float32_model(D, L0, L1, dtype):
    q, k0, v0, k1, v1 = _inputs(D, L0, L1, dtype, seed=D + L0 + L1)
    for mix in MIXES:
        out, guard = _run(q, k0, v0, k1, v1, mix)  # (the output buffer is pre-filled with NaN: _cmp refuses a non-finite value)
        assert torch.isnan(guard).all(), "wrote past the last query row"
        _assert_close(out, _model(q, k0, v0, k1, v1, mix, D), dtype, f"D={D} L=({L0},{L1}) mix={mix}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L0,L1", LENGTHS)
@pytest.mark.parametrize("D", [40, 80, 160])
def test_mix_one_and_zero_match_attention_general(D, L0, L1, dtype):
    """mix = [1, 1] (and a NULL mix) is attention_general over the concatenated keys, mix = [0, 0] attention_general over segment 0."""
    q, k0, v0, k1, v1 = _inputs(D, L0, L1, dtype, seed=3 * D + L0 + L1)
    B, Lq, C = q.shape
    both = torch.full((B, Lq, C), NAN, dtype=dtype, device=DEV)
    native.attention_general(q, torch.cat([k0, k1], 1), _vt(torch.cat([v0, v1], 1)), both, H, L0 + L1)
    own = torch.full((B, Lq, C), NAN, dtype=dtype, device=DEV)
    native.attention_general(q, k0, _vt(v0), own, H, L0)
    for mix, ref in (((1.0, 1.0), both), (None, both), ((0.0, 0.0), own)):
        out, _ = _run(q, k0, v0, k1, v1, mix)
        _assert_close(out, ref.float(), dtype, f"D={D} L=({L0},{L1}) mix={mix} against attention_general")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["late_in_segment_1", "late_in_segment_0"])
@pytest.mark.parametrize("D", [40, 160])
def test_spiked_key(D, where, dtype):
    """One key far above the others: late in segment 1 the running maximum jumps AFTER the snapshot was taken (the parked term must not be
    rescaled with the accumulator); late in segment 0 it jumps just before it."""
    L0, L1 = 100, 150
    q, k0, v0, k1, v1 = _inputs(D, L0, L1, dtype, seed=17 + D)
    if where == "late_in_segment_1":
        k1[:, L1 - 3] *= 6.0
    else:
        k0[:, L0 - 2] *= 6.0
    for mix in ((0.5, 1.0), (0.3, 0.7)):
        out, _ = _run(q, k0, v0, k1, v1, mix)
        _assert_close(out, _model(q, k0, v0, k1, v1, mix, D), dtype, f"spike {where} D={D} mix={mix}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [40, 80, 160])
def test_keys_as_column_slices_of_a_wider_buffer(D, dtype):
    """K as the second half of a [B * L, 2 C] Q|K buffer (what the Q|K|V^T projection writes), Q as its first half."""
    B, L0, L1, C = 2, 100, 37, H * D
    qk0 = _rand(B, L0, 2 * C, dtype=dtype, seed=5 + D)
    qk1 = _rand(B, L1, 2 * C, dtype=dtype, seed=6 + D)
    v0, v1 = _rand(B, L0, C, dtype=dtype, seed=7 + D), _rand(B, L1, C, dtype=dtype, seed=8 + D)
    q, k0, k1 = qk0[:, :, :C], qk0[:, :, C:], qk1[:, :, C:]
    mix = (0.5, 1.0)
    out, guard = _run(q, k0, v0, k1, v1, mix)
    assert torch.isnan(guard).all()
    _assert_close(out, _model(q, k0, v0, k1, v1, mix, D), dtype, f"column slices D={D}")


def test_mix_is_read_from_device_memory_at_every_launch():
    """The same recorded arguments follow a new value of the device buffer (what a captured graph replays)."""
    D, L0, L1, dtype = 40, 64, 64, torch.float32
    q, k0, v0, k1, v1 = _inputs(D, L0, L1, dtype, seed=99)
    mix = torch.tensor([0.5, 1.0], device=DEV)
    out = torch.full_like(q, NAN)
    vt0, vt1 = _vt(v0), _vt(v1)
    for value in (0.5, 1.0, 0.0, 0.25):
        mix[0] = value
        native.attention_joint(q, k0, vt0, L0, k1, vt1, L1, out, H, mix=mix)
        _assert_close(out, _model(q, k0, v0, k1, v1, (value, 1.0), D), dtype, f"live mix {value}")


def test_bits_are_the_parent_commits():
    """Every case of tests/attn_general_bits_cases.py (each (QK steps, PV blocks) instance of mi355x_attention_general in float32, bfloat16 with the
    lazy maximum and bfloat16 without; each instance of mi355x_attention_joint with a snapshot, without one and with segment 1 skipped) writes
    the bits that the library before the two kernels moved onto one tile loop wrote (tests/golden/attn_general_bits.safetensors), NaN guard
    rows included.  No tolerance, nothing skipped."""
    from tests import attn_general_bits_cases as AC
    from tests.support import golden

    gold = golden(AC.NAME)
    assert set(gold) == set(AC.CASES) and len(AC.CASES) == 3 * 10 + 2 * 7
    for case in AC.CASES:
        got, want = AC.run(native, case), gold[case]
        assert got.dtype == want.dtype and got.shape == want.shape, case
        assert torch.isnan(got[:, -1]).all() and not torch.isnan(got[:, :-1]).any(), f"{case}: guard row written, or an output element left unwritten"
        differ = AC.bits(got) != AC.bits(want)
        assert torch.equal(AC.bits(got), AC.bits(want)), f"{case}: {int(differ.sum())} of {got.numel()} elements differ"


def test_argument_refusals():
    D, L0, L1, dtype = 40, 64, 64, torch.float32
    q, k0, v0, k1, v1 = _inputs(D, L0, L1, dtype, seed=1)
    vt0, vt1 = _vt(v0), _vt(v1)
    out = torch.full_like(q, NAN)
    with pytest.raises(native.NativeError, match="ESHAPE"):  # a head width no instance serves
        qq = _rand(2, 64, H * 192, dtype=dtype, seed=2)
        native.attention_joint(qq, qq, _vt(qq), 64, qq, _vt(qq), 64, torch.empty_like(qq), H)
    with pytest.raises(native.NativeError, match="ESHAPE"):  # an empty segment
        native.attention_joint(q, k0, vt0, L0, k1, vt1, 0, out, H)
    with pytest.raises(native.NativeError, match="ESHAPE"):
        native.attention_joint(q, k0, vt0, 0, k1, vt1, L1, out, H)
    for alias in (q, k0, k1):  # out overlapping an input
        with pytest.raises(native.NativeError, match="EARG"):
            native.attention_joint(q, k0, vt0, L0, k1, vt1, L1, alias, H)
    with pytest.raises(native.NativeError, match="EARG"):
        native.attention_joint(q, k0, vt0, L0, k1, vt1, L1, vt0.view(-1)[: q.numel()].view_as(q), H)  # (a V^T buffer, seen as an output)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to its output"
