"""Cases of the recorded bits of mi355x_attention_general and mi355x_attention_joint (tests/golden/attn_general_bits.safetensors, written by
tools/make_golden_attn_general_bits.py from the library of the commit BEFORE the two kernels moved onto one tile loop, csrc/attn_general_kernel.cuh;
read by tests/test_reference_only_kernels_gpu.py::test_bits_are_the_parent_commits).  The smallest shapes that reach every branch of every instance:

general, per type in {f32, bf16 with the lazy maximum (fast = 1), bf16 with the per-tile maximum (fast = 0)}: B = 1, H = 2,
    d<Dqk>x<Dv>  Lq = 40 (one full wave, one wave with 8 live queries, two idle), Lk = 150 (three tiles, the last with 22 keys: both LDS stages),
                 one (Dqk, Dv) per (QK steps, PV blocks) instance
    d40_2wg      Lq = 136: two workgroups per head
    d64_causal   Lq = Lk = 136: diagonal tiles and skipped tiles
    d80_spike    Lk = 470 (eight tiles), key Lk - 3 six times as large: the lazy maximum moves after seven tiles
joint, per type in {f32, bf16}: B = 3 with mix = (0.3, 1.0, 0.0) (snapshot, no snapshot, segment 1 skipped), H = 2, Lq = 40, (Lk0, Lk1) = (100, 37),
    d<D>         one D per instance
    d40_nomix    mix = None
    d160_spike   Lk1 = 150, key Lk1 - 3 of segment 1 six times as large: the reference moves after the snapshot was parked

Inputs come from tests/kernel_cases._rand seeds and are not stored.  Every V^T padding column holds 3.0.  A record is the whole output buffer,
[B, Lq + 1, H * Dv] pre-filled with NaN, whose last row per sample is a guard that no launch may touch: compare bit patterns (`bits`)."""
from __future__ import annotations

import torch

from tests.kernel_cases import DEV, _rand

NAME = "attn_general_bits"
H = 2
NAN = float("nan")
#: type tag -> (storage type, value for mi355x_attention_general_set_fast)
GENERAL_TYPES = {"f32": (torch.float32, 1), "bf16_fast": (torch.bfloat16, 1), "bf16_slow": (torch.bfloat16, 0)}
JOINT_TYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
INSTANCE_WIDTHS = [(40, 40), (64, 64), (80, 80), (112, 80), (128, 128), (160, 160), (208, 80)]
#: shape tag -> (Lq, Lk, Dqk, Dv, causal, spiked key or None)
GENERAL_SHAPES = {
    **{f"d{dqk}x{dv}": (40, 150, dqk, dv, False, None) for dqk, dv in INSTANCE_WIDTHS},
    "d40_2wg": (136, 150, 40, 40, False, None),
    "d64_causal": (136, 136, 64, 64, True, None),
    "d80_spike": (40, 470, 80, 80, False, 467),
}
MIX = (0.3, 1.0, 0.0)
#: shape tag -> (D, Lk0, Lk1, mix, spiked key of segment 1 or None)
JOINT_SHAPES = {
    **{f"d{d}": (d, 100, 37, MIX, None) for d in (40, 64, 80, 128, 160)},
    "d40_nomix": (40, 100, 37, None, None),
    "d160_spike": (160, 100, 150, MIX, 147),
}
CASES = [f"general.{t}.{s}" for t in GENERAL_TYPES for s in GENERAL_SHAPES] + [f"joint.{t}.{s}" for t in JOINT_TYPES for s in JOINT_SHAPES]


def _pad64(n):
    return (n + 63) // 64 * 64


def _vt(v, junk=3.0):
    """[B, Lk, C] -> V^T [C, B, Lkp] whose padding columns are finite and NOT zero."""
    B, Lk, C = v.shape
    vt = torch.full((C, B, _pad64(Lk)), junk, dtype=v.dtype, device=v.device)
    vt[:, :, :Lk] = v.permute(2, 0, 1)
    return vt


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns as integers (NaN compares equal to the same NaN)."""
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def run(native, case: str) -> torch.Tensor:
    """One launch of the case through the public wrapper; returns the whole NaN-prefilled buffer, guard rows included, on the CPU."""
    kind, tname, shape = case.split(".")
    seed = 1000 + 10 * CASES.index(case)
    if kind == "general":
        dtype, fast = GENERAL_TYPES[tname]
        Lq, Lk, Dqk, Dv, causal, spike = GENERAL_SHAPES[shape]
        q = _rand(1, Lq, H * Dqk, dtype=dtype, seed=seed)
        k = _rand(1, Lk, H * Dqk, dtype=dtype, seed=seed + 1)
        v = _rand(1, Lk, H * Dv, dtype=dtype, seed=seed + 2)
        if spike is not None:
            k[:, spike] *= 6.0
        buf = torch.full((1, Lq + 1, H * Dv), NAN, dtype=dtype, device=DEV)
        lib = native.load()
        lib.mi355x_attention_general_set_fast(fast)
        try:
            native.attention_general(q, k, _vt(v), buf[:, :Lq], H, Lk, causal=causal)
        finally:
            lib.mi355x_attention_general_set_fast(1)
    else:
        dtype = JOINT_TYPES[tname]
        D, L0, L1, mix, spike = JOINT_SHAPES[shape]
        B, Lq, C = len(MIX), 40, H * D
        q = _rand(B, Lq, C, dtype=dtype, seed=seed)
        k0, v0 = _rand(B, L0, C, dtype=dtype, seed=seed + 1), _rand(B, L0, C, dtype=dtype, seed=seed + 2)
        k1, v1 = _rand(B, L1, C, dtype=dtype, seed=seed + 3), _rand(B, L1, C, dtype=dtype, seed=seed + 4, scale=2.0)
        if spike is not None:
            k1[:, spike] *= 6.0
        buf = torch.full((B, Lq + 1, C), NAN, dtype=dtype, device=DEV)
        m = None if mix is None else torch.tensor(mix, device=DEV, dtype=torch.float32)
        native.attention_joint(q, k0, _vt(v0), L0, k1, _vt(v1), L1, buf[:, :Lq], H, mix=m)
    torch.cuda.synchronize()
    return buf.cpu()
