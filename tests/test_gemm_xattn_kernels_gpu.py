"""mi355x_gemm_attention (a cross-attention folded into its Q projection) against the two launches it replaces and against float32 torch.

Every case runs, on the same seeded inputs, the fused launch, mi355x_gemm (64 x 64 tile) followed by mi355x_attention, and a float32 reference
that rounds Q to bfloat16 where the stored tensor would be, in all four forms of the Q projection: bias or folded LayerNorm, with or without
the in-launch LoRA (2 x rank 16).  Shapes are the smallest at which the kernel can go wrong: two batch elements with their own K / V, 2 and 3
heads (head <-> column tile, an odd tile grid for the rasteriser), one and two row tiles per batch element, K of one block, of the two-stage
ring's wrap and long enough for the peeled LoRA look (4 trips and more), every slot layout of the key tiles.

Expectation: the fused output is BIT-EQUAL to the two launches' (same arithmetic, same rounding points; the 16-query form of the short kernel on
both sides).  Should the compiler pair an addition differently in the two kernels, no element may differ by more than one bfloat16 unit in the
last place at its own magnitude, and the fused path's relative l2 error against float32 must not exceed the two-launch path's.
"""
from __future__ import annotations

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from refiners_amd import native  # noqa: E402
from tests import kernel_cases as KC  # noqa: E402

DT = torch.bfloat16
KEYS = [(1, 0), (32, 0), (33, 0), (64, 0), (65, 0), (77, 0), (77, 4), (64, 16), (33, 33)]  # (text keys, second-stream keys)
SHAPES = [(H, Lq, K) for H in (2, 3) for Lq in (64, 128) for K in (64, 128, 320)]
FORMS = [(ln, lora) for ln in (False, True) for lora in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from refiners_amd.build_native import build_native

    build_native()
    native.load()


def _inputs(B, H, Lq, K, Lk, Lk2, seed, spike=False):
    C, M = 64 * H, B * Lq
    d = dict(B=B, H=H, Lq=Lq, K=K, C=C, M=M)
    d["x"] = KC._rand(M, K, dtype=DT, seed=seed) + 1.5  # a non-zero row mean: the mean * s cancellation of the folded LayerNorm
    d["w"] = KC._rand(C, K, dtype=DT, seed=seed + 1, scale=K ** -0.5)
    d["b"] = KC._rand(C, dtype=DT, seed=seed + 2)
    d["gamma"] = (1 + 0.2 * KC._rand(K, dtype=torch.float32, seed=seed + 3)).float()
    d["beta"] = (0.3 * KC._rand(K, dtype=torch.float32, seed=seed + 4)).float()
    d["lora"] = KC._lora_pack(K, C, DT, (16, 16), seed + 5)
    streams, plain = [], []
    for i, (n, osc) in enumerate(((Lk, 1.0), (Lk2, 0.6))):
        if n:
            k = KC._rand(B, n, C, dtype=DT, seed=seed + 20 + 2 * i)
            v = KC._rand(B, n, C, dtype=DT, seed=seed + 21 + 2 * i)
            if spike:  # large running-maximum jumps late in the key sequence
                k[:, n - 3 if n >= 3 else 0] *= 6.0
                k[:, n // 2] *= 4.0
            streams.append((k, KC._vt_from_v(v, (n + 63) // 64 * 64), n, osc))
            plain.append((k, v, osc))
    d["streams"], d["plain"] = streams, plain
    return d


def _q_kwargs(d, ln, lora):
    """(x operand pair, keyword arguments of native.gemm, float32 Q) of one form of the Q projection."""
    x, w, K = d["x"], d["w"], d["K"]
    a_kb, bs, delta = d["lora"]
    eps = 1e-5
    kw = {}
    if ln:
        h = torch.nn.functional.layer_norm(x.float(), (K,), d["gamma"], d["beta"], eps)
        wl = (w.float() * d["gamma"].unsqueeze(0)).to(DT).contiguous()
        ls, lc = wl.float().sum(1).contiguous(), (w.float() @ d["beta"] + d["b"].float()).contiguous()
        kw["ln"] = (KC._stats_ref(x.float()).to(KC.DEV), ls, lc, eps)
        wop = wl
        if lora:
            a = a_kb.dense().float()
            al = (a * d["gamma"].unsqueeze(0)).to(DT).contiguous()
            kw["lora"] = ([(0, native.KBlocked(al))], bs, al.float().sum(1).contiguous(), (a @ d["beta"]).contiguous())
    else:
        h = x.float()
        kw["bias"] = d["b"]
        wop = w
        if lora:
            kw["lora"] = ([(0, a_kb)], bs)
    q32 = h @ (w.float() + (delta if lora else 0)).t() + d["b"].float()
    return (x, native.KBlocked(wop)), kw, q32


def _ulp(v: torch.Tensor) -> torch.Tensor:
    """One bfloat16 unit in the last place at |v|'s magnitude (8 significand bits)."""
    return torch.where(v > 0, torch.exp2(torch.floor(torch.log2(v.clamp_min(1e-38))) - 7), torch.zeros_like(v))


def _run(d, ln, lora):
    """(fused output, two-launch output, float32 reference) of one form."""
    B, H, Lq, C, M = d["B"], d["H"], d["Lq"], d["C"], d["M"]
    seg, kw, q32 = _q_kwargs(d, ln, lora)
    fused = torch.full((B, Lq, C), float("nan"), dtype=DT, device=KC.DEV)
    native.gemm([seg], None, M=M, N=C, tile=4, attn=native.attention_args(None, fused, H, d["streams"]), **kw)
    q = torch.full((M, C), float("nan"), dtype=DT, device=KC.DEV)
    native.gemm([seg], q, tile=4, **kw)
    two = torch.full((B, Lq, C), float("nan"), dtype=DT, device=KC.DEV)
    native.attention(q.view(B, Lq, C), two, H, d["streams"])
    qr = q32.to(DT).view(B, Lq, C)  # Q as the stored tensor holds it
    ref = sum(osc * KC._sdpa_ref(qr, k, v, H) for k, v, osc in d["plain"])
    return fused, two, ref


def _check(tag, fused, two, ref):
    assert torch.isfinite(fused.float()).all() and torch.isfinite(two.float()).all(), tag
    f, t = fused.float(), two.float()
    rel = lambda o: ((o - ref).norm() / ref.norm()).item()  # noqa: E731
    ef, et = rel(f), rel(t)
    differ = (f != t)
    share = differ.float().mean().item()
    print(f"{tag}: rel l2 fused {ef:.3e} two-launch {et:.3e}, differing elements {share:.2%}")
    assert et < 1.6e-2, (tag, et)  # the two-launch path itself is sane (bfloat16 output rounding)
    if share:
        bound = _ulp(torch.maximum(f.abs(), t.abs()))
        assert ((f - t).abs() <= bound).all(), (tag, "more than one bfloat16 unit in the last place", share)
    assert ef <= et, (tag, ef, et)
    return share


@pytest.mark.parametrize("Lk,Lk2", KEYS, ids=[f"{a}+{b}" if b else str(a) for a, b in KEYS])
@pytest.mark.parametrize("H,Lq,K", SHAPES, ids=[f"H{h}_Lq{lq}_K{k}" for h, lq, k in SHAPES])
def test_fused_matches_two_launches(H, Lq, K, Lk, Lk2):
    d = _inputs(2, H, Lq, K, Lk, Lk2, seed=400 + 7 * H + Lq + K + 3 * Lk + Lk2)
    for ln, lora in FORMS:
        fused, two, ref = _run(d, ln, lora)
        _check(f"H{H} Lq{Lq} K{K} keys {Lk}+{Lk2} ln{int(ln)} lora{int(lora)}", fused, two, ref)


def test_fused_spiked_scores():
    """As attn_*_short_1plus1_spike: scores that move the running maximum late in the key sequence, a one-key second stream."""
    d = _inputs(2, 3, 128, 320, 17, 1, seed=480, spike=True)
    for ln, lora in FORMS:
        fused, two, ref = _run(d, ln, lora)
        _check(f"spike ln{int(ln)} lora{int(lora)}", fused, two, ref)


def test_step_shape_class():
    """The benchmarked step's class (2 x 1024 tokens, 20 heads, K = 1280, 77 + 4 keys) at a fifth of its rows: every XCD gets tiles, the weight
    prefetch workgroups and the LoRA producers sit in front of them."""
    d = _inputs(2, 20, 192, 1280, 77, 4, seed=490)
    pf = KC._rand(1 << 19, dtype=DT, seed=491)
    seg, kw, _q32 = _q_kwargs(d, True, True)
    fused, two, ref = _run(d, True, True)
    _check("step class", fused, two, ref)
    again = torch.full_like(fused, float("nan"))
    native.gemm([seg], None, M=d["M"], N=d["C"], tile=4, prefetch=pf, attn=native.attention_args(None, again, d["H"], d["streams"]), **kw)
    assert torch.equal(again, fused)  # prefetch workgroups change nothing; the launch is reproducible


def test_refused_on_device():
    """A refused call launches nothing (the output keeps its fill)."""
    d = _inputs(2, 2, 64, 64, 77, 0, seed=495)
    seg, kw, _ = _q_kwargs(d, False, False)
    out = torch.full((2, 64, 128), 7.0, dtype=DT, device=KC.DEV)
    with pytest.raises(native.NativeError, match="ESHAPE"):
        native.gemm([seg], None, M=128, N=128, tile=4, attn=native.attention_args(None, out[:, :, :64], 1, [(s[0][:, :, :64], s[1][:64], s[2], s[3]) for s in d["streams"]]), **kw)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and math.isfinite(out.float().sum().item())
