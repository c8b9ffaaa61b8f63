"""mi355x_attention_streams (csrc/attn_streams.hip) against float64 torch on the GPU: out = sum_s out_scale_s softmax(scale q k_s^T) v_s.

Inputs are seeded unit normals rounded to the storage dtype before the reference is formed; the bound is the project's kernel bound, max-abs
error over max|reference| <= 1e-3 in float32 and <= 1.6e-2 with bfloat16 storage.  B = 2, H = 2; Q and K are column slices of wider buffers, V^T
rows are padded to 64 keys.  Lq = 64 / 100 / 256: less than a workgroup, no multiple of a wave's queries, several workgroups -- all of them short
grids (16-query waves); Lq = 8200 reaches the 32-query waves."""
import ctypes as C

import pytest
import torch

from refiners_amd import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, H = 2, 2
TOL = {torch.float32: 1e-3, torch.bfloat16: 1.6e-2}
DTYPES = [torch.float32, torch.bfloat16]
#: (Lq, key ranges, out_scale of stream 1): partial last tiles, a whole tile, exactly three tiles, one stream, a stream switched off
SHAPES = [(64, (77, 4), 0.7), (100, (77, 16), 0.7), (256, (64, 16), 0.7), (100, (128, 64), 0.7), (256, (77,), 0.7), (64, (77, 16), 0.0)]


def _inputs(D, Lq, lks, dtype, seed=0, pad=None, k_gain=(1.0, 1.0)):
    """q [B, Lq, C] and per stream (k [B, Lkp, C], vt [C, B, Lkp], Lk) as views the kernel takes; `pad`: what rows / columns at keys >= Lk hold."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    C_ = H * D
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).to(dtype)  # noqa: E731
    q = rnd(B, Lq, C_ + 16)[:, :, 8 : 8 + C_]
    kv = []
    for Lk, gain in zip(lks, k_gain):
        lkp = (Lk + 63) // 64 * 64
        k, vt = (rnd(B, lkp, C_ + 16) * gain)[:, :, 8 : 8 + C_], rnd(C_, B, lkp)
        if pad is not None:
            k[:, Lk:], vt[:, :, Lk:] = pad, pad
        kv.append((k, vt, Lk))
    return q, kv


def _reference(q, kv, scales):
    qh = q.double().reshape(B, -1, H, q.shape[2] // H).transpose(1, 2)
    out = 0.0
    for (k, vt, Lk), osc in zip(kv, scales):
        kh = k[:, :Lk].double().reshape(B, Lk, H, -1).transpose(1, 2)
        vh = vt[:, :, :Lk].double().permute(1, 2, 0).reshape(B, Lk, H, -1).transpose(1, 2)
        p = torch.softmax(qh @ kh.transpose(2, 3) * qh.shape[-1] ** -0.5, -1)
        out = out + osc * (p @ vh).transpose(1, 2).reshape(B, -1, q.shape[2])
    return out


def _launch(q, kv, scales):
    out = torch.full((B, q.shape[1], q.shape[2] + 4), float("nan"), device=DEV, dtype=q.dtype)[:, :, : q.shape[2]]
    native.attention_streams(q, out, H, [(k, vt, Lk, osc) for (k, vt, Lk), osc in zip(kv, scales)])
    return out


def _err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("D, Lq, lks, osc1", [(D,) + s for D in (40, 80, 160) for s in SHAPES] + [(D, 8200, (77, 4), 0.7) for D in (40, 160)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_streams_match_float64(gpu_device, D, Lq, lks, osc1, dtype):
    q, kv = _inputs(D, Lq, lks, dtype, seed=D + Lq)
    scales = (1.0, osc1)[: len(lks)]
    got = _launch(q, kv, scales)
    err = _err(got, _reference(q, kv, scales))
    print(f"D {D} Lq {Lq} keys {lks} out_scale_1 {osc1} {dtype}: {err:.2e}")
    assert err <= TOL[dtype]
    assert torch.equal(got, _launch(q, kv, scales)), "a repeat launch differs"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [40, 160])
def test_each_stream_has_its_own_softmax(gpu_device, D, dtype):
    """Stream 0's keys are 24 times larger: its score maximum lies about 60 above stream 1's, which a maximum shared by both would flush to zero."""
    q, kv = _inputs(D, 100, (77, 16), dtype, seed=5, k_gain=(24.0, 1.0))
    ref = _reference(q, kv, (1.0, 0.7))
    assert _err(_launch(q, kv, (1.0, 0.7)), ref) <= TOL[dtype]
    assert _err(_reference(q, kv[:1], (1.0,)), ref) > 10 * TOL[dtype], "stream 1 carries no weight in this case"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("lks", [(77, 4), (100, 33)])
def test_padding_keys_do_not_show(gpu_device, lks, dtype):
    q, kv = _inputs(80, 100, lks, dtype, seed=6, pad=1e4)
    assert _err(_launch(q, kv, (1.0, 0.7)), _reference(q, kv, (1.0, 0.7))) <= TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_a_stream_scaled_by_zero_contributes_an_exact_zero(gpu_device, dtype):
    q, kv = _inputs(80, 100, (77, 16), dtype, seed=7)
    kv[1][0].fill_(3e38)  # its scores would overflow
    got, one = _launch(q, kv, (1.0, 0.0)), _launch(q, kv[:1], (1.0,))
    assert torch.isfinite(got).all() and _err(got, one.double()) <= TOL[dtype] and _err(got, _reference(q, kv[:1], (1.0,))) <= TOL[dtype]


@pytest.mark.parametrize("what", ["four key tiles", "D = 168", "nstream = 3"])
def test_refusals_launch_nothing(gpu_device, what):
    D = 168 if what == "D = 168" else 40
    q, kv = _inputs(D, 64, (128, 128) if what == "four key tiles" else (77, 4), torch.float32)
    out = torch.full((B, 64, H * D), float("nan"), device=DEV)
    a, _keep = native.attention_args(q, out, H, [(k, vt, Lk, 1.0) for k, vt, Lk in kv])
    if what == "nstream = 3":
        a.nstream = 3
    with pytest.raises(native.NativeError, match="ESHAPE"):
        native.check(native.load().mi355x_attention_streams(C.byref(a), native.stream_ptr()), "mi355x_attention_streams")
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
