"""Kernel-level parity cases for the glue kernels (csrc/elementwise.hip) and the norm edges (csrc/norm.hip) that kernel_cases.py does not reach.

Conventions as in kernel_cases.py: seeded inputs rounded to the compute dtype, outputs pre-filled with NaN (arithmetic) or a sentinel (data
movement, row gaps, the element behind the output), and a case returns (max_abs_err, ref_scale, tol_rel) -- the caller asserts
err <= tol_rel * ref_scale.  Here every reference is computed in FLOAT64 ON THE CPU from the same rounded inputs (the nearest-neighbour mask
of Self-Attention Guidance must be torch's own CPU interpolate, and float64 convolutions need no GPU library).  Pure data movement returns
(number of differing bit patterns, 1, 0): bit-equal or failed.  Used by tests/test_glue_kernels_gpu.py; the references that need no GPU
(relpos_gather_ref, sag_reference, nearest_cells_f32) are checked on their own by tests/test_glue_refs_cpu.py.

Shapes are the smallest at which each path can go wrong; the `wrap` cases hold just over 2^20 work items, so the grid-stride loops
(grid_for caps a launch at 4096 x 256 work items) take their second trip.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from refiners_amd import native
from tests import kernel_cases as KC

DEV = KC.DEV
SENT = 7.0  # exactly representable in both dtypes
WRAP = 1 << 20  # work items of one full grid


def _fill(*shape, dtype, value=float("nan")):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _bit_diff(out: torch.Tensor, ref: torch.Tensor) -> int:
    assert out.shape == ref.shape and out.dtype == ref.dtype
    return int((_bits(out.cpu()) != _bits(ref.cpu())).sum())


def _cmp64(out: torch.Tensor, ref: torch.Tensor, dtype) -> tuple[float, float, float]:
    o = out.detach().cpu().double()
    assert torch.isfinite(o).all(), "non-finite (unwritten?) values in kernel output"
    return (o - ref).abs().max().item(), max(ref.abs().max().item(), 1e-6), KC._tol(dtype)


def _worst(results) -> tuple[float, float, float]:
    """The result with the largest err / (tol * scale) of several sub-runs of one case (exact sub-runs: any difference wins)."""
    return max(results, key=lambda r: r[0] / (r[2] * r[1]) if r[2] else (math.inf if r[0] else -1.0))


def _refused(code: str, fn, out: torch.Tensor) -> tuple[float, float, float]:
    """A call rejected on the host raises MI355X_<code> and launches nothing: `out` (sentinel-filled) is untouched."""
    try:
        fn()
    except native.NativeError as e:
        assert code in str(e), f"refused with {e}, expected {code}"
    else:
        raise AssertionError(f"the call was accepted, expected {code}")
    torch.cuda.synchronize()
    return float((out.float() != SENT).sum()), 1.0, 0.0


# ------------------------------------------------------------------------------------------------ relpos_pack
def relpos_gather_ref(src: torch.Tensor, H: int, d: int, S1: int, S2: int, Lp: int, Dq: int) -> torch.Tensor:
    """The comment above relpos_pack_kernel as a plain gather.  src [M, >= H*Lp] (cpu); row t % (S1*S2) sits at grid position
    (a, b) = (t / S2, t % S2); per head  out = [ src[0:d] | P1[S1-1-a + a'], a' < S1 | P2[S2-1-b + b'], b' < S2 | 0 ]  with P1 at column d
    and P2 at column d + 2*S1 - 1 of the head's Lp source columns."""
    M = src.shape[0]
    out = torch.zeros(M, H * Dq, dtype=src.dtype)
    for row in range(M):
        t = row % (S1 * S2)
        a, b = t // S2, t % S2
        for hd in range(H):
            s, o = src[row, hd * Lp : (hd + 1) * Lp], out[row, hd * Dq : (hd + 1) * Dq]
            o[:d] = s[:d]
            for a2 in range(S1):
                o[d + a2] = s[d + (S1 - 1 - a) + a2]
            for b2 in range(S2):
                o[d + S1 + b2] = s[d + (2 * S1 - 1) + (S2 - 1 - b) + b2]
    return out


def relpos_pack_case(dtype, d, Lp, Dq, *, lds_pad=0, ldo_pad=0, offset=0, S1=3, S2=5, H=2, samples=2, seed=600):
    """Bit-equal to the gather; the zero pad [d+S1+S2, Dq) is part of the reference, the bytes between H*Dq and ldo keep the sentinel."""
    M = samples * S1 * S2
    lds, ldo = H * Lp + lds_pad, H * Dq + ldo_pad
    buf = KC._rand(M * lds + 8, dtype=dtype, seed=seed)
    src = buf[offset : offset + M * lds].view(M, lds)
    out = _fill(M, ldo, dtype=dtype, value=SENT)
    native.relpos_pack(src, out, H, d, S1, S2, Lp, Dq)
    torch.cuda.synchronize()
    want = torch.full((M, ldo), SENT, dtype=dtype)
    want[:, : H * Dq] = relpos_gather_ref(src.cpu(), H, d, S1, S2, Lp, Dq)
    return float(_bit_diff(out, want)), 1.0, 0.0


def relpos_chain_case(dtype, B=2, H=2, S1=3, S2=5, d=16, seed=620):
    """mi355x_relpos_pack -> mi355x_attention_general against torch softmax with the decomposed bias computed DIRECTLY:
    bias[t, t'] = q . E1[a - a' + S1 - 1] + q . E2[b - b' + S2 - 1].  The source rows hold what the folded projection GEMM would have stored:
    q * scale and the products with the reversed tables, each rounded to the compute dtype -- the reference rounds the same quantities."""
    L, Lp, Dq, scale = S1 * S2, 32, 32, d ** -0.5
    cpu = lambda *s, seed, sc=1.0: KC._rand(*s, dtype=dtype, seed=seed, scale=sc).cpu().double()  # noqa: E731
    q, k, v = cpu(B, L, H, d, seed=seed), cpu(B, L, H, d, seed=seed + 1), cpu(B, L, H, d, seed=seed + 2)
    E1, E2 = cpu(2 * S1 - 1, d, seed=seed + 3, sc=0.5), cpu(2 * S2 - 1, d, seed=seed + 4, sc=0.5)
    rnd = lambda t: t.to(dtype).double()  # noqa: E731
    src = KC._rand(B, L, H, Lp, dtype=dtype, seed=seed + 5).cpu()  # (columns behind the products: never read)
    src[..., :d] = (q * scale).to(dtype)
    src[..., d : d + 2 * S1 - 1] = (q @ E1.flip(0).t()).to(dtype)  # P1[r] = q . E1[2*S1 - 2 - r]
    src[..., d + 2 * S1 - 1 : d + 2 * S1 - 1 + 2 * S2 - 1] = (q @ E2.flip(0).t()).to(dtype)
    qa = _fill(B * L, H * Dq, dtype=dtype)
    native.relpos_pack(src.reshape(B * L, H * Lp).to(DEV), qa, H, d, S1, S2, Lp, Dq)
    ka = torch.zeros(B, L, H, Dq, dtype=dtype, device=DEV)  # K' = [ k | onehot(a') | onehot(b') | 0 ], as attention_relpos_case builds it
    ka[..., :d] = k.to(dtype).to(DEV)
    idx = torch.arange(L, device=DEV)
    ka[:, idx, :, d + idx // S2] = 1
    ka[:, idx, :, d + S1 + idx % S2] = 1
    out = _fill(B, L, H * d, dtype=dtype)
    native.attention_general(qa.view(B, L, H * Dq), ka.reshape(B, L, H * Dq), KC._vt_from_v(v.to(dtype).to(DEV).reshape(B, L, H * d), 64), out, H, L, scale=1.0)
    t = torch.arange(L)
    a, b = t // S2, t % S2
    i1, i2 = a[:, None] - a[None, :] + S1 - 1, b[:, None] - b[None, :] + S2 - 1  # [t, t']
    bias = rnd(torch.einsum("bthd,tsd->bhts", q, E1[i1])) + rnd(torch.einsum("bthd,tsd->bhts", q, E2[i2]))
    logits = torch.einsum("bthd,bshd->bhts", rnd(q * scale), k) + bias
    ref = torch.einsum("bhts,bshd->bthd", torch.softmax(logits, dim=-1), v).reshape(B, L, H * d)
    return _cmp64(out, ref, dtype)


# ------------------------------------------------------------------------------------------------ pointwise_nchw
def pointwise_case(dtype, Ci, Co, B, HW, bias, seed=640):
    x = KC._rand(B, Ci, HW, 1, dtype=dtype, seed=seed)
    w = KC._rand(Co, Ci, dtype=dtype, seed=seed + 1, scale=0.7)
    b = KC._rand(Co, dtype=dtype, seed=seed + 2) if bias else None
    out = _fill(B, Co, HW, 1, dtype=dtype)
    native.pointwise_nchw(x, w, b, out)
    ref = F.conv2d(x.cpu().double(), w.cpu().double().view(Co, Ci, 1, 1), b.cpu().double() if bias else None)
    return _cmp64(out, ref, dtype)


def pointwise_refused_case(dtype):
    x, w = KC._rand(2, 9, 16, 1, dtype=dtype, seed=650), KC._rand(4, 9, dtype=dtype, seed=651)
    out = _fill(2, 4, 16, 1, dtype=dtype, value=SENT)
    return _refused("EARG", lambda: native.pointwise_nchw(x, w, None, out), out)


# ------------------------------------------------------------------------------------------------ colsum_rows
def colsum_case(dtype, M, L, seed=660):
    """accumulate = 0 over a NaN-filled acc, then accumulate = 1 with other rows on the same acc; acc is longer than L (sentinel behind),
    ldp > L.  Against the float64 sum of the STORED values with the derivable bound: a launch adds at most M values per column in float32
    (ceil(M / 4) per row lane, three LDS adds, one multiply), so its error is below M * 2^-23 * sum_i |p[i][j]| * scale; the second launch's
    acc + t rounds once more, 2^-24 of the total.  Returns the worst err / bound as (ratio, 1, 1).  A repeated run is bit-equal."""
    scale = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))
    ps = [KC._rand(M, L + 8, dtype=dtype, seed=seed + i)[:, :L] for i in range(2)]
    accs = []
    for _ in range(2):
        acc = _fill(L + 5, dtype=torch.float32)
        acc[L:] = SENT
        native.colsum_rows(ps[0], acc, False, scale)
        first = acc.clone()
        native.colsum_rows(ps[1], acc, True, scale)
        accs.append((first, acc))
    torch.cuda.synchronize()
    assert all(torch.equal(accs[0][i], accs[1][i]) for i in range(2)), "colsum_rows must be bit-reproducible"
    first, acc = (t.cpu().double() for t in accs[0])
    assert (acc[L:] == SENT).all() and (first[L:] == SENT).all(), "wrote behind column L"
    assert torch.isfinite(acc).all() and torch.isfinite(first).all()
    s = [p.cpu().double().sum(0) * scale for p in ps]
    bd = [M * 2.0 ** -23 * p.cpu().double().abs().sum(0) * scale for p in ps]
    r1 = ((first[:L] - s[0]).abs() / bd[0]).max().item()
    r2 = ((acc[:L] - (s[0] + s[1])).abs() / (bd[0] + bd[1] + 2.0 ** -24 * (s[0] + s[1]).abs())).max().item()
    return max(r1, r2), 1.0, 1.0


def colsum_chain_case(dtype, heads=2, L=96, d=64, seed=670):
    """scores GEMM -> softmax_rows -> colsum_rows per head (LoweredBlocks.sag_attention_mass) against attn.mean(heads).sum(queries) in float64:
    the quantity compute_sag_mask thresholds at 1."""
    q, k = KC._rand(L, heads * d, dtype=dtype, seed=seed), KC._rand(L, heads * d, dtype=dtype, seed=seed + 1)
    mass, sc, pr = _fill(L, dtype=torch.float32), _fill(L, L, dtype=torch.float32), _fill(L, L, dtype=dtype)
    for h in range(heads):
        native.gemm([(q[:, h * d : (h + 1) * d], k[:, h * d : (h + 1) * d])], sc, out_f32=dtype != torch.float32)
        native.softmax_rows(sc, pr, L, d ** -0.5)
        native.colsum_rows(pr, mass, accumulate=h > 0, scale=1.0 / heads)
    qh, kh = (t.cpu().double().view(L, heads, d).transpose(0, 1) for t in (q, k))
    attn = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(d), dim=-1)  # [heads, queries, keys]
    return _cmp64(mass, attn.mean(0).sum(0), dtype)


# ------------------------------------------------------------------------------------------------ sag_degrade
def nearest_cells_f32(n_out: int, n_in: int) -> np.ndarray:
    """The source index torch's interpolate(mode="nearest") takes for every destination index, emulated in float32 as sag_degrade_kernel
    computes it: min(floor(dst * (float(n_in) / float(n_out))), n_in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def gaussian_w1(ks: int, sigma: float = 1.0) -> torch.Tensor:
    t = torch.linspace(-(ks - 1) * 0.5, (ks - 1) * 0.5, steps=ks, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    return pdf / pdf.sum()


def sag_reference(x, eps, mass, ah, aw, a, sd, w1) -> torch.Tensor:
    """compute_degraded_latents in float64 on the CPU.  x, eps [n, C, h, w] and w1 [ks] float64, mass float32 [n, ah*aw], a / sd = the
    step's cumulative scale factor / noise std.  remove_noise; reflect pad, then the separable ks-tap blur as two conv2d; the mask is
    F.interpolate(mass > 1, size=(h, w), mode="nearest") by torch itself; blend; add_noise."""
    n, C, h, w = x.shape
    ks = w1.numel()
    x0 = (x - sd * eps) / a
    p = ks // 2
    pad = F.pad(x0, (p, p, p, p), mode="reflect")
    blur = F.conv2d(pad, w1.view(1, 1, ks, 1).expand(C, 1, ks, 1), groups=C)
    blur = F.conv2d(blur, w1.view(1, 1, 1, ks).expand(C, 1, 1, ks), groups=C)
    m = F.interpolate((mass.view(n, 1, ah, aw) > 1.0).float(), size=(h, w), mode="nearest").double()
    return a * (blur * m + x0 * (1 - m)) + sd * eps


def checker_mass(n, ah, aw):
    """Alternates 1.5 / 0.5 per cell (and per sample): reading a neighbour's cell flips blurred <-> untouched."""
    i = torch.arange(ah)[:, None] + torch.arange(aw)[None, :]
    return torch.stack([torch.where((i + s) % 2 == 0, 1.5, 0.5) for s in range(n)]).reshape(n, ah * aw).float()


def sag_case(dtype, n, C, h, w, ah, aw, mass, ks=9, seed=700):
    x, eps = KC._rand(n, C, h, w, dtype=dtype, seed=seed), KC._rand(n, C, h, w, dtype=dtype, seed=seed + 1)
    coef = torch.tensor([7.5, 0.83, 0.55], dtype=torch.float32)
    w1 = gaussian_w1(ks)
    mass = mass.float().reshape(n, ah * aw).contiguous()
    out = _fill(n, C, h, w, dtype=dtype)
    native.sag_degrade(x, eps, mass.to(DEV), (ah, aw), coef.to(DEV), w1.to(DEV), out)
    ref = sag_reference(x.cpu().double(), eps.cpu().double(), mass, ah, aw, float(coef[1]), float(coef[2]), w1.double())
    return _cmp64(out, ref, dtype)


def sag_refused_case(dtype, h, w, ks):
    x = KC._rand(1, 2, h, w, dtype=dtype, seed=730)
    out = _fill(1, 2, h, w, dtype=dtype, value=SENT)
    coef, w1, mass = torch.ones(3, device=DEV), torch.full((ks,), 1.0 / ks, device=DEV), torch.full((1, 1), 1.5, device=DEV)
    return _refused("EARG", lambda: native.sag_degrade(x, x, mass, (1, 1), coef, w1, out), out)


# ------------------------------------------------------------------------------------------------ silu, axpby, concat2, cfg_ddim_step
def silu_case(dtype, n, seed=740):
    """Out of place with the sentinel behind element n, then in place (out is x, as unet_lowering calls it): bit-equal to the first."""
    x = KC._rand(n, dtype=dtype, seed=seed, scale=3.0)
    x[: min(n, 3)] = torch.tensor([20.0, -20.0, 0.0], dtype=dtype, device=DEV)[: min(n, 3)]
    buf = _fill(n + 8, dtype=dtype)
    buf[n:] = SENT
    native.silu(x, buf[:n])
    xd = x.cpu().double()
    native.silu(x, x)
    torch.cuda.synchronize()
    assert (buf[n:].float() == SENT).all(), "wrote behind element n"
    assert _bit_diff(x, buf[:n]) == 0, "in place differs from out of place"
    return _cmp64(x, xd / (1 + torch.exp(-xd)), dtype)


def axpby_case(dtype, n, seed=760):
    """out = alpha a + beta b: the 16-byte body and the scalar tail (n % EPC elements, block 0), the sentinel behind element n; `out is b`
    (CompiledSDXL._prepare_sag) and `out is a` bit-equal to the launch without aliasing."""
    al, be = 0.55, -1.25
    a, b = KC._rand(n, dtype=dtype, seed=seed), KC._rand(n, dtype=dtype, seed=seed + 1)
    buf = _fill(n + 8, dtype=dtype)
    buf[n:] = SENT
    native.axpby(a, al, b, be, buf[:n])
    a2, b2 = a.clone(), b.clone()
    native.axpby(a, al, b2, be, b2)
    native.axpby(a2, al, b, be, a2)
    torch.cuda.synchronize()
    assert (buf[n:].float() == SENT).all(), "wrote behind element n"
    assert _bit_diff(b2, buf[:n]) == 0, "out is b differs"
    assert _bit_diff(a2, buf[:n]) == 0, "out is a differs"
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    return _cmp64(buf[:n], f32(al) * a.cpu().double() + f32(be) * b.cpu().double(), dtype)


def concat2_case(dtype, M, C1, C2, seed=780):
    """lda, ldb, ldo larger than the widths; bit-equal, and the gap of every output row keeps the sentinel."""
    epc = 16 // (4 if dtype == torch.float32 else 2)
    a = KC._rand(M, C1 + epc, dtype=dtype, seed=seed)[:, :C1]
    b = KC._rand(M, C2 + 2 * epc, dtype=dtype, seed=seed + 1)[:, :C2]
    out = _fill(M, C1 + C2 + epc, dtype=dtype, value=SENT)
    native.concat2(a, b, out[:, : C1 + C2])
    want = torch.full(out.shape, SENT, dtype=dtype)
    want[:, :C1], want[:, C1 : C1 + C2] = a.cpu(), b.cpu()
    return float(_bit_diff(out, want)), 1.0, 0.0


def cfg_ddim_case(dtype, n, seed=800):
    x, uo = KC._rand(n, dtype=dtype, seed=seed), KC._rand(2 * n, dtype=dtype, seed=seed + 1)
    coef = torch.tensor([5.0, 0.8, 0.6, 0.9, math.sqrt(1 - 0.81)], dtype=torch.float32)
    cfg, sa, s1a, sap, s1ap = (float(c) for c in coef)
    xd, u, c = x.cpu().double(), uo[:n].cpu().double(), uo[n:].cpu().double()
    e = u + cfg * (c - u)
    ref = sap * ((xd - s1a * e) / sa) + s1ap * e
    native.cfg_ddim_step(x, uo, coef.to(DEV))
    return _cmp64(x, ref, dtype)


# ------------------------------------------------------------------------------------------------ LayerNorm / GroupNorm edges
def _epc(dtype) -> int:
    return 4 if dtype == torch.float32 else 8


def layernorm_edge_case(dtype, nvec, *, narrow=False, seed=820):
    """One width per end of every MAXV instance's range (nvec = 16-byte vectors per row).  M = 1 and 5 (the last workgroup's waves past M return
    early), ldx and ldo larger than C; the row gaps and a whole row behind the output keep the sentinel.  narrow: rows of mean 100 and
    deviation 0.1 (float32: the two-pass variance must not cancel; bfloat16 stores such a row as the constant 100: variance 0, out = beta)."""
    C, e = nvec * _epc(dtype), _epc(dtype)
    res = []
    for M in (1, 5):
        x = KC._rand(M, C + 2 * e, dtype=dtype, seed=seed + M, scale=2.0) + 0.5
        if narrow:
            x = (100.0 + 0.1 * KC._rand(M, C + 2 * e, dtype=torch.float32, seed=seed + M)).to(dtype)
        g = (1 + 0.1 * KC._rand(C, dtype=torch.float32, seed=seed + 10)).to(dtype)
        b = (0.1 * KC._rand(C, dtype=torch.float32, seed=seed + 11)).to(dtype)
        out = _fill(M + 1, C + e, dtype=dtype, value=SENT)
        native.layernorm(x[:, :C], g, b, 1e-5, out[:M, :C])
        torch.cuda.synchronize()
        assert (out[M].float() == SENT).all() and (out[:, C:].float() == SENT).all(), "wrote outside the M x C output"
        ref = F.layer_norm(x[:, :C].cpu().double(), (C,), g.cpu().double(), b.cpu().double(), 1e-5)
        res.append(_cmp64(out[:M, :C], ref, dtype))
    return _worst(res)


def layernorm_refused_case(dtype):
    C = 1025 * _epc(dtype)  # one vector more than the widest instance holds: 8200 in bfloat16
    x, g = KC._rand(2, C, dtype=dtype, seed=840), KC._rand(C, dtype=dtype, seed=841)
    out = _fill(2, C, dtype=dtype, value=SENT)
    return _refused("ESHAPE", lambda: native.layernorm(x, g, g, 1e-5, out), out)


def groupnorm_edge_case(dtype, C, G, HWs=(1, 3, 5), B=3, *, constant=False, seed=860):
    """mi355x_groupnorm (statistics pass, finalize, apply) with and without SiLU, ldx and ldo larger than C (the gaps keep the sentinel).
    constant: every input is 1.5 (sums of it are exact in float32): variance 0, so the output is beta, or silu(beta)."""
    e = _epc(dtype)
    res = []
    for HW in HWs:
        for silu in (False, True):
            x = KC._rand(B, HW, C + e, dtype=dtype, seed=seed + HW, scale=1.5) + 3.0
            if constant:
                x = torch.full_like(x, 1.5)
            g = (1 + 0.1 * KC._rand(C, dtype=torch.float32, seed=seed + 10)).to(dtype)
            b = KC._rand(C, dtype=dtype, seed=seed + 11)
            out = _fill(B, HW, C + 2 * e, dtype=dtype, value=SENT)
            native.groupnorm_nhwc(x[:, :, :C], g, b, G, 1e-5, silu, out[:, :, :C])
            torch.cuda.synchronize()
            assert (out[:, :, C:].float() == SENT).all(), "wrote into the row gap"
            if constant:
                ref = b.cpu().double().view(1, C, 1).expand(B, C, HW)
            else:
                ref = F.group_norm(x[:, :, :C].cpu().double().permute(0, 2, 1), G, g.cpu().double(), b.cpu().double(), 1e-5)
            if silu:
                ref = ref / (1 + torch.exp(-ref))
            res.append(_cmp64(out[:, :, :C].permute(0, 2, 1), ref, dtype))
    return _worst(res)


def groupnorm_refused_case(dtype, C, G):
    x, g = KC._rand(1, 8, C, dtype=dtype, seed=880), KC._rand(C, dtype=dtype, seed=881)
    out = _fill(1, 8, C, dtype=dtype, value=SENT)
    return _refused("ESHAPE", lambda: native.groupnorm_nhwc(x, g, g, G, 1e-5, False, out), out)


# ------------------------------------------------------------------------------------------------ the list
SAG_NEAREST = [(122, 16), (198, 50)]  # (latent size, attention size) at which py * ah / h in integers and torch's float32 rule differ (rows 61 / 99)


def all_cases():
    """(name, thunk) list; every case runs in float32 and bfloat16."""
    cases = []
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        epc = _epc(dt)
        # relpos_pack: S1 x S2 = 3 x 5 (swapping a and b is caught), 2 heads, two samples (row % L).  Vector path first, then the scalar fallback
        # entered by each of its conditions alone: d not a whole number of vectors (12: bfloat16, 14: both), Lp odd (lds stays a multiple of 16 bytes),
        # a source view offset by one element.
        cases += [
            (f"relpos_pack_{tag}_vec", lambda dt=dt: relpos_pack_case(dt, 16, 32, 32)),
            (f"relpos_pack_{tag}_vec_Dq24", lambda dt=dt: relpos_pack_case(dt, 16, 32, 24)),
            (f"relpos_pack_{tag}_vec_wide_rows", lambda dt=dt, epc=epc: relpos_pack_case(dt, 16, 32, 32, lds_pad=2 * epc, ldo_pad=epc)),
            (f"relpos_pack_{tag}_d12", lambda dt=dt: relpos_pack_case(dt, 12, 32, 32)),  # (float32: three whole vectors, still the vector path)
            (f"relpos_pack_{tag}_scalar_d14", lambda dt=dt: relpos_pack_case(dt, 14, 32, 32)),
            (f"relpos_pack_{tag}_scalar_Lp31", lambda dt=dt: relpos_pack_case(dt, 16, 31, 32, lds_pad=2)),
            (f"relpos_pack_{tag}_scalar_offset_src", lambda dt=dt: relpos_pack_case(dt, 16, 32, 32, offset=1)),
            (f"relpos_pack_{tag}_attention_chain", lambda dt=dt: relpos_chain_case(dt)),
        ]
        for ci, co in ((4, 4), (1, 8), (8, 1), (3, 5)):
            for bias in (False, True):
                cases.append((f"pointwise_{tag}_{ci}to{co}{'_bias' if bias else ''}", lambda dt=dt, ci=ci, co=co, bias=bias: pointwise_case(dt, ci, co, 2, 333, bias)))
        cases += [
            (f"pointwise_{tag}_4to4_wrap", lambda dt=dt: pointwise_case(dt, 4, 4, 1, WRAP + 259, True)),
            (f"pointwise_{tag}_9_channels_refused", lambda dt=dt: pointwise_refused_case(dt)),
        ]
        cases += [(f"colsum_{tag}_{M}x{L}", lambda dt=dt, M=M, L=L: colsum_case(dt, M, L)) for M, L in ((1, 1), (3, 64), (7, 65), (130, 200))]
        cases.append((f"colsum_{tag}_softmax_chain", lambda dt=dt: colsum_chain_case(dt)))
        # sag_degrade.  5 x 7 is the smallest size a 9-tap blur is legal at (every pixel reflects on both sides); masses 0.5 / 1.5 / exactly 1.0
        # (not masked) / the next float32 above 1.0 (masked); two samples with different masses and 4 planes each; ks = 1; one grid wrap.
        one_up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
        m6 = torch.tensor([[0.5, 1.5, 1.0, one_up, 0.5, 1.5]])
        m9 = torch.tensor([[0.5, 1.5, 1.0, 1.5, 0.5, 1.0, one_up, 1.5, 0.5], [1.5, 0.5, 1.5, 1.0, 1.5, 0.5, 1.0, 0.5, 1.5]])
        cases += [
            (f"sag_{tag}_5x7_ks9", lambda dt=dt, m6=m6: sag_case(dt, 1, 3, 5, 7, 2, 3, m6)),
            (f"sag_{tag}_12x9_two_samples", lambda dt=dt, m9=m9: sag_case(dt, 2, 4, 12, 9, 3, 3, m9)),
            (f"sag_{tag}_ks1", lambda dt=dt, m6=m6: sag_case(dt, 1, 2, 4, 3, 3, 2, m6, ks=1)),
            (f"sag_{tag}_wrap", lambda dt=dt: sag_case(dt, 2, 4, 364, 364, 91, 91, 1.0 + 0.5 * torch.randn(2, 91 * 91, generator=torch.Generator().manual_seed(7)))),
            (f"sag_{tag}_short_image_refused", lambda dt=dt: sag_refused_case(dt, 4, 9, 9)),
            (f"sag_{tag}_narrow_image_refused", lambda dt=dt: sag_refused_case(dt, 9, 4, 9)),
            (f"sag_{tag}_even_kernel_refused", lambda dt=dt: sag_refused_case(dt, 9, 9, 4)),
        ]
        for s, c in SAG_NEAREST:  # torch's nearest rule, on either axis
            cases += [
                (f"sag_{tag}_nearest_rows_{s}_from_{c}", lambda dt=dt, s=s, c=c: sag_case(dt, 1, 2, s, 9, c, 3, checker_mass(1, c, 3))),
                (f"sag_{tag}_nearest_cols_{s}_from_{c}", lambda dt=dt, s=s, c=c: sag_case(dt, 1, 2, 9, s, 3, c, checker_mass(1, 3, c))),
            ]
        cases += [(f"silu_{tag}_{n}", lambda dt=dt, n=n: silu_case(dt, n)) for n in (1, 255, 257, WRAP + 3)]
        cases += [(f"axpby_{tag}_{n}", lambda dt=dt, n=n: axpby_case(dt, n)) for n in (3, *range(41, 48))]  # 8 * 5 + r: every tail length of both dtypes
        cases.append((f"axpby_{tag}_wrap", lambda dt=dt: axpby_case(dt, 8 * WRAP + 13)))  # more than 2^20 vectors in either dtype, and a tail
        cases += [
            (f"concat2_{tag}_wide_rows", lambda dt=dt: concat2_case(dt, 5, 16, 24)),
            (f"concat2_{tag}_wrap", lambda dt=dt: concat2_case(dt, WRAP // 2 + 3, 8, 8)),  # 2 (bfloat16) / 4 (float32) vectors per row
            (f"cfg_ddim_{tag}_65537", lambda dt=dt: cfg_ddim_case(dt, 65537)),
            (f"cfg_ddim_{tag}_wrap", lambda dt=dt: cfg_ddim_case(dt, WRAP + 5)),
        ]
        # LayerNorm: both ends of the nvec range of the MAXV = 1, 2, 4, 8, 16 instances (bfloat16 C = 8, 512, 520, ... 8192; float32 half of that)
        cases += [(f"layernorm_{tag}_{nv}vec", lambda dt=dt, nv=nv: layernorm_edge_case(dt, nv)) for nv in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)]
        cases += [(f"layernorm_{tag}_{nv}vec_mean100", lambda dt=dt, nv=nv: layernorm_edge_case(dt, nv, narrow=True)) for nv in (65, 1024)]
        cases.append((f"layernorm_{tag}_1025vec_refused", lambda dt=dt: layernorm_refused_case(dt)))
        # GroupNorm at HW = 1, 3, 5 (fewer pixels than pixel lanes) and B = 3: group widths 1, 4, 16; G = 1 and 8 at C = 64.  (The statistics
        # kernels at widths 4 and 16 with HW = 30 / 64 run in test_tiled_vae_kernels_gpu.py through mi355x_groupnorm_table; widths 10 ... 80 at
        # HW >= 256 in kernel_cases.py.)  Width 256 is the widest the finalize kernel takes: C = 8192 in bfloat16; float32 rows hold at most
        # 1024 vectors = 4096 channels, so there it is C = 4096 in 16 groups and C = 8192 is refused.
        cases += [(f"groupnorm_{tag}_C{C}_G{G}", lambda dt=dt, C=C, G=G: groupnorm_edge_case(dt, C, G)) for C, G in ((32, 32), (128, 32), (512, 32), (64, 1), (64, 8))]
        cases += [(f"groupnorm_{tag}_C{C}_G{G}_constant", lambda dt=dt, C=C, G=G: groupnorm_edge_case(dt, C, G, HWs=(5,), constant=True)) for C, G in ((128, 32), (64, 1))]
        if dt == torch.bfloat16:
            cases.append((f"groupnorm_{tag}_width256", lambda dt=dt: groupnorm_edge_case(dt, 8192, 32, HWs=(8,), B=2)))
        else:
            cases.append((f"groupnorm_{tag}_width256", lambda dt=dt: groupnorm_edge_case(dt, 4096, 16, HWs=(8,), B=2)))
            cases.append((f"groupnorm_{tag}_C8192_refused", lambda dt=dt: groupnorm_refused_case(dt, 8192, 32)))
    return cases
