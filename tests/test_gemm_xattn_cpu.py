"""mi355x_gemm_attention without a GPU: every refusal the header lists returns its code (a refused call launches nothing, so no device is
needed), a model of the fused kernel's LDS plan (csrc/gemm_kernel.cuh, XATTN), and a dry-run lowering of the SDXL tree with the lever on and off."""
from __future__ import annotations

import ctypes as C
from collections import Counter

import pytest
import torch

import refiners_amd
from refiners_amd import native, synth
from refiners_amd.engine.packing import launches
from refiners_amd.latent_diffusion.sdxl import SDXLUNet
from tests import support as S
from tests.test_lowering_cpu import _dry

OK, EDTYPE, ESHAPE, EARG = 0, -1, -2, -4
P = 0x7F0000001000  # a 4 KB-aligned address nobody reads: refusals are decided from the arguments alone


@pytest.fixture(scope="module")
def lib():
    from refiners_amd.build_native import build_native

    build_native()
    return native.load()


def _valid(B=2, H=20, Lq=1024, K=1280, Lk=77, Lk2=4):
    """The benchmarked step's 1024-token class: LayerNorm folded in, in-launch LoRA of stacked rank 32, text + image-prompt keys."""
    g, a = native.GemmArgs(), native.AttnArgs()
    g.dtype, g.M, g.N, g.nseg = native.MI355X_BF16, B * Lq, H * 64, 1
    sg = g.seg[0]
    sg.x, sg.ldx, sg.w, sg.ldw, sg.k, sg.ksize, sg.stride, sg.ups, sg.kblocked = P, K, P, K, K, 1, 1, 1, 1
    g.rows_per_group = 1
    g.ln_stats, g.ln_parts, g.ln_eps, g.ln_s, g.ln_c = P, K // 32, 1e-5, P, P
    g.lora_a[0], g.lora_nb[0], g.lora_groups, g.lora_r, g.lora_b, g.lora_ls, g.lora_lc = P, 0, 1, 32, P, P, P
    g.lora_t, g.lora_flags, g.lora_epoch = P, P, P
    a.dtype, a.B, a.H, a.D, a.Lq, a.nstream, a.scale = native.MI355X_BF16, B, H, 64, Lq, 2 if Lk2 else 1, 0.125
    a.out, a.ldo, a.o_batch_stride = P, H * 64, Lq * H * 64
    for s, n in enumerate((Lk, Lk2)[: a.nstream]):
        kv = a.kv[s]
        lkp = (n + 63) // 64 * 64
        kv.k, kv.ldk, kv.k_batch_stride, kv.vt, kv.ldvt, kv.vt_batch_stride, kv.Lk, kv.out_scale = P, H * 64, lkp * H * 64, P, B * lkp, lkp, n, 1.0
    return g, a


def _set(obj, path, value):
    *head, last = path.split(".")
    for h in head:
        obj = getattr(obj, h[:-3])[int(h[-2])] if h.endswith("]") else getattr(obj, h)
    if last.endswith("]"):
        getattr(obj, last[:-3])[int(last[-2])] = value
    else:
        setattr(obj, last, value)


REFUSALS = [
    ("g", "dtype", native.MI355X_F32, EDTYPE), ("a", "dtype", native.MI355X_F32, EDTYPE), ("g", "dtype", 5, EDTYPE),
    ("a", "out", None, EARG),
    ("a", "D", 32, ESHAPE), ("g", "N", 1216, ESHAPE), ("g", "M", 2047, ESHAPE), ("a", "B", 1, ESHAPE),
    ("a", "nstream", 3, ESHAPE), ("a", "nstream", 0, ESHAPE), ("a", "kv[0].Lk", 0, ESHAPE), ("a", "kv[1].Lk", 0, ESHAPE),
    ("a", "kv[0].Lk", 129, ESHAPE),   # 3 + 1 tiles
    ("a", "kv[0].Lk", 97, ESHAPE),    # three tiles, the second with more than 32 keys
    ("a", "kv[1].Lk", 33, ESHAPE),    # three tiles, the third with more than 32 keys
    ("a", "kv[1].Lk", 65, ESHAPE),    # 2 + 2 tiles
    ("g", "nseg", 2, ESHAPE), ("g", "conv", 1, ESHAPE), ("g", "geglu", 1, ESHAPE), ("g", "geglu", 2, ESHAPE), ("g", "res", P, ESHAPE), ("g", "rowbias", P, ESHAPE),
    ("g", "out_t", P, ESHAPE), ("g", "out_f32", 1, ESHAPE), ("g", "ksplit", 2, ESHAPE), ("g", "stats_out", P, ESHAPE), ("g", "colstats_out", P, ESHAPE),
    ("g", "out_kblocked", 1, ESHAPE),
    ("g", "lora_r", 64, ESHAPE), ("g", "lora_groups", 2, ESHAPE),
    ("g", "tile", 1, ESHAPE), ("g", "tile", 2, ESHAPE), ("g", "tile", 9, ESHAPE),
    ("g", "seg[0].ldx", 1 << 21, ESHAPE),   # x spans 2 GB and more
    ("a", "kv[0].ldk", 1 << 24, ESHAPE),    # 64 key rows span 2 GB and more
    ("a", "ldo", 1 << 21, ESHAPE),          # the output spans 2 GB and more
    ("g", "seg[0].k", 1290, ESHAPE), ("a", "kv[0].k", P + 8, ESHAPE), ("g", "ln_s", None, ESHAPE),  # mi355x_gemm's / mi355x_attention's own checks still apply
]


@pytest.mark.parametrize("which,field,value,code", REFUSALS, ids=[f"{w}.{f}={v}" for w, f, v, _ in REFUSALS])
def test_refusals_return_their_code_without_a_device(lib, which, field, value, code):
    g, a = _valid()
    _set(g if which == "g" else a, field, value)
    assert lib.mi355x_gemm_attention(C.byref(g), C.byref(a), None) == code


def test_null_arguments_and_lq_rule(lib):
    g, a = _valid()
    assert lib.mi355x_gemm_attention(None, C.byref(a), None) == EARG and lib.mi355x_gemm_attention(C.byref(g), None, None) == EARG
    g, a = _valid(B=2, Lq=1000)  # M = B Lq holds, but a 64-row tile would straddle the two batch elements
    assert lib.mi355x_gemm_attention(C.byref(g), C.byref(a), None) == ESHAPE
    assert lib.mi355x_gemm_attention.argtypes == [C.POINTER(native.GemmArgs), C.POINTER(native.AttnArgs), C.c_void_p]


# ------------------------------------------------------------------------------------------------ LDS plan
RING, STAGE, SLOT, TILEB, CU_LDS = 32768, 16384, 16384, 8192, 163840


def lds_plan(ln: bool, lora: bool, lk: int, lk2: int):
    """Byte ranges of the fused kernel's LDS regions, as csrc/gemm_kernel.cuh lays them out: {name: [(begin, end), ...]} and the total."""
    r = {"stage0": [(0, STAGE)], "stage1": [(STAGE, RING)]}
    top = RING
    if ln:
        r["rowstat"] = [(top, top + 512)]
        top += 512
    if lora:
        r["lora_b0"] = [(top, top + 4096)]
        top += 4096
    r["slot0"] = [(top, top + SLOT)]
    top += SLOT
    tiles = [(s, 64 * t, n) for s, n in enumerate((lk, lk2)) if n for t in range((n + 63) // 64)]
    ntot = len(tiles)
    for sl, (_s, kv0, n) in enumerate(tiles):
        if sl == 0:
            continue
        base = (sl - 1) * SLOT
        half = n - kv0 <= 32
        r[f"late{sl}"] = [(base, base + (TILEB // 2 if half else TILEB)), (base + TILEB, base + 2 * TILEB)]  # K rows written, V^T rows
    r["qimage"] = [(4096, 8192), (20480, 24576)] if ntot == 3 else [(16384, 24576)]
    return r, top, ntot


def q_off(row: int, chunk: int, ntot: int) -> int:
    t = lambda rw: rw * 128 + ((chunk ^ ((rw >> 1) & 7)) << 4)  # noqa: E731  (tile_off<128>)
    return 4096 + (row >> 5) * 16384 + t(row & 31) if ntot == 3 else 16384 + t(row)


def _disjoint(ranges):
    flat = sorted(x for rs in ranges for x in rs)
    return all(a[1] <= b[0] for a, b in zip(flat, flat[1:]))


@pytest.mark.parametrize("lk,lk2", [(1, 0), (32, 0), (33, 0), (64, 0), (65, 0), (77, 0), (128, 0), (77, 4), (64, 16), (33, 33), (96, 32), (64, 64), (65, 1)])
@pytest.mark.parametrize("ln,lora", [(False, False), (True, False), (False, True), (True, True)])
def test_lds_plan_never_overlaps_live_regions_and_fits_three_workgroups(ln, lora, lk, lk2):
    r, total, ntot = lds_plan(ln, lora, lk, lk2)
    fixed = [r[k] for k in ("rowstat", "lora_b0", "slot0") if k in r]
    # K loop: both stages, the row statistics, the first up-projection chunk and slot 0 (arriving by LDS-DMA) are live
    assert _disjoint([r["stage0"], r["stage1"]] + fixed)
    # after the loop: the stages are dead; the late tiles (arriving), the Q image, and everything outside the ring are live
    late = [r[k] for k in r if k.startswith("late")]
    assert _disjoint(late + [r["qimage"]] + fixed)
    assert all(e <= RING for rs in late + [r["qimage"]] for _b, e in rs), "late tiles and the Q image stay inside the drained ring"
    assert sum(e - b for b, e in r["qimage"]) == 64 * 128
    assert total == RING + 512 * ln + 4096 * lora + SLOT and 3 * total <= CU_LDS
    assert total <= 54613 and max(e for rs in r.values() for _b, e in rs) <= total
    # the Q exchange: lane (g, c16) of wave (wm, wn) writes chunk 4 wn + g of rows 32 wm + 16 i + c16; wave w reads chunks 4 s + g of rows 16 w + c16
    written = Counter(q_off(32 * wm + 16 * i + c16, 4 * wn + g, ntot) for wm in range(2) for wn in range(2) for i in range(2) for g in range(4) for c16 in range(16))
    assert len(written) == 512 and set(written.values()) == {1}
    assert all(any(b <= o and o + 16 <= e for b, e in r["qimage"]) for o in written)
    read = {q_off(16 * w + c16, 4 * s + g, ntot) for w in range(4) for s in range(2) for g in range(4) for c16 in range(16)}
    assert read == set(written)


def test_with_the_production_forms_the_fourth_workgroup_does_not_fit():
    """Why the kernel asks for three waves per SIMD: 53 760 bytes with LayerNorm and LoRA -- three workgroups, 768 slots on 256 CUs for the 640 tiles."""
    _r, total, _n = lds_plan(True, True, 77, 4)
    assert total == 53760 and 3 * total == 161280 and 4 * total > CU_LDS and 3 * 256 >= (2048 // 64) * (1280 // 64)


# ------------------------------------------------------------------------------------------------ lowering
TOKENS = {("cross_attention_block", "clip_text_embedding"): (77, 2048), ("ip_adapter", "clip_image_embedding"): (4, 2048)}


def _tree(ip: bool):
    unet = SDXLUNet(4, device="meta", dtype=torch.bfloat16)
    if ip:
        specs = S.build_specs(S.CASES["sdxl_lora_ip"], S.key_shapes("sdxl"))
        specs["loras"] = []  # (on the meta device a LoRA takes the two-launch path: its Q projection is no plain GEMM)
        synth.apply_adapters(unet, refiners_amd.namespace(), device="meta", dtype=torch.bfloat16, **specs)
    return unet


def _kinds(low):
    return Counter(e[2] for e in low.step)


@pytest.mark.parametrize("ip", [False, True], ids=["bare", "ip"])
def test_lowering_folds_every_cross_attention_with_the_lever_on(monkeypatch, ip):
    tokens = TOKENS if ip else {k: v for k, v in list(TOKENS.items())[:1]}
    monkeypatch.setenv("REFINERS_AMD_XATTN_FOLD", "0")
    off = _dry(_tree(ip), 2, 32, 32, torch.bfloat16, tokens)
    monkeypatch.delenv("REFINERS_AMD_XATTN_FOLD")
    default = _dry(_tree(ip), 2, 32, 32, torch.bfloat16, tokens)
    monkeypatch.setenv("REFINERS_AMD_XATTN_FOLD", "1")
    on = _dry(_tree(ip), 2, 32, 32, torch.bfloat16, tokens)
    ko, kn = _kinds(off), _kinds(on)
    assert [e[2] for e in default.step] == [e[2] for e in off.step], "a dry run on the meta device keeps the two-launch program unless the lever is set"
    assert ko["mi355x_attention"] == 140 and ko["mi355x_gemm_attention"] == 0 and off.stats.get("xattn_fold_sites", 0) == 0
    assert kn["mi355x_gemm_attention"] == 70 and kn["mi355x_attention"] == 70 and on.stats["xattn_fold_sites"] == 70
    assert launches(on.step) == launches(off.step) - 70 and kn["mi355x_gemm"] == ko["mi355x_gemm"] - 70
    assert on.stats["fallback_nodes"] == [] and (on.stats["ip_sites"] == 70) == ip
    # what is left of mi355x_attention is the self-attentions: one stream of as many keys as queries
    for e in on.step:
        if e[2] == "mi355x_attention":
            a = e[1][0]._obj
            assert a.nstream == 1 and a.kv[0].Lk == a.Lq
    # a folded launch carries both structs, the GEMM's first (weight prefetch and the roofline read it there), and no Q pointers
    for e in on.step:
        if e[2] == "mi355x_gemm_attention":
            g, a = e[1][0]._obj, e[1][1]._obj
            assert (g.M, g.N, g.tile, g.nseg) == (a.B * a.Lq, a.H * 64, 4, 1) and not g.out and not a.q and a.nstream == (2 if ip else 1)
            assert native.gemm_signature(g).endswith("xa")
    assert native.link_weight_prefetch(list(on.step))["launches"] == native.link_weight_prefetch(list(off.step))["launches"]


def test_lowering_keeps_two_launches_where_the_rule_says_so(monkeypatch):
    monkeypatch.setenv("REFINERS_AMD_XATTN_FOLD", "1")
    # float32 parity mode
    low = _dry(SDXLUNet(4, device="meta", dtype=torch.float32), 2, 32, 32, torch.float32, {k: v for k, v in list(TOKENS.items())[:1]})
    assert _kinds(low)["mi355x_gemm_attention"] == 0
    # token counts that are no multiple of 64 (24 x 16 latents: 96 and 24 tokens): a row tile would straddle two batch elements
    low = _dry(SDXLUNet(4, device="meta", dtype=torch.bfloat16), 2, 24, 16, torch.bfloat16, {k: v for k, v in list(TOKENS.items())[:1]})
    assert _kinds(low)["mi355x_gemm_attention"] == 0
    # a text stream of four tiles (ELLA-sized)
    low = _dry(SDXLUNet(4, device="meta", dtype=torch.bfloat16), 2, 32, 32, torch.bfloat16, {list(TOKENS)[0]: (200, 2048)})
    assert _kinds(low)["mi355x_gemm_attention"] == 0
    # the benchmarked size: the 1024-token class folds (64 x 64 tiles), the 4096-token class (M = 8192, N = 640: 128-row tiles) only when the lever says 2
    for lever, n in (("1", 60), ("2", 70)):
        monkeypatch.setenv("REFINERS_AMD_XATTN_FOLD", lever)
        low = _dry(SDXLUNet(4, device="meta", dtype=torch.bfloat16), 2, 128, 128, torch.bfloat16, {k: v for k, v in list(TOKENS.items())[:1]})
        assert _kinds(low)["mi355x_gemm_attention"] == n
