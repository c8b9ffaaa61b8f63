"""Every tile id of the 8-wave loop, driven from the table (refiners_amd/engine/tiles.py): a forced-tile launch with an edge tile in both directions runs on
that id (its mi355x_get_stat counter moves by exactly one) and is right against float32 torch at kernel_cases' tolerances; the same launch with a feature the
row refuses (csrc/gemm_tiles.cuh) is still right and does NOT run on that id -- the fallback the contract promises.  (Id 11 needs a shape plan_mix admits: the
tile11 cases of kernel_cases.py.)"""
import pytest
import torch
import torch.nn.functional as F

from refiners_amd.engine import tiles
from tests import kernel_cases
from tests.kernel_cases import DEV, _cmp, _rand

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
M, K, MP = 300, 128, 304  # (MP: row stride of a transposed group's output, 16-byte aligned)
ROWS = [t for t in tiles.TILES if t.loop == 8 and not t.bm2]


def width(t):
    return 960 if t.bn == 320 else 640


@pytest.fixture(scope="module")
def data(gpu_device):
    """x, w and the float32 product per dtype, computed once and left alone."""
    from refiners_amd import native

    native.load()
    d = {}
    for dt in (BF, F32):
        x, w = _rand(M, K, dtype=dt, seed=901), _rand(960, K, dtype=dt, seed=902, scale=K ** -0.5)
        d[dt] = (x, w, x.float() @ w.float().t())
    return d


def _ok(e):
    err, scale, tol = e
    print(f"max|err|={err:.3e} ref max {scale:.3e} tol {tol:g}")
    assert err <= tol * scale + 1e-7, f"max|err|={err:.3e} vs ref max {scale:.3e} (tol {tol:g} relative)"


def _moves(t, fn):
    torch.cuda.synchronize()
    n0 = kernel_cases._launch_stat(tiles.stat(t.id).encode())
    _ok(fn())
    torch.cuda.synchronize()
    return kernel_cases._launch_stat(tiles.stat(t.id).encode()) - n0


def _nan(*shape, dtype=BF):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def launch(data, t, feature):
    from refiners_amd import native

    N = width(t)
    dt = F32 if feature == "f32" else BF
    x, w, ref = data[dt][0], data[dt][1][:N], data[dt][2][:, :N]
    if feature in ("plain", "f32"):
        return _cmp(native.gemm([(x, w)], _nan(M, N, dtype=dt), tile=t.id), ref, dt)
    if feature == "conv":
        return kernel_cases.conv_case(2, 64, 64, 9, 7, BF, seed=910, tile=t.id)
    if feature == "trans":  # the columns from 256 on, transposed
        out, vt = _nan(M, 256), _nan(N - 256, MP)
        native.gemm([(x, w)], out, out_t=vt, nt_begin=256, tile=t.id)
        e1, e2 = _cmp(out, ref[:, :256], BF), _cmp(vt[:, :M], ref[:, 256:].t(), BF)
        return max(e1[0], e2[0]), max(e1[1], e2[1]), e1[2]
    if feature == "geglu":
        perm = native.geglu_pack_index(N // 2, device=DEV)
        out = native.gemm([(x, native.KBlocked(w[perm].contiguous()))], _nan(M, N // 2), geglu=True, tile=t.id)
        return _cmp(out, ref[:, : N // 2] * F.gelu(ref[:, N // 2 :]), BF)
    if feature == "ln":  # LayerNorm (unit weight, no bias) of x folded into the launch
        stats = kernel_cases._stats_ref(x.float()).to(DEV)
        out = native.gemm([(x, w)], _nan(M, N), ln=(stats, w.float().sum(1).contiguous(), torch.zeros(N, device=DEV), 1e-5), tile=t.id)
        return _cmp(out, F.layer_norm(x.float(), (K,), eps=1e-5) @ w.float().t(), BF)
    if feature == "stats":
        stats = _nan(N // 32, M, 2, dtype=F32)
        out = native.gemm([(x, w)], _nan(M, N), stats_out=stats, tile=t.id)
        sref = kernel_cases._stats_ref(out.float())
        assert (stats - sref).abs().max().item() <= 2e-5 * sref.abs().max().item()  # (gemm_ln_chain_case's bound)
        return _cmp(out, ref, BF)
    if feature == "out_f32":
        return _cmp(native.gemm([(x, w)], _nan(M, N, dtype=F32), out_f32=True, tile=t.id), ref, F32)
    if feature == "lora":
        a, bs, delta = kernel_cases._lora_pack(K, N, BF, (16, 16), 920)
        out = native.gemm([(x, native.KBlocked(w))], _nan(M, N), lora=([(0, a)], bs), tile=t.id)
        return _cmp(out, x.float() @ (w.float() + delta).t(), BF)
    assert feature == "lora3"  # Q | K | V^T: three column groups with a LoRA set each, the last one transposed (from a multiple of 256: the group alone is no obstacle)
    cols = (0, 256, 512, N)
    packs = [kernel_cases._lora_pack(K, cols[g + 1] - cols[g], BF, (16, 16) if g != 1 else (8,), 930 + 20 * g) for g in range(3)]
    out, vt = _nan(M, 512), _nan(N - 512, MP)
    native.gemm([(x, native.KBlocked(w))], out, out_t=vt, nt_begin=512, lora=([(cols[g], packs[g][0]) for g in range(3)], torch.cat([p[1] for p in packs], 0).contiguous()), tile=t.id)
    full = x.float() @ (w.float() + torch.cat([p[2] for p in packs], 0)).t()
    e1, e2 = _cmp(out, full[:, :512], BF), _cmp(vt[:, :M], full[:, 512:].t(), BF)
    return max(e1[0], e2[0]), max(e1[1], e2[1]), e1[2]


def refused(t):
    """The features row t marks as not taken."""
    out = [f for f, taken in (("trans", t.trans), ("f32", t.f32), ("conv", t.conv)) if not taken]
    if t.plain:
        out += ["geglu", "ln", "stats", "out_f32", "lora"]
    elif t.lora and t.trans:
        out.append("lora3")  # (the loop's LoRA is ONE column group)
    return out


@pytest.mark.parametrize("tile,feature", [(t.id, f) for t in ROWS for f in ["plain"] + (["f32"] if t.f32 else [])])
def test_a_forced_tile_runs_on_its_row(data, tile, feature):
    t = tiles.BY_ID[tile]
    assert _moves(t, lambda: launch(data, t, feature)) == 1


@pytest.mark.parametrize("tile,feature", [(t.id, f) for t in ROWS for f in refused(t)])
def test_a_refused_feature_runs_elsewhere_and_is_right(data, tile, feature):
    t = tiles.BY_ID[tile]
    assert _moves(t, lambda: launch(data, t, feature)) == 0


def test_the_cases_cover_what_the_rows_refuse():
    got = {(t.id, f) for t in ROWS for f in refused(t)}
    want = {(9, "trans"), (10, "trans"), (12, "trans"), (10, "f32"), (10, "conv"), (12, "geglu"), (12, "ln"), (12, "stats"), (12, "out_f32"), (12, "lora"), (7, "lora3")}
    assert want <= got, want - got
