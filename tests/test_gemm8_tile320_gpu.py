"""Tile id 12 of mi355x_gemm: the 8-wave eight-phase loop on 128 x 320 tiles (wave tile 64 x 80, refiners_amd/csrc/gemm8_kernel.cuh NT = 5), against
float32 torch at the loop's bf16 bound (kernel_cases._tol: 1.6e-2 of the reference's max-abs), outputs NaN-filled before every launch.  Every case checks
through mi355x_get_stat("g12") that the tile really ran, or, for the epilogues it does not take (GEGLU, LayerNorm-folded, row statistics, in-launch
LoRA), that the launch went elsewhere and is still right."""
import pytest
import torch
import torch.nn.functional as F

from tests import kernel_cases
from tests.kernel_cases import DEV, _cmp, _rand

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _require_native(gpu_device):
    from refiners_amd import native

    native.load()


def _g12():
    from refiners_amd import native

    return native.load().mi355x_get_stat(b"g12")


def _ok(e):
    err, scale, tol = e
    assert err <= tol * scale + 1e-7, f"max|err|={err:.3e} vs ref max {scale:.3e} (tol {tol:g} relative)"


def _ran_on_12(fn):
    torch.cuda.synchronize()
    n0 = _g12()
    e = fn()
    torch.cuda.synchronize()
    assert _g12() > n0, "the launch did not run on tile 12"
    return e


@pytest.mark.parametrize("M,K,N", [(256, 640, 320), (300, 320, 640), (1000, 1280, 1280), (130, 640, 10240), (4096, 320, 320), (300, 64, 320)])
@pytest.mark.parametrize("epi", ["plain", "bias_res", "rowbias_gelu"])
def test_gemm_tile12(M, K, N, epi):
    """N = 320 / 640 / 1280 / 10240; M not a multiple of 128 (a partial last row tile) except for the whole-round case."""
    from refiners_amd import native

    x = _rand(M, K, dtype=BF, seed=M + N)
    w = _rand(N, K, dtype=BF, seed=M + N + 1, scale=K ** -0.5)
    b = _rand(N, dtype=BF, seed=3) if epi != "plain" else None
    r = _rand(M, N, dtype=BF, seed=4) if epi == "bias_res" else None
    rpg = 7 if epi == "rowbias_gelu" else 1
    rb = _rand((M + rpg - 1) // rpg, N, dtype=BF, seed=5) if epi == "rowbias_gelu" else None
    out = torch.full((M, N), float("nan"), dtype=BF, device=DEV)

    def run():
        native.gemm([(x, native.KBlocked(w))], out, bias=b, res=r, rowbias=rb, rows_per_group=rpg, gelu=epi == "rowbias_gelu", tile=12)
        ref = x.double() @ w.double().t()
        if b is not None:
            ref = ref + b.double()
        if rb is not None:
            ref = ref + rb.double().repeat_interleave(rpg, dim=0)[:M]
            ref = F.gelu(ref)
        if r is not None:
            ref = ref + r.double()
        return _cmp(out, ref.float(), BF)

    _ok(_ran_on_12(run))


def test_gemm_tile12_bit_reproducible():
    from refiners_amd import native

    x = _rand(777, 640, dtype=BF, seed=1)
    w = native.KBlocked(_rand(640, 640, dtype=BF, seed=2, scale=640 ** -0.5))
    o1, o2 = torch.full((777, 640), float("nan"), dtype=BF, device=DEV), torch.zeros(777, 640, dtype=BF, device=DEV)
    native.gemm([(x, w)], o1, tile=12)
    native.gemm([(x, w)], o2, tile=12)
    assert torch.equal(o1, o2)


@pytest.mark.parametrize("kw", [{}, {"stride": 2}, {"ups": 2}, {"split": 640, "rowbias": True, "res": True}, {"Cout": 640}])
def test_conv_tile12(kw):
    """3x3 with zero padding, stride 2, nearest-2x input, and three segments (a two-way channel split + fused 1x1 shortcut); row bias and residual."""
    kw = dict(kw)
    cout = kw.pop("Cout", 320)
    cin = 960 if "split" in kw else 320
    _ok(_ran_on_12(lambda: kernel_cases.conv_case(2, cin, cout, 16, 12, BF, seed=222, tile=12, **kw)))


def test_conv_three_segments_tile12():
    """Three real K segments, as a decoder-side concat conv: two NHWC images concatenated along C + a 1x1 shortcut of a third."""
    from refiners_amd import native

    B, H, W = 2, 8, 8
    xa, xb, xc = _rand(B, H, W, 320, dtype=BF, seed=10), _rand(B, H, W, 640, dtype=BF, seed=11), _rand(B, H, W, 320, dtype=BF, seed=12)
    wa = _rand(320, 320, 3, 3, dtype=BF, seed=13, scale=(960 * 9) ** -0.5)
    wb = _rand(320, 640, 3, 3, dtype=BF, seed=14, scale=(960 * 9) ** -0.5)
    wc = _rand(320, 320, 1, 1, dtype=BF, seed=15, scale=320 ** -0.5)
    out = torch.full((B * H * W, 320), float("nan"), dtype=BF, device=DEV)

    def run():
        segs = [(xa, native.pack_conv_weight(wa), 3, 1, 1), (xb, native.pack_conv_weight(wb), 3, 1, 1), (xc, native.pack_conv_weight(wc), 1, 1, 1)]
        native.conv_gemm(segs, out, B, H, W, tile=12)
        nchw = lambda t: t.double().permute(0, 3, 1, 2)  # noqa: E731
        ref = F.conv2d(nchw(xa), wa.double(), padding=1) + F.conv2d(nchw(xb), wb.double(), padding=1) + F.conv2d(nchw(xc), wc.double())
        return _cmp(out.float().reshape(B, H, W, 320).permute(0, 3, 1, 2), ref.float(), BF)

    _ok(_ran_on_12(run))


@pytest.mark.parametrize("M,N", [(200, 320), (1000, 640), (96, 1280)])
def test_colstats_tile12(M, N):
    """GroupNorm column statistics from the epilogue: 80-column waves, so 32-column chunks straddle two waves and every lane hands over 16 + 4 columns."""
    _ok(_ran_on_12(lambda: kernel_cases.colstats_case(M, 640, N, BF, tile=12)))
    _ok(_ran_on_12(lambda: kernel_cases.colstats_case(M, 320, N, BF, tile=12, res=False, seed=311)))


@pytest.mark.parametrize("Cout", [320, 640])
def test_conv_groupnorm_chain_tile12(Cout):
    _ok(_ran_on_12(lambda: kernel_cases.conv_groupnorm_chain_case(2, 320, Cout, 16, 16, BF, tile=12)))


def test_epilogues_tile12_refuses_run_elsewhere():
    """GEGLU + LayerNorm-folded, row statistics (residual + stats) and live LoRA producers on FF1 ask for tile 12 and run on the library's own choice:
    right results, and the g12 counter does not move."""
    torch.cuda.synchronize()
    n0 = _g12()
    _ok(kernel_cases.gemm_ln_chain_case(256, 640, 2560, BF, geglu=True, tile1=12, tile2=12))
    _ok(kernel_cases.gemm_ln_chain_case(300, 640, 640, BF, tile1=12, tile2=12))
    _ok(kernel_cases.gemm_lora_inlaunch_case(256, 640, 1280, BF, ranks=(16, 16), tile=12, geglu=True))
    torch.cuda.synchronize()
    assert _g12() == n0
