"""ctypes binding of libmi355x_refiners.so (the C ABI declared in include/mi355x_refiners.h).

This module is the ONLY place where Python touches the native library.  It deliberately passes nothing but raw
device pointers, sizes, strides and scalars; torch is used as the owner of device memory and of the current HIP
stream.  There is no CPU or PyTorch fallback here: if the library is missing or a kernel refuses a shape, the call
raises `NativeError` (the fused fluxion nodes decide, *before* calling, whether a sub-tree is eligible).

The header is the only description of the ABI: the argument structs (GemmArgs, AttnArgs, ...), the prototypes `load()` sets and the
scalar constants are read from it at import by refiners_amd.abi, nothing of it is restated here.  What this module adds is the
Python name of each struct (STRUCT_NAMES), the probing entry points the header leaves out on purpose (UNSTABLE), and the wrappers.

A feature's entry points live in an extension header of their own, include/mi355x_refiners_<feature>.h.  Adding one takes a row in
ABI_HEADERS here and its source in build_native.SOURCES: the structs, the bound prototypes, the build's dependencies and the header
tests (tests/test_abi_header_cpu.py) all follow from those two.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from pathlib import Path
from typing import Any, Optional, Sequence

import torch
from torch import Tensor

from . import abi

#: C struct of the header -> the name its ctypes.Structure class has in this module (a header struct that is missing here is an import error)
STRUCT_NAMES = {
    "mi355x_gemm_seg": "GemmSeg",
    "mi355x_gemm_args": "GemmArgs",
    "mi355x_kv_stream": "KvStream",
    "mi355x_attn_args": "AttnArgs",
    "mi355x_attn_general_args": "AttnGeneralArgs",
    "mi355x_layernorm_args": "LayerNormArgs",
    "mi355x_groupnorm_args": "GroupNormArgs",
    "mi355x_sam_attn_args": "SamAttnArgs",
    "mi355x_sam_mask_head_args": "SamMaskHeadArgs",
    "mi355x_sam_postprocess_args": "SamPostprocessArgs",  # its field `in` is `in_` here
    "mi355x_adain_stats_args": "AdainStatsArgs",
    "mi355x_style_aligned_args": "StyleAlignedArgs",
    "mi355x_md_gather_desc": "MdGatherDesc",
    "mi355x_md_gather_args": "MdGatherArgs",
    "mi355x_md_step_args": "MdStepArgs",
    "mi355x_md_blend_desc": "MdBlendDesc",
    "mi355x_md_blend_args": "MdBlendArgs",
    "mi355x_groupnorm_table_args": "GroupNormTableArgs",
    "mi355x_groupnorm_fixed_args": "GroupNormFixedArgs",
    "mi355x_vae_tile_pos": "VaeTilePos",
    "mi355x_vae_gather_args": "VaeGatherArgs",
    "mi355x_vae_axis": "VaeAxis",
    "mi355x_vae_blend_tile": "VaeBlendTile",
    "mi355x_vae_blend_args": "VaeBlendArgs",
}
#: every header of the ABI, mi355x_refiners.h (a frozen list) first: (key, file under include/, {C struct: Python class name})
ABI_HEADERS = [
    ("core", "mi355x_refiners.h", STRUCT_NAMES),
    ("sam_hq", "mi355x_refiners_sam_hq.h", {"mi355x_sam_hq_mask_head_args": "SamHqMaskHeadArgs", "mi355x_sam_mask_head_up_args": "SamMaskHeadUpArgs"}),
    ("solver_step", "mi355x_refiners_solver_step.h", {}),  # the guidance-free solver updates
    ("swin", "mi355x_refiners_swin.h", {"mi355x_window_attention_args": "WindowAttentionArgs"}),
    ("mvanet", "mi355x_refiners_mvanet.h", {"mi355x_mvanet_pool_args": "MvanetPoolArgs", "mi355x_mvanet_gate_args": "MvanetGateArgs", "mi355x_mvanet_resize_add_args": "MvanetResizeAddArgs"}),
    ("dinov2", "mi355x_refiners_dinov2.h", {"mi355x_dinov2_pos_resample_args": "Dinov2PosResampleArgs", "mi355x_dinov2_tokens_args": "Dinov2TokensArgs"}),
    ("ella", "mi355x_refiners_ella.h", {"mi355x_ella_adaln_args": "EllaAdaLnArgs"}),  # the AdaLayerNorm pass of ELLA's Perceiver resampler
    ("lineart", "mi355x_refiners_lineart.h", {"mi355x_lineart_stem_args": "LineartStemArgs", "mi355x_lineart_in_stats_args": "LineartInStatsArgs",
                                              "mi355x_lineart_in_apply_args": "LineartInApplyArgs", "mi355x_lineart_head_args": "LineartHeadArgs"}),
    ("reference_only", "mi355x_refiners_reference_only.h", {"mi355x_attn_joint_args": "AttnJointArgs"}),  # the joint self-attention of reference-only control
    ("cond_input", "mi355x_refiners_cond_input.h", {}),  # step-constant UNet input channels (inpainting, IC-Light)
    ("xattn", "mi355x_refiners_xattn.h", {}),  # a cross-attention folded into its Q projection: it takes the core header's GemmArgs and AttnArgs
    ("sde_step", "mi355x_refiners_sde_step.h", {}),  # the stochastic solver updates (SDE DPM-Solver++)
]
#: key -> what refiners_amd.abi read from that header (a name that two headers declare is an import error)
ABIS = abi.read_all(ABI_HEADERS)
globals().update({cls.__name__: cls for a in ABIS.values() for cls in a.structs.values()})  # GemmSeg ... AttnJointArgs: real ctypes.Structure subclasses
_abi = ABIS["core"]
_K = _abi.constants

#: every symbol include/mi355x_refiners.h declares (tests check that the library exports all of them)
EXPORTS = list(_abi.functions)
#: every symbol any header declares, in table order: what load() binds and the build checks
ALL_EXPORTS = [name for a in ABIS.values() for name in a.functions]
#: exported for probing and A/B runs, by design not in the header (no stable contract): name -> (restype, argtypes), applied by load() like the header's
UNSTABLE = {
    "mi355x_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "mi355x_get_stat": (C.c_int, [C.c_char_p]),
    "mi355x_attention_set_glds": (C.c_int, [C.c_int]),
    "mi355x_attention_set_nw": (C.c_int, [C.c_int]),
    "mi355x_attention_set_pipeline": (C.c_int, [C.c_int, C.c_int]),
    "mi355x_attention_general_set_fast": (C.c_int, [C.c_int]),
}

ABI_VERSION = _K["MI355X_ABI_VERSION"]
MI355X_F32, MI355X_BF16 = _K["MI355X_F32"], _K["MI355X_BF16"]
MAX_SEG, MAX_PREFETCH = _K["MI355X_MAX_SEG"], _K["MI355X_MAX_PREFETCH"]
_ERR = {v: k[len("MI355X_"):] for k, v in next(e for e in _abi.enums if "MI355X_OK" in e).items()}  # 0: "OK", -1: "EDTYPE", ...

LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libmi355x_refiners.so"


class NativeError(RuntimeError):
    """Raised when the native library is unavailable or a native call returns a negative status."""


class KBlocked:
    """A weight matrix [N, K] re-laid K-BLOCKED for mi355x_gemm: `t` is [K * itemsize / 128][N][128 / itemsize], so the
    N x 128-byte slab one K step of the kernel streams is contiguous (mi355x_gemm_seg.kblocked).  global -> LDS streaming
    runs at 10 TB/s on 2.5 KB rows but 5 TB/s on 10 KB rows and 4.5 TB/s on the 23-46 KB rows of a 3x3 convolution's
    weights (profiles/r01_aa_probe_glds.log); weights are static, so the host pays for the re-layout once."""

    def __init__(self, w: Tensor, _adopt: Optional[tuple[int, int]] = None) -> None:
        if _adopt is not None:  # `w` already IS the blocked buffer of an [n, k] matrix (written that way by a kernel)
            self.N, self.K = _adopt
            self.t = w
            return
        assert w.dim() == 2 and w.stride(1) == 1
        n, k = w.shape
        blk = 128 // w.element_size()
        assert k % blk == 0, f"K = {k} is not a multiple of {blk}"
        self.N, self.K = n, k
        self.t = w.reshape(n, k // blk, blk).permute(1, 0, 2).contiguous()

    @classmethod
    def adopt(cls, buf: Tensor, rows: int, k: int) -> "KBlocked":
        """Wrap a contiguous buffer of rows * k elements that a kernel fills in blocked order (mi355x_gemm_args.out_kblocked)."""
        assert buf.is_contiguous() and buf.numel() == rows * k
        return cls(buf, _adopt=(rows, k))

    def dense(self) -> Tensor:
        """Back to a row-major [N, K] tensor (tests / debugging)."""
        blk = 128 // self.t.element_size()
        return self.t.view(self.K // blk, self.N, blk).permute(1, 0, 2).reshape(self.N, self.K)

    @property
    def shape(self) -> tuple[int, int]:
        return (self.N, self.K)

    def data_ptr(self) -> int:
        return self.t.data_ptr()

    @property
    def dtype(self) -> torch.dtype:
        return self.t.dtype

    @property
    def device(self) -> torch.device:
        return self.t.device


LORA_R = 32  # granularity of the stacked LoRA rank mi355x_gemm handles inside the parent launch (gemm_kernel.cuh: LORA_RC)
LORA_RMAX = 128  # largest stacked rank (LORA_RMAX there)


def lora_rank(rt: int) -> int:
    """Stacked rank -> the padded rank the kernel handles (32, 64 or 128); 0 = too large for the in-launch path."""
    return next((r for r in (32, 64, 128) if rt <= r), 0)


_lib: Optional[C.CDLL] = None
_lib_path: Optional[str] = None


def load(path: Optional[Path] = None) -> C.CDLL:
    """Load the shared library (once). Raises NativeError if it has not been built."""
    global _lib, _lib_path
    if _lib is not None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("REFINERS_AMD_LIB") or LIB_PATH)  # (REFINERS_AMD_LIB: an experiment build, tools only)
    if not p.exists():
        raise NativeError(
            f"{p} is missing: build it with `python -m refiners_amd.build_native` (or __graft_entry__.build()). "
            "There is no fallback path for the MI355X kernels."
        )
    try:
        lib = C.CDLL(str(p))
    except OSError as e:  # e.g. no HIP runtime on this machine
        raise NativeError(f"cannot load {p}: {e}") from e
    for name, (restype, argtypes) in {**{name: sig for a in ABIS.values() for name, sig in a.functions.items()}, **UNSTABLE}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.mi355x_abi_version() != ABI_VERSION:
        raise NativeError("libmi355x_refiners.so ABI version mismatch")
    if os.environ.get("REFINERS_AMD_FORCE_TILE"):  # probing: every GEMM / conv launch that can run on this tile configuration does (tools, A/B runs)
        lib.mi355x_set_option(b"tile", int(os.environ["REFINERS_AMD_FORCE_TILE"]))
    _lib = lib
    _lib_path = str(p)
    attention_pipeline_from_env()
    return lib


def attention_pipeline_from_env() -> None:
    """A/B: REFINERS_AMD_ATTN_PIPE="<K/V tiles in flight 1|2>,<XCD-aware block order 0|1>,<OPT bits of attn_kernel>,<short grids: 0 auto = 16-query waves where the grid is short|1 never|2 key-split workgroups always|3 16-query waves always>,<software-pipelined loop 0 off|1 register-staged|2 = 1 without the pinned order|3 LDS-DMA>,<short-K/V kernel: 0 default|1 128-query workgroups|2 64-query workgroups, +4 = the register-staged form>"
    (default 1,1,13,0,3,0; "/" separates as well); read at launch / capture time."""
    import os

    d, x, o, k, sp, sh = (os.environ.get("REFINERS_AMD_ATTN_PIPE", "").replace("/", ",").split(",") + ["", "", "", "", "", ""])[:6]
    _lib.mi355x_attention_set_pipeline(int(d or 1) | (int(o or 13) << 4) | (int(k or 0) << 16) | (int(sp or 3) << 19) | (int(sh or 0) << 23), int(x or 1))


def available() -> bool:
    try:
        load()
        return True
    except NativeError:
        return False


def switch_library(path: Optional[Path]) -> C.CDLL:
    """Tools only (tools/ab_step.py): make another build of the library the one new launches / recordings bind to (None = the product library).
    Programs recorded earlier keep the entry points they were recorded with."""
    global _lib
    _lib = None
    return load(path)


def loaded_library_path() -> Optional[str]:
    """The shared library the process is bound to (the product library unless a tool switched to an experiment build), None before load()."""
    return _lib_path if _lib is not None else None


def check(status: int, what: str) -> None:
    if status != 0:
        raise NativeError(f"{what} failed with MI355X_{_ERR.get(status, status)}")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return MI355X_F32
    if dt == torch.bfloat16:
        return MI355X_BF16
    raise NativeError(f"unsupported dtype {dt} (the MI355X path computes in float32 or bfloat16)")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def device_info() -> str:
    buf = C.create_string_buffer(256)
    check(load().mi355x_device_info(buf, 256), "mi355x_device_info")
    return buf.value.decode()



# ------------------------------------------------------------------------------------------------ launch / record
_recorder: Optional[list] = None


class recording:
    """Context manager: native calls made inside are appended to `ops` instead of being launched.

    The engine lowers a Chain tree once into such a list (all argument structs prebuilt, all buffers static) and then
    replays it, directly or under HIP-graph capture.  An entry is (cfunc, args, name, keepalive)."""

    def __init__(self, ops: list) -> None:
        self.ops = ops

    def __enter__(self) -> list:
        global _recorder
        self._saved = _recorder
        _recorder = self.ops
        return self.ops

    def __exit__(self, *exc: object) -> None:
        global _recorder
        _recorder = self._saved


class not_recording:
    """Context manager: native calls made inside are LAUNCHED even while a program is being recorded (weight preparation at lowering time)."""

    def __enter__(self) -> None:
        global _recorder
        self._saved = _recorder
        _recorder = None

    def __exit__(self, *exc: object) -> None:
        global _recorder
        _recorder = self._saved


def matmul_f32(x: Tensor, w: Tensor, res: Optional[Tensor] = None) -> Tensor:
    """x [M, K] @ w [N, K]^T (+ res) in float32 on the library's own f32 MFMA path (v_mfma_f32_16x16x4_f32), launched at once.  For the
    set-up arithmetic of the engine (LoRA merges, LayerNorm folding): no vendor BLAS inside the product package.  K is zero-padded to the
    kernel's 32-float granularity."""
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.dtype == torch.float32 and w.dtype == torch.float32
    Kp = (K + 31) // 32 * 32

    def prep(t: Tensor) -> Tensor:
        if Kp == K and t.is_contiguous() and t.data_ptr() % 16 == 0:
            return t
        p = torch.zeros(t.shape[0], Kp, dtype=torch.float32, device=t.device)
        p[:, :K] = t
        return p

    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    with not_recording():
        gemm([(prep(x), prep(w))], out, res=res)
    return out


def _launch(sym: str, args: tuple, what: str, keep: tuple = ()) -> None:
    fn = getattr(load(), sym)
    if _recorder is not None:
        _recorder.append((fn, args, what, keep))
        return
    check(fn(*args, stream_ptr()), what)


def record_python(fn, what: str = "python") -> bool:
    """Record a Python callable (torch glue or an unfused fallback sub-tree) as a step of the program being recorded.
    Returns False when nothing is recording (the caller then runs `fn` itself)."""
    if _recorder is None:
        return False
    _recorder.append((None, fn, what, ()))
    return True


def replay(ops: list) -> None:
    """Launch a recorded program on the current stream."""
    s = stream_ptr()
    for fn, args, what, _ in ops:
        if fn is None:
            args()
            continue
        st = fn(*args, s)
        if st:
            check(st, what)

_zeros: dict[int, Tensor] = {}


def zero_page(device: torch.device) -> Tensor:
    idx = (device.index if device.index is not None else torch.cuda.current_device()) if device.type == "cuda" else -1
    z = _zeros.get(idx)
    if z is None:
        z = torch.zeros(256, dtype=torch.uint8, device=device)
        _zeros[idx] = z
    return z


# ------------------------------------------------------------------------------------------------ weight packing
def geglu_pack_index(n_out: int, device: torch.device | str = "cpu") -> Tensor:
    """Row order of a GEGLU-fused Linear(C -> 2*n_out): packed row p holds reference row index[p].

    Packed rows come in blocks of 64 = 32 value rows + 32 gate rows of the same 32 output columns, arranged so that the
    lane that owns packed columns 16g+4j+r (j = 0..3, r = 0..3) of a block holds value columns 8g+4j+r (j < 2) and
    the matching gate columns (j >= 2): see gemm.hip's epilogue.
    """
    assert n_out % 32 == 0, "GEGLU fusion needs the output width to be a multiple of 32"
    p = torch.arange(2 * n_out, device=device)
    blk, q = p // 64, p % 64
    g, j, r = q // 16, (q // 4) % 4, q % 4
    u = 8 * g + 4 * (j % 2) + r
    return torch.where(j >= 2, n_out + 32 * blk + u, 32 * blk + u)


def pack_conv_weight(w: Tensor) -> Tensor:
    """OIHW conv weight -> [O][kh*kw*I] rows with K ordered (ky, kx, channel), as conv mode of mi355x_gemm expects."""
    o, i, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(o, kh * kw * i).contiguous()


# ------------------------------------------------------------------------------------------------ in-launch LoRA hand-off state
class LoraSync:
    """Device-side state of mi355x_gemm's in-launch LoRA (include/mi355x_refiners.h: lora_t / lora_flags / lora_epoch): the epoch word that
    a recorded program bumps once per replay (`bump_op()` goes to the head of the program), per-site flag arrays (zeroed, never shared
    between launches of one replay) and scratch for t = x A^T, which consecutive launches may share (stream order).

    The flag arrays of all sites are cut from a few large int32 chunks, so that the sites' error words (the int32 behind each site's last
    flag, raised by a tile whose hand-over never arrived) can be consulted with ONE gather per chunk: `pending()` is what the engines poll
    at their host sync points (CompiledUNet.check_handovers)."""

    CHUNK = 1 << 20  # int32 words per chunk (4 MB): the SDXL step's 722 sites need ~0.1 M

    def __init__(self, device: torch.device) -> None:
        self.device = device
        self.epoch = torch.zeros(1, dtype=torch.int32, device=device)
        self.chunks: list[Tensor] = []
        self.err_pos: list[list[int]] = []   # per chunk: positions of the sites' error words
        self._err_idx: list[Optional[Tensor]] = []  # the same as device index tensors (built on first use, dropped when a site is added)
        self.cursor = 0

    def flags(self, groups: int, M: int) -> Tensor:
        n = groups * ((M + 31) // 32) + 1  # (+ the launch's error word)
        if not self.chunks or self.cursor + n > self.chunks[-1].numel():
            self.chunks.append(torch.zeros(max(self.CHUNK, n), dtype=torch.int32, device=self.device))
            self.err_pos.append([])
            self._err_idx.append(None)
            self.cursor = 0
        f = self.chunks[-1][self.cursor : self.cursor + n]
        self.err_pos[-1].append(self.cursor + n - 1)
        self._err_idx[-1] = None
        self.cursor += (n + 3) // 4 * 4  # sites start on 16-byte boundaries
        return f

    def reset(self) -> None:
        """Forget every site (eager calls: one launch at a time, fresh flags and a fresh error word per call)."""
        if self.chunks:
            self.chunks, self.err_pos, self._err_idx = self.chunks[:1], [[]], [None]
            self.chunks[0].zero_()
        self.cursor = 0

    def pending(self) -> Optional[Tensor]:
        """A 0-d bool tensor on the device: some site's error word is raised (None: no site yet).  No host synchronisation."""
        parts = []
        for i, (chunk, pos) in enumerate(zip(self.chunks, self.err_pos)):
            if not pos:
                continue
            if self._err_idx[i] is None:
                self._err_idx[i] = torch.tensor(pos, dtype=torch.int64, device=self.device)
            parts.append(chunk[self._err_idx[i]].any())
        if not parts:
            return None
        return parts[0] if len(parts) == 1 else torch.stack(parts).any()

    def clear_errors(self) -> None:
        for i, (chunk, pos) in enumerate(zip(self.chunks, self.err_pos)):
            if pos:
                if self._err_idx[i] is None:
                    self._err_idx[i] = torch.tensor(pos, dtype=torch.int64, device=self.device)
                chunk[self._err_idx[i]] = 0

    def check(self) -> None:
        """Raise if a launch of this state's sites reported a hand-over that never arrived (mi355x_gemm_args.lora_flags: the last word)."""
        bad = self.pending()
        if bad is not None and bool(bad.item()):
            self.clear_errors()
            raise NativeError("mi355x_gemm (in-launch LoRA): a tile waited 2 s for t = x A^T that never came (MI355X_ELAUNCH)")

    def scratch(self, groups: int, M: int, r: int, dtype: torch.dtype) -> Tensor:
        return torch.empty(lora_scratch_rows(groups, M, r, dtype) * r, dtype=dtype, device=self.device)

    def bump_op(self) -> tuple:
        return (getattr(load(), "mi355x_epoch_bump"), (self.epoch.data_ptr(),), "mi355x_epoch_bump", (self,))

    def bump(self) -> None:
        check(load().mi355x_epoch_bump(self.epoch.data_ptr(), stream_ptr()), "mi355x_epoch_bump")


_eager_sync: dict[int, "LoraSync"] = {}


def lora_scratch_rows(groups: int, M: int, R: int, dtype: torch.dtype) -> int:
    """Rows of R elements the in-launch LoRA hand-off scratch needs: every group's block starts on a 128-byte line (mi355x_gemm_args.lora_t)."""
    rb = R * (4 if dtype == torch.float32 else 2)
    return groups * (((M * rb + 127) // 128 * 128) // rb)


def _lora_fill(a: GemmArgs, lora: tuple, ln_given: bool, dtype: torch.dtype, K: int, keep: list, sync: Optional[tuple]) -> None:
    """lora = ([(first column of the group, K-blocked stacked down rows [R, K])], pre-scaled up rows [N, R] (, sA, cA float32 [groups, R])).
    sync = (t scratch, flags, LoraSync) from the engine; None (eager calls: tests, probes) = fresh buffers and an epoch bump per call."""
    groups, lb = lora[0], lora[1]
    R = lb.shape[1]
    assert 1 <= len(groups) <= 3 and lb.dim() == 2 and lb.shape[0] == a.N and R in (32, 64, 128) and lb.is_contiguous() and lb.dtype == dtype
    for g, (nb, la) in enumerate(groups):
        assert isinstance(la, KBlocked) and la.shape == (R, K) and la.dtype == dtype, (la.shape, R, K)
        a.lora_a[g], a.lora_nb[g] = la.data_ptr(), nb
    a.lora_groups, a.lora_r, a.lora_b = len(groups), R, lb.data_ptr()
    if len(lora) > 2:  # LayerNorm folded into this launch as well
        ls_, lc_ = lora[2], lora[3]
        assert ln_given and ls_.dtype == torch.float32 and lc_.dtype == torch.float32 and ls_.is_contiguous() and lc_.is_contiguous()
        assert ls_.numel() == len(groups) * R and lc_.numel() == len(groups) * R
        a.lora_ls, a.lora_lc = ls_.data_ptr(), lc_.data_ptr()
    if sync is None:
        assert _recorder is None, "a recorded program passes its own LoRA hand-off buffers (Lowering.lora_sync)"
        dev = lb.device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        ls = _eager_sync.setdefault(idx, LoraSync(dev))
        ls.reset()
        ls.bump()
        sync = (ls.scratch(len(groups), a.M, R, dtype), ls.flags(len(groups), a.M), ls)
    t, flags, ls = sync
    assert t.numel() >= lora_scratch_rows(len(groups), a.M, R, dtype) * R and t.dtype == dtype and t.data_ptr() % 128 == 0
    assert flags.numel() >= len(groups) * ((a.M + 31) // 32) + 1 and flags.dtype == torch.int32  # (+ the error word)
    a.lora_t, a.lora_flags, a.lora_epoch = t.data_ptr(), flags.data_ptr(), ls.epoch.data_ptr()
    keep.append((lora, t, flags, ls))


# ------------------------------------------------------------------------------------------------ call wrappers
def _seg_plain(x: Any, w: Any) -> tuple:
    """(x, ldx, w, ldw, k, kblocked flags) of one plain K segment; either operand may be a KBlocked weight."""
    assert tuple(x.shape)[1] == tuple(w.shape)[1], (x.shape, w.shape)
    flags = (1 if isinstance(w, KBlocked) else 0) | (2 if isinstance(x, KBlocked) else 0)
    ldx = x.K if isinstance(x, KBlocked) else x.stride(0)
    ldw = w.K if isinstance(w, KBlocked) else w.stride(0)
    for t in (x, w):
        assert isinstance(t, KBlocked) or (t.dim() == 2 and t.stride(1) == 1)
    return (x, ldx, w, ldw, tuple(x.shape)[1], flags)


def gemm(
    segs: Sequence[tuple[Tensor, Tensor]],
    out: Optional[Tensor],
    *,
    bias: Optional[Tensor] = None,
    rowbias: Optional[Tensor] = None,
    rows_per_group: int = 1,
    res: Optional[Tensor] = None,
    geglu: bool = False,
    gelu: bool = False,
    relu: bool = False,
    squared_relu: bool = False,
    M: Optional[int] = None,
    N: Optional[int] = None,
    tile: int = 0,
    stages: int = 0,
    ksplit: int = 1,
    ws: Optional[Tensor] = None,
    prefetch: Optional[Tensor] = None,
    weight_operand: str = "w",
    out_kblocked: bool = False,
    out_t: Optional[Tensor] = None,
    nt_begin: int = 0,
    ln: Optional[tuple[Tensor, Tensor, Tensor, float]] = None,
    stats_out: Optional[Tensor] = None,
    out_f32: bool = False,
    lora: Optional[tuple[Sequence[tuple[int, "KBlocked"]], Tensor]] = None,
    lora_sync: Optional[tuple] = None,
    colstats_out: Optional[Tensor] = None,
    attn: Optional[tuple] = None,
) -> Optional[Tensor]:
    """out[M,N] = epi(sum_s x_s @ w_s^T) for plain row-major 2-D segments (x_s: [M,K_s], w_s: [N,K_s]).
    attn = (AttnArgs, keep-alive) from attention_args(None, ...): this GEMM is the Q projection of that cross-attention and both run as ONE
    launch, mi355x_gemm_attention (include/mi355x_refiners_xattn.h); `out` is None, Q is never written.
    weight_operand="x" marks launches whose PARAMETERS sit in the x slot (transposed projections) for link_weight_prefetch.
    out_t / nt_begin: columns >= nt_begin are written transposed, out_t[n - nt_begin][m] (`out` then has nt_begin columns).
    ln = (stats [parts, M, 2] float32, s [N] float32, c [N] float32, eps): LayerNorm of x folded into this launch (see the header);
    stats_out [N / 32, M, 2] float32: per-row (mean, M2) of every 32-column chunk of the stored output."""
    a = GemmArgs()
    a.weight_is_x = weight_operand == "x"
    a.out_kblocked = int(out_kblocked)
    if prefetch is not None:
        a.prefetch[0], a.prefetch_bytes[0] = prefetch.data_ptr(), prefetch.numel() * prefetch.element_size()
    x0, w0 = segs[0]
    a.dtype = dtype_code(x0.dtype)
    a.M = M if M is not None else x0.shape[0]
    a.N = N if N is not None else w0.shape[0]
    a.nseg = len(segs)
    a.conv = 0
    keep = []
    for s, (x, w) in enumerate(segs):
        t = _seg_plain(x, w)
        sg = a.seg[s]
        sg.x, sg.ldx, sg.w, sg.ldw, sg.k = t[0].data_ptr(), t[1], t[2].data_ptr(), t[3], t[4]
        sg.ksize, sg.stride, sg.ups, sg.H, sg.W, sg.kblocked = 1, 1, 1, 0, 0, t[5]
        keep.append((x, w))
    assert int(bool(geglu)) + int(bool(gelu)) + int(relu) + int(squared_relu) <= 1
    if out_t is not None:
        assert out_t.dim() == 2 and out_t.stride(1) == 1 and out_t.shape[0] >= a.N - nt_begin and out_t.shape[1] >= a.M
        a.out_t, a.ldt, a.nt_begin = out_t.data_ptr(), out_t.stride(0), nt_begin
    if out is None:
        assert attn is not None or (out_t is not None and nt_begin == 0)
        a.out, a.ldo = None, 0
        a.bias = bias.data_ptr() if bias is not None else None
        a.rowbias, a.ld_rowbias, a.rows_per_group, a.res, a.ldres, a.geglu = None, 0, 1, None, 0, 0
    else:
        _fill_epilogue(a, out, bias, rowbias, rows_per_group, res, (3 if gelu == "quick" else 2) if gelu else (4 if relu else (5 if squared_relu else geglu)))
    if out_f32:
        assert out is not None and out.dtype == torch.float32
        a.out_f32 = 1
    if lora is not None:  # LoRA inside this launch (see _lora_fill)
        _lora_fill(a, lora, ln is not None, x0.dtype, tuple(x0.shape)[1], keep, lora_sync)
    if ln is not None:
        stats, ls, lc, eps = ln
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.dim() == 3 and stats.shape[1] == a.M and stats.shape[2] == 2
        assert ls.dtype == torch.float32 and lc.dtype == torch.float32 and ls.numel() == a.N and lc.numel() == a.N and bias is None
        a.ln_stats, a.ln_parts, a.ln_eps, a.ln_s, a.ln_c = stats.data_ptr(), stats.shape[0], eps, ls.data_ptr(), lc.data_ptr()
        keep.append(ln)
    if stats_out is not None:
        assert stats_out.dtype == torch.float32 and stats_out.is_contiguous() and stats_out.numel() >= (a.N // 32) * a.M * 2 and a.N % 64 == 0
        a.stats_out = stats_out.data_ptr()
        keep.append(stats_out)
    _fill_colstats(a, colstats_out, keep)
    _fill_split(a, tile, ksplit, ws, stages, operand=out if out is not None else out_t)
    if attn is not None:
        assert out is None and a.tile in (0, 4)
        a.xattn = True  # (a Python attribute, like weight_is_x: gemm_signature marks the class)
        _launch("mi355x_gemm_attention", (C.byref(a), C.byref(attn[0])), "mi355x_gemm_attention", keep=tuple(keep) + (attn,))
        return None
    _launch("mi355x_gemm", (C.byref(a),), "mi355x_gemm", keep=tuple(keep))
    return out


def conv_gemm(
    segs: Sequence[tuple],
    out: Tensor,
    B: int,
    OH: int,
    OW: int,
    *,
    bias: Optional[Tensor] = None,
    rowbias: Optional[Tensor] = None,
    rows_per_group: int = 1,
    res: Optional[Tensor] = None,
    tile: int = 0,
    ksplit: int = 1,
    ws: Optional[Tensor] = None,
    stages: int = 0,
    lora: Optional[tuple] = None,
    lora_sync: Optional[tuple] = None,
    colstats_out: Optional[Tensor] = None,
    table_may_replace_split: bool = False,
    gelu: bool = False,
) -> Tensor:
    """Implicit-GEMM convolution over NHWC images.  gelu: the erf-GELU epilogue (geglu = 2), not combinable with ksplit.

    segs: (image [B,H,W,C] NHWC-contiguous or channel-sliced view, packed weight [N, ksize*ksize*C], ksize, stride, ups).
    out: [B*OH*OW, N] rows (i.e. NHWC output).
    lora = ([(0, K-blocked packed down-conv weights [R, ksize*ksize*C])], pre-scaled 1x1 up weights [N, R]): Conv2dLora on segment 0 inside this launch.
    """
    a = GemmArgs()
    img0, w0 = segs[0][0], segs[0][1]
    a.dtype = dtype_code(img0.dtype)
    a.M = B * OH * OW
    a.N = w0.shape[0]
    a.nseg = len(segs)
    a.conv = 1
    a.B, a.OH, a.OW = B, OH, OW
    for s, seg in enumerate(segs):
        img, w, ksize, stride, ups = seg[:5]
        asym = seg[5] if len(seg) > 5 else 0
        assert img.dim() == 4 and img.stride(3) == 1, "conv segment must be an NHWC tensor [B,H,W,C]"
        b, h, wd, c = img.shape
        assert img.stride(1) == wd * img.stride(2) and img.stride(0) == h * img.stride(1), "pixels must be uniformly strided"
        assert tuple(w.shape)[1] == ksize * ksize * c and (isinstance(w, KBlocked) or w.stride(1) == 1)
        sg = a.seg[s]
        sg.x, sg.ldx, sg.w, sg.ldw, sg.k = img.data_ptr(), img.stride(2), w.data_ptr(), (w.K if isinstance(w, KBlocked) else w.stride(0)), c
        sg.ksize, sg.stride, sg.ups, sg.H, sg.W, sg.asym = ksize, stride, ups, h, wd, asym
        sg.kblocked = 1 if isinstance(w, KBlocked) else 0
    a.zeros = zero_page(img0.device).data_ptr()
    assert not (gelu and ksplit > 1)
    _fill_epilogue(a, out, bias, rowbias, rows_per_group, res, 2 if gelu else False)
    keep: list = []
    if lora is not None:
        _lora_fill(a, lora, False, img0.dtype, tuple(w0.shape)[1], keep, lora_sync)
    _fill_colstats(a, colstats_out, keep)
    _fill_split(a, tile, ksplit, ws, stages, table_may_replace_split=table_may_replace_split, operand=out)
    _launch("mi355x_gemm", (C.byref(a),), "mi355x_gemm(conv)", keep=tuple(keep))
    return out


def weight_spans(a: GemmArgs) -> list[tuple[int, int]]:
    """(address, bytes) of the weight operands of a recorded GEMM / conv launch, one per K segment: N rows of ldw elements,
    the last row counted to its K-th element only (the operand may be a column slice of a wider tensor); for a launch
    recorded with weight_operand="x" -- the transposed projections -- M rows of ldx elements."""
    es = 4 if a.dtype == 0 else 2
    out = []
    for s in range(a.nseg):
        sg = a.seg[s]
        k = int(sg.k) * (int(sg.ksize) ** 2 if a.conv else 1)
        if getattr(a, "weight_is_x", False):
            out.append((int(sg.x or 0), (int(a.M) * k if sg.kblocked & 2 else (int(a.M) - 1) * int(sg.ldx) + k) * es))
        else:
            out.append((int(sg.w or 0), (int(a.N) * k if sg.kblocked & 1 else (int(a.N) - 1) * int(sg.ldw) + k) * es))
    return out


def link_weight_prefetch(ops: list, enable: bool = True, min_bytes: int = 1 << 19, bytes_per_block: int = 128 << 10, min_blocks: Optional[int] = None,
                         max_blocks: Optional[int] = None) -> dict:
    """Post-pass over a recorded program that is replayed again and again (a denoising step, an encoder): every GEMM / conv
    launch gets the weight operands of the NEXT GEMM / conv launch as its `prefetch` spans (the last one wraps around to the
    first).  Weights are read exactly once per replay from HBM (5.1 GB per SDXL step), so without this every kernel starts on
    cold lines and its short K loop cannot hide DRAM latency: in place, launches run 25-40 % slower than the same launch on
    hot weights; with the weights pulled into the Infinity Cache one launch ahead the step is 7-8 % shorter
    (tools/probe_prefetch.py, tools/probe_step.py, profiles/r01_t*).  A burst of 32-128 prefetch workgroups at the head of
    the grid beats a thin continuous stream: one workgroup sustains only ~20 GB/s of misses.  Prefetch workgroups per launch: 32 ... 128 by the
    bytes to pull; REFINERS_AMD_PF_BLOCKS="min-max" moves the bounds (an A/B lever: these workgroups sit in front of the launch's own tiles)."""
    import os

    lo, hi = (os.environ.get("REFINERS_AMD_PF_BLOCKS", "").replace("-", ",") + ",").split(",")[:2]  # "min,max" or "min-max" (tools/ab_step.py splits its variants on commas)
    min_blocks = min_blocks if min_blocks is not None else int(lo or 32)
    max_blocks = max(min_blocks, max_blocks if max_blocks is not None else int(hi or 128))
    gemms = [e[1][0]._obj for e in ops if e[0] is not None and e[2].startswith("mi355x_gemm")]
    linked = nbytes_total = 0
    for i, a in enumerate(gemms):
        for s in range(MAX_PREFETCH):
            a.prefetch[s], a.prefetch_bytes[s] = None, 0
        a.prefetch_blocks = 0
        if not enable or len(gemms) < 2:
            continue
        # (round 6 also tried the next launch's LoRA up rows [N, R] in the free second slot -- they sit on the path between a tile's last MFMA and its epilogue --:
        #  25.54 against 25.53 ms, profiles/r06_v_ab_pf_lora.log: all adapters' rows together are ~100 MB and stay in the Infinity Cache from step to step)
        spans = [(p, b) for p, b in weight_spans(gemms[(i + 1) % len(gemms)]) if p and b >= min_bytes][:MAX_PREFETCH]
        if not spans:
            continue
        for s, (p, b) in enumerate(spans):
            a.prefetch[s], a.prefetch_bytes[s] = p, b
        total = sum(b for _, b in spans)
        a.prefetch_blocks = max(min_blocks, min(max_blocks, -(-total // bytes_per_block)))
        linked += 1
        nbytes_total += total
    return {"linked": linked, "bytes": nbytes_total, "launches": len(gemms)}


def gemm_signature(a: GemmArgs) -> str:
    """Shape class of a GEMM / conv launch: the key of the measured tile table (refiners_amd/engine/tuning.py)."""
    k = sum(int(a.seg[s].k) * (int(a.seg[s].ksize) ** 2 if a.conv else 1) for s in range(a.nseg))
    flags = ("geglu" if a.geglu == 1 else "") + ("T%d" % a.nt_begin if a.out_t else "") + ("ln" if a.ln_stats else "") + ("st" if a.stats_out else "") + ("lora" if a.lora_b else "")
    flags += "xa" if getattr(a, "xattn", False) else ""  # the launch is mi355x_gemm_attention: a cross-attention rides in it
    return f"{'conv' if a.conv else 'gemm'}:{'f32' if a.dtype == 0 else 'bf16'}:{a.M}x{a.N}x{k}:s{a.nseg}:{flags}"


def colstats_shape(M: int, N: int) -> tuple[int, int, int]:
    """Shape of the float32 buffer mi355x_gemm_args.colstats_out fills: (sum, sum of squares) per (32-row block, column)."""
    return ((M + 31) // 32, N, 2)


def _fill_colstats(a: GemmArgs, cs: Optional[Tensor], keep: list) -> None:
    if cs is None:
        return
    assert cs.dtype == torch.float32 and cs.is_contiguous() and cs.numel() >= (a.M + 31) // 32 * a.N * 2 and a.N % 16 == 0
    a.colstats_out = cs.data_ptr()
    keep.append(cs)


class StreamK:
    """Scratch of the stream-K launches (tile 8; mi355x_gemm_args.sk_ws / sk_flags): 256 slots of 256 KB + the hand-off flags.  Launches on ONE stream
    share it (a recorded program owns one: Lowering._sk, installed by Lowering._Section while the program is recorded; eager calls use one per
    (operand device, stream): _fill_split); allocated on first use."""

    SLOTS = 256

    def __init__(self, device: torch.device) -> None:
        self.device = device
        self.ws: Optional[Tensor] = None
        self.flags: Optional[Tensor] = None

    def tensors(self) -> tuple[Tensor, Tensor]:
        if self.ws is None:
            self.ws = torch.empty(self.SLOTS * 65536, dtype=torch.float32, device=self.device)
            self.flags = torch.zeros(self.SLOTS + 1, dtype=torch.int32, device=self.device)
        return self.ws, self.flags

    def pending(self) -> Optional[Tensor]:
        """A 0-d bool tensor on the device: a launch reported a lost deposit (None: the scratch was never used).  No host synchronisation."""
        return None if self.flags is None else self.flags[-1] != 0

    def check(self) -> None:
        """Raise if a launch reported a lost deposit.  ALL flags are reset then: an owner that gave up has cleared its range, but a late depositor may
        still have set its flag afterwards, and the next launch on this scratch would find it set at once and add a stale slot (round-5 advisor)."""
        bad = self.pending()
        if bad is not None and bool(bad.item()):
            self.flags.zero_()  # type: ignore[union-attr]
            raise NativeError("mi355x_gemm (stream-K): a workgroup's partial tile never arrived (MI355X_ELAUNCH)")


_streamk_current: Optional[StreamK] = None
_streamk_eager: dict[tuple[int, int], StreamK] = {}


def set_streamk(sk: Optional[StreamK]) -> Optional[StreamK]:
    """Make `sk` the scratch that tile-8 launches made from now on carry (a Lowering installs its own while it records); returns the previous one."""
    global _streamk_current
    old, _streamk_current = _streamk_current, sk
    return old


def attach_streamk(a: GemmArgs, sk: StreamK) -> None:
    w, f = sk.tensors()
    a.sk_ws, a.sk_flags, a.sk_slots = w.data_ptr(), f.data_ptr(), sk.SLOTS
    a._sk_keep = sk


def _fill_split(a: GemmArgs, tile: int, ksplit: int, ws: Optional[Tensor], stages: int = 0, table_may_replace_split: bool = False, operand: Optional[Tensor] = None) -> None:
    """tile / stages / split-K of a launch.  tile == 0 and no split: the measured table of this GPU decides, if it knows the shape.  An EXPLICIT choice
    (tile != 0, or a split) is the caller's and stays (tests and probes of split-K on tabled shapes must run split-K) -- unless the caller says its
    split is only a heuristic (`table_may_replace_split`: Lowering.conv's three-way split for want of tiles): where the table prefers the 8-wave loop
    (engine/tiles.py: whole tiles or stream-K) the launch asks for that tile and KEEPS ksplit / ws: mi355x_gemm drops the split when the 8-wave loop
    takes the launch and runs the split on the 128 x 128 tile when it cannot (unaligned operands, 2 GB and more)."""
    from .engine import tiles, tuning

    if tile == 0 and ksplit <= 1:
        tile, stages = tuning.lookup(gemm_signature(a), stages)
    elif ksplit > 1 and table_may_replace_split:
        t8, _ = tuning.lookup(gemm_signature(a), 0)
        if tiles.takes_whole_k(t8):
            tile = t8
    a.tile, a.ksplit, a.stages = tile, ksplit, stages
    if tiles.needs_streamk_scratch(tile) or tiles.needs_streamk_scratch(int(os.environ.get("REFINERS_AMD_FORCE_TILE") or 0)):
        sk = _streamk_current
        if sk is None:
            # eager call (tests, probes): one scratch per (device of the operands, current stream) -- launches on two streams of one device must not
            # share it, and the current device need not be the operands' (round-5 advisor)
            dev = operand.device if operand is not None and operand.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
            if dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
            key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
            sk = _streamk_eager.get(key)
            if sk is None:
                sk = _streamk_eager[key] = StreamK(dev)
        attach_streamk(a, sk)
    if ksplit > 1:
        assert ws is not None and ws.is_contiguous(), "split-K needs a scratch tensor of ksplit * M * N float32"
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    else:
        a.ws, a.ws_bytes = None, 0


def _fill_epilogue(a: GemmArgs, out: Tensor, bias, rowbias, rows_per_group, res, geglu) -> None:
    assert out.dim() == 2 and out.stride(1) == 1
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    a.bias = bias.data_ptr() if bias is not None else None
    if rowbias is not None:
        assert rowbias.dim() == 2 and rowbias.stride(1) == 1
        a.rowbias, a.ld_rowbias, a.rows_per_group = rowbias.data_ptr(), rowbias.stride(0), rows_per_group
    else:
        a.rowbias, a.ld_rowbias, a.rows_per_group = None, 0, 1
    if res is not None:
        assert res.dim() == 2 and res.stride(1) == 1
        a.res, a.ldres = res.data_ptr(), res.stride(0)
    else:
        a.res, a.ldres = None, 0
    a.geglu = int(geglu)  # 0 none, 1 GEGLU, 2 GELU (erf), 3 quick GELU, 4 ReLU, 5 squared ReLU


def attention(
    q: Tensor,
    out: Tensor,
    num_heads: int,
    streams: Sequence[tuple[Tensor, Tensor, int, float]],
    scale: Optional[float] = None,
) -> Tensor:
    """q, out: [B, Lq, H*D] views (last dim contiguous). streams: (k [B, Lk(+), H*D] view, vt [H*D, B, Lkp] view, Lk, out_scale)."""
    a, _ = attention_args(q, out, num_heads, streams, scale)
    _launch("mi355x_attention", (C.byref(a),), "mi355x_attention")
    return out


def attention_args(q: Optional[Tensor], out: Tensor, num_heads: int, streams: Sequence[tuple[Tensor, Tensor, int, float]], scale: Optional[float] = None) -> tuple:
    """(AttnArgs, the tensors it points to) of mi355x_attention; q = None for gemm(..., attn=): the Q projection's launch produces the queries itself."""
    a = AttnArgs()
    B, Lq, HD = out.shape
    D = HD // num_heads
    a.dtype = dtype_code(out.dtype)
    a.B, a.H, a.D, a.Lq, a.nstream = B, num_heads, D, Lq, len(streams)
    assert out.stride(2) == 1
    if q is not None:
        assert q.stride(2) == 1 and tuple(q.shape) == (B, Lq, HD)
        a.q, a.ldq, a.q_batch_stride = q.data_ptr(), q.stride(1), q.stride(0)
    a.out, a.ldo, a.o_batch_stride = out.data_ptr(), out.stride(1), out.stride(0)
    a.scale = scale if scale is not None else D ** -0.5
    for s, (k, vt, Lk, osc) in enumerate(streams):
        assert k.dim() == 3 and vt.dim() == 3 and k.stride(2) == 1 and vt.stride(2) == 1
        kv = a.kv[s]
        kv.k, kv.ldk, kv.k_batch_stride = k.data_ptr(), k.stride(1), k.stride(0)
        kv.vt, kv.ldvt, kv.vt_batch_stride = vt.data_ptr(), vt.stride(0), vt.stride(1)
        kv.Lk, kv.out_scale = Lk, osc
    return a, (q, out, tuple(streams))


def xattn_tile_ok(M: int, N: int, K: int, dtype: torch.dtype, ln: bool, lora: bool) -> bool:
    """Would mi355x_gemm run this one-segment GEMM on the 64 x 64 tile of the 4-wave loop, the only tile with a cross-attention form?  The measured table's
    entry for the shape class, else the library's heuristic (gemm_kernel.cuh pick_tile: at most 256 tiles of 128 x 128)."""
    from .engine import tuning

    tile, _ = tuning.lookup(f"gemm:{'f32' if dtype == torch.float32 else 'bf16'}:{M}x{N}x{K}:s1:{'ln' if ln else ''}{'lora' if lora else ''}", 0)
    if os.environ.get("REFINERS_AMD_FORCE_TILE"):
        tile = int(os.environ["REFINERS_AMD_FORCE_TILE"])
    return tile == 4 or (tile == 0 and ((M + 127) // 128) * ((N + 127) // 128) <= 256)


def attention_general(
    q: Tensor,
    k: Tensor,
    vt: Tensor,
    out: Tensor,
    num_heads: int,
    Lk: int,
    scale: Optional[float] = None,
    causal: bool = False,
    out_scale: float = 1.0,
) -> Tensor:
    """Head shapes other than 64.  q [B, Lq, H*Dqk], k [B, Lk(+), H*Dqk], vt [H*Dv, B, Lkp] (Lkp = Lk rounded up to 64,
    finite padding), out [B, Lq, H*Dv] -- all views with a contiguous last dimension."""
    a = AttnGeneralArgs()
    B, Lq, HD = q.shape
    assert HD % num_heads == 0 and vt.shape[0] % num_heads == 0 and out.shape[2] == vt.shape[0]
    assert q.stride(2) == 1 and k.stride(2) == 1 and vt.stride(2) == 1 and out.stride(2) == 1
    a.dtype = dtype_code(q.dtype)
    a.B, a.H, a.Lq, a.Lk = B, num_heads, Lq, Lk
    a.Dqk, a.Dv, a.causal = HD // num_heads, vt.shape[0] // num_heads, int(causal)
    a.q, a.ldq, a.q_batch_stride = q.data_ptr(), q.stride(1), q.stride(0)
    a.k, a.ldk, a.k_batch_stride = k.data_ptr(), k.stride(1), k.stride(0)
    a.vt, a.ldvt, a.vt_batch_stride = vt.data_ptr(), vt.stride(0), vt.stride(1)
    a.out, a.ldo, a.o_batch_stride = out.data_ptr(), out.stride(1), out.stride(0)
    a.scale = scale if scale is not None else a.Dqk ** -0.5
    a.out_scale = out_scale
    _launch("mi355x_attention_general", (C.byref(a),), "mi355x_attention_general")
    return out


def attention_joint(q: Tensor, k0: Tensor, vt0: Tensor, Lk0: int, k1: Tensor, vt1: Tensor, Lk1: int, out: Tensor, num_heads: int,
                    mix: Optional[Tensor] = None, scale: Optional[float] = None) -> Tensor:
    """mi355x_attention_joint (csrc/reference_only.hip): out[b] = mix[b] * SDPA(q, [k0 ; k1], [v0 ; v1]) + (1 - mix[b]) * SDPA(q, k0, v0).
    q, out [B, Lq, H*D]; k0 / k1 [B, Lk(+), H*D] (column slices of a wider buffer are fine); vt0 / vt1 [H*D, B, Lkp] with Lkp the segment's Lk
    rounded up to 64 and finite padding -- views with a contiguous last dimension.  mix: float32 [B] on the device, or None (all ones)."""
    a = AttnJointArgs()
    B, Lq, HD = q.shape
    assert HD % num_heads == 0 and vt0.shape[0] == HD and vt1.shape[0] == HD and out.shape[2] == HD
    assert all(t.stride(2) == 1 for t in (q, k0, vt0, k1, vt1, out)) and all(t.dtype == q.dtype for t in (k0, vt0, k1, vt1, out))
    assert vt0.shape[2] >= -(-Lk0 // 64) * 64 and vt1.shape[2] >= -(-Lk1 // 64) * 64 and k0.shape[1] >= Lk0 and k1.shape[1] >= Lk1
    a.dtype = dtype_code(q.dtype)
    a.B, a.H, a.Lq, a.D, a.Lk0, a.Lk1 = B, num_heads, Lq, HD // num_heads, Lk0, Lk1
    a.q, a.ldq, a.q_batch_stride = q.data_ptr(), q.stride(1), q.stride(0)
    a.k0, a.ldk0, a.k0_batch_stride = k0.data_ptr(), k0.stride(1), k0.stride(0)
    a.vt0, a.ldvt0, a.vt0_batch_stride = vt0.data_ptr(), vt0.stride(0), vt0.stride(1)
    a.k1, a.ldk1, a.k1_batch_stride = k1.data_ptr(), k1.stride(1), k1.stride(0)
    a.vt1, a.ldvt1, a.vt1_batch_stride = vt1.data_ptr(), vt1.stride(0), vt1.stride(1)
    if mix is not None:
        assert mix.dtype == torch.float32 and tuple(mix.shape) == (B,) and mix.is_contiguous() and mix.device == q.device
        a.mix = mix.data_ptr()
    a.out, a.ldo, a.o_batch_stride = out.data_ptr(), out.stride(1), out.stride(0)
    a.scale = scale if scale is not None else a.D ** -0.5
    _launch("mi355x_attention_joint", (C.byref(a),), "mi355x_attention_joint", keep=(q, k0, vt0, k1, vt1, mix, out))
    return out


def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, out: Tensor) -> Tensor:
    a = LayerNormArgs()
    assert x.dim() == 2 and out.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1
    a.dtype = dtype_code(x.dtype)
    a.M, a.C = x.shape
    a.x, a.ldx, a.gamma, a.beta, a.eps = x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), eps
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    _launch("mi355x_layernorm", (C.byref(a),), "mi355x_layernorm")
    return out


_gn_ws: "weakref.WeakValueDictionary[tuple[int, int, int], Tensor]" = weakref.WeakValueDictionary()


def groupnorm_nhwc(x: Tensor, gamma: Tensor, beta: Tensor, groups: int, eps: float, silu: bool, out: Tensor, colstats: Optional[Tensor] = None,
                   x2: Optional[Tensor] = None, colstats2: Optional[Tensor] = None) -> Tensor:
    """x, out: [B, HW, C] views with contiguous channels.  `colstats`: what the launch that produced x wrote through `colstats_out`
    ([B * HW / 32, C, 2] float32): the statistics pass over x is skipped.  `x2` [B, HW, C2]: the normalised tensor is the channel concatenation
    (x | x2), which never exists (out has C + C2 channels; `colstats2` then belongs to x2)."""
    a = GroupNormArgs()
    B, HW, C1 = x.shape
    Cc = C1 + (x2.shape[2] if x2 is not None else 0)
    assert x.stride(2) == 1 and out.stride(2) == 1 and x.stride(0) == HW * x.stride(1) and out.stride(0) == HW * out.stride(1) and out.shape[2] == Cc
    if x2 is not None:
        assert x2.shape[:2] == x.shape[:2] and x2.stride(2) == 1 and x2.stride(0) == HW * x2.stride(1) and x2.dtype == x.dtype and (colstats is None) == (colstats2 is None)
        a.x2, a.ldx2, a.C1 = x2.data_ptr(), x2.stride(1), C1
    need = load().mi355x_groupnorm_ws_floats(B, HW, Cc)
    # one scratch per (device, stream) for eager calls, one per PROGRAM while recording: two recorded programs may replay concurrently on two
    # streams (CompiledSDXL's split CFG pair, two trajectories in one process) whatever stream they were lowered on.  The table holds weak
    # references: a program's scratch lives in the keep-alive tuples of its launches and goes with them.
    if x.device.type == "cuda":
        dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
        key = (dev, torch.cuda.current_stream().cuda_stream, id(_recorder) if _recorder is not None else 0)
    else:  # dry-run lowering on the meta / cpu device (tests): nothing is launched
        key = (-1, 0, 0)
    ws = _gn_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1 << 20), dtype=torch.float32, device=x.device)
        _gn_ws[key] = ws
    a.dtype = dtype_code(x.dtype)
    a.B, a.HW, a.C, a.G = B, HW, Cc, groups
    a.x, a.ldx, a.gamma, a.beta, a.eps, a.silu = x.data_ptr(), x.stride(1), gamma.data_ptr(), beta.data_ptr(), eps, int(silu)
    a.out, a.ldo, a.ws = out.data_ptr(), out.stride(1), ws.data_ptr()
    if colstats is not None:
        assert HW % 32 == 0 and colstats.dtype == torch.float32 and colstats.is_contiguous() and colstats.numel() >= B * HW // 32 * C1 * 2
        a.colstats = colstats.data_ptr()
        if colstats2 is not None:
            assert colstats2.dtype == torch.float32 and colstats2.is_contiguous() and colstats2.numel() >= B * HW // 32 * (Cc - C1) * 2
            a.colstats2 = colstats2.data_ptr()
    _launch("mi355x_groupnorm", (C.byref(a),), "mi355x_groupnorm", keep=(ws, colstats, x2, colstats2))
    return out


def nchw_to_nhwc(x: Tensor, out: Tensor) -> Tensor:
    B, Cc, H, W = x.shape
    assert x.is_contiguous() and out.stride(-1) == 1
    _launch("mi355x_nchw_to_nhwc", (dtype_code(x.dtype), x.data_ptr(), out.data_ptr(), B, Cc, H * W, out.stride(-2),), "mi355x_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x: Tensor, out: Tensor, C_: int) -> Tensor:
    """x: [B, HW, ld] rows; out: [B, C, H, W] contiguous."""
    B, HW = x.shape[0], x.shape[1]
    assert out.is_contiguous() and x.stride(-1) == 1
    _launch("mi355x_nhwc_to_nchw", (dtype_code(x.dtype), x.data_ptr(), out.data_ptr(), B, C_, HW, x.stride(1),), "mi355x_nhwc_to_nchw")
    return out


def im2col3x3_nchw(x: Tensor, out: Tensor) -> Tensor:
    B, Cc, H, W = x.shape
    assert x.is_contiguous() and out.dim() == 2 and out.is_contiguous()
    _launch("mi355x_im2col3x3_nchw", (dtype_code(x.dtype), x.data_ptr(), out.data_ptr(), B, Cc, H, W, out.shape[1],), "mi355x_im2col3x3_nchw")
    return out


def concat2(a_: Tensor, b_: Tensor, out: Tensor) -> Tensor:
    """Channel concat of two row-major 2-D tensors [M, C1] ++ [M, C2] -> out [M, C1+C2]."""
    M = a_.shape[0]
    _launch("mi355x_concat2", (dtype_code(a_.dtype), a_.data_ptr(), a_.stride(0), a_.shape[1], b_.data_ptr(), b_.stride(0), b_.shape[1],
                              out.data_ptr(), out.stride(0), M,), "mi355x_concat2")
    return out


def axpby(a_: Tensor, alpha: float, b_: Tensor, beta: float, out: Tensor) -> Tensor:
    assert a_.is_contiguous() and b_.is_contiguous() and out.is_contiguous() and a_.numel() == b_.numel() == out.numel()
    _launch("mi355x_axpby", (dtype_code(a_.dtype), a_.data_ptr(), alpha, b_.data_ptr(), beta, out.data_ptr(), a_.numel(),), "mi355x_axpby")
    return out


def softmax_rows(s: Tensor, out: Tensor, L: int, scale: float) -> Tensor:
    """out[m, :L] = softmax(scale * s[m, :L]), out[m, L:] = 0.  s: float32 [M, >= L] rows; out: [M, Lp] rows of the compute dtype."""
    assert s.dtype == torch.float32 and s.dim() == 2 and out.dim() == 2 and s.stride(1) == 1 and out.stride(1) == 1 and s.shape[0] == out.shape[0]
    assert s.shape[1] >= L and out.shape[1] >= L
    _launch("mi355x_softmax_rows", (dtype_code(out.dtype), s.data_ptr(), s.stride(0), out.data_ptr(), out.stride(0), s.shape[0], L, out.shape[1], scale), "mi355x_softmax_rows")
    return out


def colsum_rows(p: Tensor, acc: Tensor, accumulate: bool, scale: float) -> Tensor:
    """acc[j] (+)= scale * sum_i p[i, j]: p [M, L] rows of the compute dtype, acc float32 [L] (contiguous)."""
    assert p.dim() == 2 and p.stride(1) == 1 and acc.dtype == torch.float32 and acc.is_contiguous() and acc.numel() >= p.shape[1]
    _launch("mi355x_colsum_rows", (dtype_code(p.dtype), p.data_ptr(), p.stride(0), p.shape[0], p.shape[1], acc.data_ptr(), int(accumulate), scale), "mi355x_colsum_rows")
    return acc


def sag_degrade(x: Tensor, eps: Tensor, mass: Tensor, attn_hw: tuple[int, int], coef: Tensor, w1: Tensor, out: Tensor) -> Tensor:
    """Self-attention-guidance degraded latents (see the header): x, eps, out [n, C, h, w]; mass float32 [n, ah*aw]; coef device row; w1 float32 [k]."""
    n, Cc, h, w = x.shape
    assert x.is_contiguous() and eps.is_contiguous() and out.is_contiguous() and eps.shape == x.shape == out.shape and x.dtype == eps.dtype == out.dtype
    assert mass.dtype == torch.float32 and mass.is_contiguous() and mass.numel() == n * attn_hw[0] * attn_hw[1] and w1.dtype == torch.float32 and w1.is_contiguous()
    _launch("mi355x_sag_degrade", (dtype_code(x.dtype), x.data_ptr(), eps.data_ptr(), mass.data_ptr(), attn_hw[0], attn_hw[1], coef.data_ptr(), w1.data_ptr(), w1.numel(),
                                   out.data_ptr(), n, Cc, h, w), "mi355x_sag_degrade", keep=(mass, w1, coef))
    return out


def silu(x: Tensor, out: Tensor) -> Tensor:
    assert x.is_contiguous() and out.is_contiguous()
    _launch("mi355x_silu", (dtype_code(x.dtype), x.data_ptr(), out.data_ptr(), x.numel(),), "mi355x_silu")
    return out


_NO = object()  # an operand the entry point's prototype does not have (None is an operand passed as NULL)


def _solver_step(sym: str, rows: int, ncoef: int, x: Tensor, unet_out: Tensor, hist: Any, noise: Any, model_in: Any, coef: Tensor) -> Tensor:
    """The launch behind the six solver-step wrappers below (csrc/solver_step.hip): x, hist, noise have n elements, unet_out and model_in
    rows * n (rows = 2: the CFG pair); model_in may be None; coef: at least `ncoef` float32 on the device."""
    ops = [t for t in (hist, noise) if t is not _NO]
    assert x.is_contiguous() and unet_out.is_contiguous() and all(t.is_contiguous() for t in ops) and rows in (1, 2)
    assert unet_out.numel() == rows * x.numel() and all(t.numel() == x.numel() for t in ops)
    assert unet_out.dtype == x.dtype and all(t.dtype == x.dtype for t in ops)
    assert coef.dtype == torch.float32 and coef.numel() >= ncoef and coef.is_cuda
    assert model_in is _NO or model_in is None or (
        model_in.is_contiguous() and model_in.numel() == rows * x.numel() and model_in.dtype == x.dtype and model_in.data_ptr() != x.data_ptr())
    ptrs = [None if t is None else t.data_ptr() for t in (hist, noise, model_in) if t is not _NO]
    _launch(sym, (dtype_code(x.dtype), x.data_ptr(), unet_out.data_ptr(), *ptrs, coef.data_ptr(), x.numel()), sym, keep=() if noise is _NO else (noise,))
    return x


def cfg_ddim_step(x: Tensor, unet_out: Tensor, coef: Tensor) -> Tensor:
    """In-place: x <- ddim(x, cfg(unet_out)). unet_out = [uncond; cond] (2*x.numel() elements); coef: f32[5] on device."""
    return _solver_step("mi355x_cfg_ddim_step", 2, 5, x, unet_out, _NO, _NO, _NO, coef)


def cfg_linear_step(x: Tensor, unet_out: Tensor, hist: Tensor, model_in: Optional[Tensor], coef: Tensor) -> Tensor:
    """x, hist: [N, ...] latents (in place); unet_out: [2N, ...] = (unconditional, conditional); model_in: [2N, ...] or None;
    coef: 8 float32 on the device = (cfg, hx, he, kx, ke, kd, kp, s_next) -- see mi355x_cfg_linear_step in the header."""
    return _solver_step("mi355x_cfg_linear_step", 2, 8, x, unet_out, hist, _NO, model_in, coef)


def ddim_step(x: Tensor, unet_out: Tensor, model_in: Optional[Tensor], coef: Tensor) -> Tensor:
    """Guidance-free DDIM update, in place: x <- ddim(x, unet_out); model_in (x's shape, or None) <- the new x, the next step's model input.
    coef: the 8-float row of cfg_ddim_step on the device (coef[0], the guidance scale, is not read) -- see mi355x_ddim_step in its header."""
    return _solver_step("mi355x_ddim_step", 1, 5, x, unet_out, _NO, _NO, model_in, coef)


def linear_step(x: Tensor, unet_out: Tensor, hist: Tensor, model_in: Optional[Tensor], coef: Tensor) -> Tensor:
    """Guidance-free form of cfg_linear_step: x, hist, unet_out and model_in (or None) all have x's n elements; coef: 8 float32 on the device =
    (-, hx, he, kx, ke, kd, kp, s_next) -- see mi355x_linear_step in its header."""
    return _solver_step("mi355x_linear_step", 1, 8, x, unet_out, hist, _NO, model_in, coef)


def cfg_sde_step(x: Tensor, unet_out: Tensor, hist: Tensor, noise: Tensor, model_in: Optional[Tensor], coef: Tensor) -> Tensor:
    """cfg_linear_step with the step's Gaussian draw as a fifth operand (SDE DPM-Solver++): x, hist [N, ...] in place; noise [N, ...] read only;
    unet_out [2N, ...]; model_in [2N, ...] or None; coef: 9 float32 on the device = (cfg, hx, he, kx, ke, kd, kp, s_next, kn) -- see
    mi355x_cfg_sde_step in its header."""
    return _solver_step("mi355x_cfg_sde_step", 2, 9, x, unet_out, hist, noise, model_in, coef)


def sde_step(x: Tensor, unet_out: Tensor, hist: Tensor, noise: Tensor, model_in: Optional[Tensor], coef: Tensor) -> Tensor:
    """Guidance-free form of cfg_sde_step: unet_out and model_in (or None) have x's n elements; coef[0] is not read -- see mi355x_sde_step."""
    return _solver_step("mi355x_sde_step", 1, 9, x, unet_out, hist, noise, model_in, coef)


def _cond_geometry(x_like: tuple, model_in: Tensor, cond: Optional[Tensor]) -> tuple[int, int, int, int, int]:
    """(n, C, E, nc, hw) of latents [n, C, h, w], a model input [n or 2n, C + E, h, w] and constants [1 or n, E, h, w] (or None)."""
    n, Cc, h, w = x_like
    assert model_in.dim() == 4 and model_in.is_contiguous() and tuple(model_in.shape[2:]) == (h, w) and model_in.shape[1] >= Cc
    E = model_in.shape[1] - Cc
    nc = 1
    if cond is not None:
        assert cond.is_contiguous() and cond.dtype == model_in.dtype and tuple(cond.shape[1:]) == (E, h, w) and cond.shape[0] in (1, n), (tuple(cond.shape), (n, E, h, w))
        nc = cond.shape[0]
    return n, Cc, E, nc, h * w


def cond_step(x: Tensor, unet_out: Tensor, hist: Optional[Tensor], model_in: Tensor, cond: Optional[Tensor], coef: Tensor, linear: bool, guided: bool) -> Tensor:
    """The step's last launch of a UNet with step-constant input channels (see mi355x_cond_step in its header): x, hist [n, C, h, w] in place;
    unet_out [2n or n, C, h, w]; model_in [2n or n, C + E, h, w]; cond [1 or n, E, h, w], or None to leave the constant channels as they are."""
    n, Cc, E, nc, hw = _cond_geometry(tuple(x.shape), model_in, cond)
    B = 2 * n if guided else n
    assert x.is_contiguous() and unet_out.is_contiguous() and tuple(unet_out.shape) == (B,) + tuple(x.shape[1:]) and model_in.shape[0] == B
    assert unet_out.dtype == x.dtype == model_in.dtype and coef.dtype == torch.float32 and coef.numel() >= 8
    assert not linear or (hist is not None and hist.is_contiguous() and hist.shape == x.shape and hist.dtype == x.dtype)
    _launch("mi355x_cond_step", (dtype_code(x.dtype), ABIS["cond_input"].constants["MI355X_COND_LINEAR" if linear else "MI355X_COND_DDIM"], int(guided), x.data_ptr(),
                                unet_out.data_ptr(), hist.data_ptr() if (linear and hist is not None) else None, model_in.data_ptr(),
                                cond.data_ptr() if cond is not None else None, coef.data_ptr(), n, Cc, E, nc, hw), "mi355x_cond_step", keep=(cond,))
    return x


def cond_fill(x: Optional[Tensor], cond: Optional[Tensor], model_in: Tensor, s: Optional[Tensor], n: int, channels: int) -> Tensor:
    """model_in[b, :channels] = s x[b % n] (x given) and model_in[b, channels:] = s cond[0 or b % n] (cond given) for every row b of model_in
    [n or 2n, channels + E, h, w]; s: one float32 on the device, None = 1 (see mi355x_cond_fill in its header)."""
    h, w = model_in.shape[2:]
    n, Cc, E, nc, hw = _cond_geometry((n, channels, h, w), model_in, cond)
    assert x is None or (x.is_contiguous() and tuple(x.shape) == (n, Cc, h, w) and x.dtype == model_in.dtype)
    assert s is None or (s.dtype == torch.float32 and s.numel() >= 1 and s.is_cuda)
    _launch("mi355x_cond_fill", (dtype_code(model_in.dtype), x.data_ptr() if x is not None else None, cond.data_ptr() if cond is not None else None, model_in.data_ptr(),
                                s.data_ptr() if s is not None else None, n, model_in.shape[0], Cc, E, nc, hw), "mi355x_cond_fill", keep=(x, cond, s))
    return model_in


def inpaint_conditions(image: Tensor, mask: Tensor, masked_image: Tensor, mask_latents: Tensor) -> tuple[Tensor, Tensor]:
    """image uint8 [n, H, W, 3], mask uint8 [1 or n, H, W] -> masked_image [n, 3, H, W] and mask_latents [1 or n, 1, h, w] in the model dtype
    (see mi355x_inpaint_conditions in its header)."""
    n, H, W, three = image.shape
    nm = mask.shape[0]
    assert three == 3 and image.dtype == torch.uint8 and mask.dtype == torch.uint8 and image.is_contiguous() and mask.is_contiguous()
    assert tuple(mask.shape) == (nm, H, W) and nm in (1, n) and tuple(masked_image.shape) == (n, 3, H, W) and masked_image.is_contiguous()
    assert mask_latents.dim() == 4 and tuple(mask_latents.shape[:2]) == (nm, 1) and mask_latents.is_contiguous() and mask_latents.dtype == masked_image.dtype
    _launch("mi355x_inpaint_conditions", (dtype_code(masked_image.dtype), image.data_ptr(), mask.data_ptr(), masked_image.data_ptr(), mask_latents.data_ptr(), n, nm, H, W,
                                         mask_latents.shape[2], mask_latents.shape[3]), "mi355x_inpaint_conditions", keep=(image, mask))
    return masked_image, mask_latents


def sinusoidal(x: Tensor, dim: int, out: Tensor, group: int = 1, col0: int = 0) -> Tensor:
    """x: float32 values (any shape, contiguous); out: 2-D [x.numel() / group, >= col0 + group * dim] rows of the compute dtype."""
    assert x.dtype == torch.float32 and x.is_contiguous() and out.dim() == 2 and out.stride(1) == 1
    assert x.numel() % group == 0 and out.shape[0] >= x.numel() // group and out.shape[1] >= col0 + group * dim
    _launch("mi355x_sinusoidal", (dtype_code(out.dtype), x.data_ptr(), x.numel(), dim, group, out.data_ptr(), out.stride(0), col0), "mi355x_sinusoidal")
    return out


def patchify_nchw(x: Tensor, patch: int, out: Tensor) -> Tensor:
    """x: [B, C, H, W] contiguous; out: [B * (H/P) * (W/P), >= C*P*P] rows."""
    B, Cc, H, W = x.shape
    assert x.is_contiguous() and out.dim() == 2 and out.stride(1) == 1 and out.shape[1] >= Cc * patch * patch
    _launch("mi355x_patchify_nchw", (dtype_code(x.dtype), x.data_ptr(), out.data_ptr(), B, Cc, H, W, patch, out.stride(0)), "mi355x_patchify_nchw")
    return out


def gather_rows(x: Tensor, idx: Tensor, out: Tensor) -> Tensor:
    """out[i] = x[idx[i]] (zero row where idx[i] < 0); x, out: 2-D with unit column stride; idx: int32 on the device."""
    assert x.dim() == 2 and out.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1 and x.shape[1] == out.shape[1]
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == out.shape[0]
    _launch("mi355x_gather_rows", (dtype_code(x.dtype), x.data_ptr(), x.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0), out.shape[0], x.shape[1]),
            "mi355x_gather_rows", keep=(idx,))
    return out


def relpos_pack(src: Tensor, out: Tensor, heads: int, d: int, S1: int, S2: int, Lp: int, Dq: int) -> Tensor:
    """src [M, heads*Lp] -> out [M, heads*Dq]: the per-token windows of the folded relative-position products (see the header)."""
    assert src.dim() == 2 and out.dim() == 2 and src.stride(1) == 1 and out.stride(1) == 1 and src.shape[0] == out.shape[0]
    assert src.shape[1] >= heads * Lp and out.shape[1] >= heads * Dq
    _launch("mi355x_relpos_pack", (dtype_code(src.dtype), src.data_ptr(), src.stride(0), out.data_ptr(), out.stride(0), src.shape[0], heads, d, S1, S2, Lp, Dq),
            "mi355x_relpos_pack")
    return out


def pointwise_nchw(x: Tensor, w: Tensor, bias: Optional[Tensor], out: Tensor) -> Tensor:
    """1x1 conv of a few-channel NCHW image: x [B, Ci, H, W], w [Co, Ci], out [B, Co, H, W] (all contiguous)."""
    B, Ci, H, W = x.shape
    assert x.is_contiguous() and out.is_contiguous() and w.is_contiguous() and tuple(w.shape) == (out.shape[1], Ci)
    _launch("mi355x_pointwise_nchw", (dtype_code(x.dtype), x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(),
                                      B, Ci, out.shape[1], H * W), "mi355x_pointwise_nchw")
    return out



# ------------------------------------------------------------------------------------------------ SAM mask decoder (csrc/sam_decoder.hip)
def sam_attention_ws_floats(B: int, H: int, D: int, Lq: int, Lk: int) -> int:
    """Floats of the workspace mi355x_sam_attention needs (0 in the short-key regime)."""
    return 0 if Lk <= 64 else B * H * ((Lk + 255) // 256) * Lq * (D + 2)


def sam_attention(q: Tensor, k: Tensor, v: Tensor, out: Tensor, num_heads: int, ws: Optional[Tensor] = None, scale: Optional[float] = None) -> Tensor:
    """q [B|1, Lq, >= H*D], k / v [B|1, Lk, >= H*D], out [B, Lq, >= H*D]: 3-D views with a contiguous last dimension; a leading size of 1
    (or a batch stride of 0) shares that operand across the batch.  ws: float32 workspace of sam_attention_ws_floats(...) elements."""
    B, Lq = out.shape[0], out.shape[1]
    Lk = k.shape[1]
    D = out.shape[2] // num_heads if q.shape[2] == out.shape[2] else q.shape[2] // num_heads
    assert D in (16, 32), f"head width {D}: mi355x_sam_attention takes D = 16 or 32"
    for t in (q, k, v, out):
        assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == out.dtype
        assert t.shape[2] >= num_heads * D, f"a view of {t.shape[2]} columns for {num_heads} heads of {D}: the kernel would read past it"
    assert q.shape[1] == Lq and v.shape[1] == Lk and q.shape[0] in (1, B) and k.shape[0] in (1, B) and v.shape[0] in (1, B)
    bs = lambda t: 0 if t.shape[0] == 1 else t.stride(0)  # noqa: E731
    a = SamAttnArgs()
    a.dtype = dtype_code(out.dtype)
    a.B, a.H, a.D, a.Lq, a.Lk = B, num_heads, D, Lq, Lk
    a.q, a.ldq, a.q_batch_stride = q.data_ptr(), q.stride(1), bs(q)
    a.k, a.ldk, a.k_batch_stride = k.data_ptr(), k.stride(1), bs(k)
    a.v, a.ldv, a.v_batch_stride = v.data_ptr(), v.stride(1), bs(v)
    a.out, a.ldo, a.o_batch_stride = out.data_ptr(), out.stride(1), out.stride(0)
    a.scale = scale if scale is not None else D ** -0.5
    need = sam_attention_ws_floats(B, num_heads, D, Lq, Lk)
    if need:
        assert ws is not None and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= need
        a.ws, a.ws_floats = ws.data_ptr(), ws.numel()
    _launch("mi355x_sam_attention", (C.byref(a),), "mi355x_sam_attention", keep=(ws,))
    return out


def convt2x2_ln_gelu(x: Tensor, C_: int, G: int, gamma: Tensor, beta: Tensor, eps: float, out: Tensor, scatter_hw: Optional[tuple[int, int]] = None) -> Tensor:
    """LayerNorm2d + GELU over G groups of C_ channels of each row of x [M, >= G*C_]; scatter_hw = (Hs, Ws): group (dy, dx) of pixel
    (p, y, x) goes to row (p, 2y + dy, 2x + dx) of out (the NHWC upsampled image), else to out[m, g*C_ : (g+1)*C_]."""
    assert x.dim() == 2 and out.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1 and x.dtype == out.dtype
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C_ == beta.numel()
    M = x.shape[0]
    Hs, Ws = scatter_hw or (0, 0)
    assert out.shape[0] == (4 * M if scatter_hw else M) and out.shape[1] >= (C_ if scatter_hw else G * C_)
    _launch("mi355x_convt2x2_ln_gelu", (dtype_code(x.dtype), x.data_ptr(), x.stride(0), M, C_, G, gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(),
                                       out.stride(0), Hs, Ws), "mi355x_convt2x2_ln_gelu", keep=(gamma, beta))
    return out


def sam_mask_head(x: Tensor, P: int, Hin: int, Win: int, w: Tensor, bias: Tensor, hyper: Tensor, out: Tensor) -> Tensor:
    """x [P*Hin*Win, >= 64] NHWC rows; w float32 [64, 128]; bias float32 [32]; hyper [P, nk, >= 32] (a view); out [P, nk, 2Hin, 2Win]."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == P * Hin * Win and x.shape[1] >= 64 and w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (64, 128)
    assert bias.dtype == torch.float32 and bias.numel() == 32 and hyper.dim() == 3 and hyper.stride(2) == 1 and hyper.shape[0] == P
    nk = hyper.shape[1]
    assert out.dim() == 4 and tuple(out.shape[1:]) == (nk, 2 * Hin, 2 * Win) and out.stride(3) == 1 and out.stride(2) == 2 * Win and out.stride(1) == 4 * Hin * Win
    a = SamMaskHeadArgs()
    a.dtype = dtype_code(x.dtype)
    a.P, a.Hin, a.Win, a.nk = P, Hin, Win, nk
    a.x, a.ldx, a.w, a.bias = x.data_ptr(), x.stride(0), w.data_ptr(), bias.data_ptr()
    a.hyper, a.ld_hyper, a.hyper_batch_stride = hyper.data_ptr(), hyper.stride(1), hyper.stride(0)
    a.out, a.out_batch_stride = out.data_ptr(), out.stride(0)
    _launch("mi355x_sam_mask_head", (C.byref(a),), "mi355x_sam_mask_head", keep=(w, bias))
    return out


def sam_postprocess_masks(low: Tensor, R: int, scaled: tuple[int, int], out: Tensor, threshold: Optional[float] = None) -> Tensor:
    """low [..., Hin, Win] (contiguous planes) -> out [..., H, W]: of low's dtype, or uint8 / bool (low > threshold) when threshold is given."""
    assert low.is_contiguous() and out.is_contiguous() and low.shape[:-2] == out.shape[:-2]
    a = SamPostprocessArgs()
    a.dtype = dtype_code(low.dtype)
    a.Hin, a.Win = low.shape[-2], low.shape[-1]
    a.N = low.numel() // (a.Hin * a.Win)
    a.R, a.sh, a.sw, a.H, a.W = R, scaled[0], scaled[1], out.shape[-2], out.shape[-1]
    a.in_, a.in_plane_stride, a.out = low.data_ptr(), a.Hin * a.Win, out.data_ptr()
    if threshold is None:
        assert out.dtype == low.dtype
        a.binarize, a.threshold = 0, 0.0
    else:
        assert out.dtype in (torch.uint8, torch.bool)
        a.binarize, a.threshold = 1, float(threshold)
    _launch("mi355x_sam_postprocess_masks", (C.byref(a),), "mi355x_sam_postprocess_masks")
    return out


# ------------------------------------------------------------------------------------------------ Swin window attention (csrc/window_attention.hip)
def window_attention(q: Tensor, k: Tensor, v: Tensor, table: Tensor, out: Tensor, num_heads: int, window_size: int, nw: int = 0, shift: int = 0,
                     scale: Optional[float] = None) -> Tensor:
    """q, k, v: [nW, N, H * 32] views (N = window_size^2, unit channel stride; normally three column views of the packed QKV rows);
    table: float32 [(2 ws - 1)^2, H], the tree's own parameter; out: [nW, N, H * 32] view.  shift > 0: the windows tile grids of nw x nw
    windows rolled by -shift and the -100 shift mask is added (see the header)."""
    a = WindowAttentionArgs()
    nW, N, HD = q.shape
    assert HD == num_heads * 32 and N == window_size * window_size and tuple(k.shape) == tuple(q.shape) == tuple(v.shape) == tuple(out.shape)
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1 and out.stride(2) == 1 and k.dtype == q.dtype == v.dtype == out.dtype
    assert table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == ((2 * window_size - 1) ** 2, num_heads)
    a.dtype = dtype_code(q.dtype)
    a.nW, a.H, a.ws, a.nw, a.shift = nW, num_heads, window_size, nw, shift
    a.q, a.ldq, a.q_win_stride = q.data_ptr(), q.stride(1), q.stride(0)
    a.k, a.ldk, a.k_win_stride = k.data_ptr(), k.stride(1), k.stride(0)
    a.v, a.ldv, a.v_win_stride = v.data_ptr(), v.stride(1), v.stride(0)
    a.table, a.scale = table.data_ptr(), scale if scale is not None else 32 ** -0.5
    a.out, a.ldo, a.o_win_stride = out.data_ptr(), out.stride(1), out.stride(0)
    _launch("mi355x_window_attention", (C.byref(a),), "mi355x_window_attention", keep=(table,))
    return out


# ------------------------------------------------------------------------------------------------ MVANet's decoder (csrc/mvanet.hip)
MVANET_MAX_RATIOS = ABIS["mvanet"].constants["MI355X_MVANET_MAX_RATIOS"]


def mvanet_pool_rows(G: int, ratios: Sequence[int]) -> int:
    """Rows MultiPool writes for a G x G map."""
    return sum((G // r) ** 2 for r in ratios)


def mvanet_pool(src: Tensor, S: int, ratios: Sequence[int], out: Tensor, split: bool) -> Tensor:
    """MultiPool as token rows.  split=False: src [4 S S, E] = four views, pooled as their PatchMerge (side 2 S), out [rows, E].  split=True:
    src [S S, E] = one view, out [4, rows, E]: group q pools quadrant q (PatchSplit).  Rows past the pooled ones are written as zeros."""
    a = MvanetPoolArgs()
    assert src.dim() == 2 and src.stride(1) == 1 and out.stride(-1) == 1 and out.shape[-1] == src.shape[1] and out.dtype == src.dtype
    assert src.shape[0] == (1 if split else 4) * S * S and out.dim() == (3 if split else 2) and (not split or out.shape[0] == 4) and len(ratios) <= MVANET_MAX_RATIOS
    a.dtype, a.mode, a.S, a.E, a.n_ratios = dtype_code(src.dtype), int(split), S, src.shape[1], len(ratios)
    for i, r in enumerate(ratios):
        a.ratio[i] = r
    a.src, a.lds, a.out, a.ldo, a.rows = src.data_ptr(), src.stride(0), out.data_ptr(), out.stride(-2), out.shape[-2]
    a.group_stride = out.stride(0) if split else 0
    _launch("mi355x_mvanet_pool", (C.byref(a),), "mi355x_mvanet_pool")
    return out


def mvanet_gate(local: Tensor, glb: Tensor, w: Tensor, b: Tensor, out: Tensor, S: int) -> Tensor:
    """out = local * sigmoid(w . glb + b), the gate map upsampled 2x (nearest) and split into quadrants.  local, out: [4 S S, E] (out may be
    local); glb: [S S, E]; w [E], b [1]: the activations' dtype, read at every launch."""
    a = MvanetGateArgs()
    E = local.shape[1]
    assert tuple(local.shape) == tuple(out.shape) == (4 * S * S, E) and tuple(glb.shape) == (S * S, E) and local.stride(1) == glb.stride(1) == out.stride(1) == 1
    assert w.dtype == b.dtype == glb.dtype == out.dtype == local.dtype and w.is_contiguous() and w.numel() == E and b.numel() == 1
    a.dtype, a.S, a.E = dtype_code(local.dtype), S, E
    a.local, a.ldl, a.glb, a.ldg, a.w, a.b, a.out, a.ldo = local.data_ptr(), local.stride(0), glb.data_ptr(), glb.stride(0), w.data_ptr(), b.data_ptr(), out.data_ptr(), out.stride(0)
    _launch("mi355x_mvanet_gate", (C.byref(a),), "mi355x_mvanet_gate", keep=(w, b))
    return out


def mvanet_resize_add(x: Tensor, x_hw: tuple[int, int], y: Tensor, out: Tensor, out_hw: tuple[int, int], B: int = 1, mode: str = "bilinear",
                      slope_x: Optional[Tensor] = None, slope_y: Optional[Tensor] = None, x_merge: bool = False, y_merge: bool = False) -> Tensor:
    """out = resize(f(x)) + g(y): x [B Hx Wx, E] resized to out_hw (torch's bilinear with align_corners=False, or nearest), y, out [B Ho Wo, E]; f / g =
    PReLU with the one-element device tensor slope_x / slope_y, identity when None.  *_merge: the operand is four views read as their PatchMerge.
    out may be y."""
    a = MvanetResizeAddArgs()
    E = out.shape[1]
    (Ha, Wa), (Ho, Wo) = x_hw, out_hw
    assert tuple(x.shape) == (B * Ha * Wa, E) and tuple(y.shape) == tuple(out.shape) == (B * Ho * Wo, E) and x.stride(1) == y.stride(1) == out.stride(1) == 1
    assert x.dtype == y.dtype == out.dtype and all(s is None or (s.dtype == out.dtype and s.numel() == 1) for s in (slope_x, slope_y)) and mode in ("bilinear", "nearest")
    a.dtype, a.mode, a.B, a.E = dtype_code(out.dtype), int(mode == "nearest"), B, E
    a.Ha, a.Wa, a.Ho, a.Wo, a.a_merge, a.b_merge = Ha, Wa, Ho, Wo, int(x_merge), int(y_merge)
    a.a, a.lda, a.b, a.ldb, a.out, a.ldo = x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), out.data_ptr(), out.stride(0)
    a.slope_a = slope_x.data_ptr() if slope_x is not None else None
    a.slope_b = slope_y.data_ptr() if slope_y is not None else None
    _launch("mi355x_mvanet_resize_add", (C.byref(a),), "mi355x_mvanet_resize_add", keep=(slope_x, slope_y))
    return out


def mvanet_prelu(x: Tensor, slope: Tensor) -> Tensor:
    """In-place PReLU of a contiguous tensor with the one-element device tensor `slope` (read at every launch)."""
    assert x.is_contiguous() and slope.dtype == x.dtype and slope.numel() == 1
    _launch("mi355x_mvanet_prelu", (dtype_code(x.dtype), x.data_ptr(), slope.data_ptr(), x.numel()), "mi355x_mvanet_prelu", keep=(slope,))
    return x


def mvanet_split_views(image: Tensor, out: Tensor) -> Tensor:
    """SplitMultiView: image [1, C, H, W] -> out [5, C, H / 2, W / 2], the four quadrants and the 2 x 2 block means (bilinear 0.5x)."""
    _one, Cc, H, W = image.shape
    assert _one == 1 and image.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (5, Cc, H // 2, W // 2) and out.dtype == image.dtype
    _launch("mi355x_mvanet_split_views", (dtype_code(image.dtype), image.data_ptr(), out.data_ptr(), Cc, H, W), "mi355x_mvanet_split_views")
    return out


# ------------------------------------------------------------------------------------------------ DINOv2's encoder (csrc/dinov2.hip)
class Dinov2Axis:
    """The tap table of one axis of mi355x_dinov2_pos_resample: per output index the first source index, the tap count and the offset of its
    first weight in `weight` (int32 [n_out] each, float32 [len]).  Built and CHECKED on the host (the kernel reads the device copy and the
    entry point cannot see it), then copied to `device`."""

    def __init__(self, first: Tensor, count: Tensor, offset: Tensor, weight: Tensor, n_src: int, device: Any = "cpu") -> None:
        first, count, offset = (t.to(torch.int32).contiguous() for t in (first, count, offset))
        weight = weight.to(torch.float32).contiguous()
        assert first.dim() == count.dim() == offset.dim() == weight.dim() == 1 and first.numel() == count.numel() == offset.numel() >= 1 and weight.numel() >= 1
        assert bool((count >= 1).all()) and bool((first >= 0).all()) and bool((first + count <= n_src).all()), "taps outside the source axis"
        assert bool((offset >= 0).all()) and bool((offset + count <= weight.numel()).all()), "taps outside the weight list"
        self.n_src, self.n_out = n_src, first.numel()
        self.host = (first, count, offset, weight)
        self.dev = tuple(t.to(device) for t in self.host)


def dinov2_pos_resample(src: Tensor, ty: Dinov2Axis, tx: Dinov2Axis, out: Tensor) -> Tensor:
    """out [h * w, D] float32 = the separable filter (ty, tx) over src [Hs * Ws, D] (rows of the learned position grid, channels-last)."""
    a = Dinov2PosResampleArgs()
    D = src.shape[1]
    assert src.dim() == 2 and out.dim() == 2 and src.stride(1) == 1 and out.stride(1) == 1 and out.dtype == torch.float32
    assert tuple(src.shape) == (ty.n_src * tx.n_src, D) and tuple(out.shape) == (ty.n_out * tx.n_out, D)
    assert all(t.device == src.device for t in ty.dev + tx.dev), "tap tables on another device"
    a.dtype, a.Hs, a.Ws, a.h, a.w, a.D = dtype_code(src.dtype), ty.n_src, tx.n_src, ty.n_out, tx.n_out, D
    a.src, a.lds, a.out, a.ldo = src.data_ptr(), src.stride(0), out.data_ptr(), out.stride(0)
    a.y0, a.ny, a.wy_off, a.wy = (t.data_ptr() for t in ty.dev)
    a.x0, a.nx, a.wx_off, a.wx = (t.data_ptr() for t in tx.dev)
    a.wy_len, a.wx_len = ty.dev[3].numel(), tx.dev[3].numel()
    _launch("mi355x_dinov2_pos_resample", (C.byref(a),), "mi355x_dinov2_pos_resample", keep=(src, ty, tx, out))
    return out


def dinov2_tokens(patch: Tensor, pos: Tensor, cls: Tensor, pos0: Tensor, reg: Optional[Tensor], out: Tensor, B: int, rows: Optional[int] = None) -> Tensor:
    """out [B * rows, D]: per image the class row (cls + pos0), the register rows (reg [R, D] or None), the n patch rows + pos [n, D] (float32),
    then zero rows up to `rows` (default 1 + R + n).  patch [B * n, D]."""
    a = Dinov2TokensArgs()
    D = patch.shape[1]
    n, R = pos.shape[0], 0 if reg is None else reg.shape[0]
    rows = rows if rows is not None else 1 + R + n
    assert patch.dim() == 2 and patch.shape[0] == B * n and tuple(pos.shape) == (n, D) and pos.dtype == torch.float32 and tuple(out.shape) == (B * rows, D) and rows >= 1 + R + n
    assert patch.stride(1) == pos.stride(1) == out.stride(1) == 1 and cls.numel() == pos0.numel() == D and cls.is_contiguous() and pos0.is_contiguous()
    assert patch.dtype == cls.dtype == pos0.dtype == out.dtype and (reg is None or (reg.dtype == out.dtype and reg.shape[1] == D and reg.stride(1) == 1))
    a.dtype, a.B, a.n, a.R, a.D, a.rows = dtype_code(out.dtype), B, n, R, D, rows
    a.patch, a.ldp, a.pos, a.ldpos, a.cls, a.pos0 = patch.data_ptr(), patch.stride(0), pos.data_ptr(), pos.stride(0), cls.data_ptr(), pos0.data_ptr()
    a.reg, a.ldr = (reg.data_ptr(), reg.stride(0)) if reg is not None else (None, 0)
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    _launch("mi355x_dinov2_tokens", (C.byref(a),), "mi355x_dinov2_tokens", keep=(pos, cls, pos0, reg))
    return out


# ------------------------------------------------------------------------------------------------ ELLA's resampler (csrc/ella.hip)
def ella_adaln(latents: Tensor, shift_l: Tensor, scale_l: Tensor, out: Tensor, x: Optional[Tensor] = None, shift_x: Optional[Tensor] = None,
               scale_x: Optional[Tensor] = None, eps: float = 1e-6) -> Tensor:
    """mi355x_ella_adaln: out [B, Lp, C] <- [LN0(latents) * (1 + scale_l) + shift_l ; LN0(x) * (1 + scale_x) + shift_x ; zero rows].
    latents [B, Nl, C], x [B, T, C] or None (the feed-forward form), out [B, Lp >= Nl + T, C]: 3-D views with a contiguous last dimension.
    shift_* / scale_* [B, C]: 2-D views of one row stride (column slices of the time table)."""
    a = EllaAdaLnArgs()
    B, Nl, C_ = latents.shape
    T = 0 if x is None else x.shape[1]
    mods = [shift_l, scale_l] + ([shift_x, scale_x] if T else [])
    assert out.dim() == 3 and out.shape[0] == B and out.shape[2] == C_ and latents.stride(2) == 1 and out.stride(2) == 1
    assert all(m is not None and tuple(m.shape) == (B, C_) and m.stride(1) == 1 and m.stride(0) == shift_l.stride(0) and m.dtype == latents.dtype for m in mods)
    a.dtype = dtype_code(latents.dtype)
    a.B, a.Nl, a.T, a.Lp, a.C = B, Nl, T, out.shape[1], C_
    a.latents, a.ldl, a.l_batch_stride = latents.data_ptr(), latents.stride(1), latents.stride(0)
    if T:
        assert x.dim() == 3 and x.shape[0] == B and x.shape[2] == C_ and x.stride(2) == 1 and x.dtype == latents.dtype
        a.x, a.ldx, a.x_batch_stride = x.data_ptr(), x.stride(1), x.stride(0)
        a.shift_x, a.scale_x = shift_x.data_ptr(), scale_x.data_ptr()
    a.shift_l, a.scale_l, a.mod_batch_stride, a.eps = shift_l.data_ptr(), scale_l.data_ptr(), shift_l.stride(0), eps
    a.out, a.ldo, a.out_batch_stride = out.data_ptr(), out.stride(1), out.stride(0)
    _launch("mi355x_ella_adaln", (C.byref(a),), "mi355x_ella_adaln", keep=(latents, x, shift_l, scale_l, shift_x, scale_x, out))
    return out


def glu_silu(x: Tensor, out: Tensor) -> Tensor:
    """out [M, F] = x[:, :F] * silu(x[:, F:]) for x [M, 2 F]: the reference's GLU(SiLU())."""
    M, F2 = x.shape
    assert x.dim() == 2 and F2 % 2 == 0 and tuple(out.shape) == (M, F2 // 2) and x.stride(1) == out.stride(1) == 1 and x.dtype == out.dtype
    _launch("mi355x_glu_silu", (dtype_code(x.dtype), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), M, F2 // 2), "mi355x_glu_silu")
    return out


# ------------------------------------------------------------------------------------------------ InformativeDrawings (csrc/lineart.hip)
LINEART_ROWS, LINEART_PADDED, LINEART_QUAD = (ABIS["lineart"].constants[f"MI355X_LINEART_{n}"] for n in ("ROWS", "PADDED", "QUAD"))
LINEART_MAX_CIN = ABIS["lineart"].constants["MI355X_LINEART_MAX_CIN"]


def lineart_rows(B: int, H: int, W: int, layout: int = LINEART_ROWS, pad: int = 0) -> int:
    """Rows of the buffer that holds a logical [B, H, W] activation in `layout` (include/mi355x_refiners_lineart.h)."""
    if layout == LINEART_QUAD:
        return B * (H // 2) * (W // 2)
    return B * (H + 2 * pad) * (W + 2 * pad)


def _lineart_src(a: Any, x: Tensor, B: int, H: int, W: int, C_: int, layout: int, pad: int) -> None:
    cols = 4 * C_ if layout == LINEART_QUAD else C_
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == lineart_rows(B, H, W, layout, pad) and x.shape[1] >= cols, "activation of another shape than its layout"
    a.dtype, a.B, a.H, a.W, a.layout, a.pad, a.x, a.ldx = dtype_code(x.dtype), B, H, W, layout, pad, x.data_ptr(), x.stride(0)


def lineart_pack_stem(w: Tensor) -> Tensor:
    """Conv2d weight [64, Cin, 7, 7] -> float32 [Cin * 49, 64] (row (ci 7 + ky) 7 + kx, column co), as mi355x_lineart_stem reads it."""
    o, i, kh, kw = w.shape
    assert (o, kh, kw) == (64, 7, 7)
    return w.detach().float().permute(1, 2, 3, 0).reshape(i * 49, 64).contiguous()


def lineart_pack_head(w: Tensor) -> Tensor:
    """Conv2d weight [1, 64, 7, 7] -> float32 [49, 64] (row 7 ky + kx, column ci), as mi355x_lineart_head reads it."""
    assert tuple(w.shape) == (1, 64, 7, 7)
    return w.detach().float()[0].permute(1, 2, 0).reshape(49, 64).contiguous()


def lineart_stem(image: Tensor, w: Tensor, bias: Optional[Tensor], out: Tensor) -> Tensor:
    """out [B * H * W, >= 64] rows = Conv2d(Cin -> 64, 7)(ReflectionPad2d(3)(image [B, Cin, H, W])); w = lineart_pack_stem(weight), bias float32 [64] or None."""
    B, Cin, H, W = image.shape
    assert image.stride(3) == 1 and image.dtype == out.dtype and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == B * H * W and out.shape[1] >= 64
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (Cin * 49, 64) and (bias is None or (bias.dtype == torch.float32 and bias.numel() == 64 and bias.is_contiguous()))
    a = LineartStemArgs()
    a.dtype, a.B, a.H, a.W, a.Cin = dtype_code(image.dtype), B, H, W, Cin
    a.image, a.batch_stride, a.channel_stride, a.row_stride = image.data_ptr(), image.stride(0), image.stride(1), image.stride(2)
    a.w, a.bias = w.data_ptr(), None if bias is None else bias.data_ptr()
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    _launch("mi355x_lineart_stem", (C.byref(a),), "mi355x_lineart_stem", keep=(image, w, bias, out))
    return out


def lineart_in_stats_ws_floats(B: int, H: int, W: int, C_: int, layout: int = LINEART_ROWS) -> int:
    return int(load().mi355x_lineart_in_stats_ws_floats(B, H, W, C_, layout))


def lineart_in_stats(x: Tensor, B: int, H: int, W: int, C_: int, eps: float, stats: Tensor, layout: int = LINEART_ROWS, pad: int = 0, ws: Optional[Tensor] = None) -> Tensor:
    """stats float32 [B, C_, 2] = (mean, 1 / sqrt(biased variance + eps)) per image and channel of the logical [B, H, W, C_] activation x."""
    assert stats.dtype == torch.float32 and tuple(stats.shape) == (B, C_, 2) and stats.is_contiguous()
    a = LineartInStatsArgs()
    _lineart_src(a, x, B, H, W, C_, layout, pad)
    if ws is None:
        ws = torch.empty(max(lineart_in_stats_ws_floats(B, H, W, C_, layout), 4) if x.device.type != "meta" else 4, device=x.device, dtype=torch.float32)
    assert ws.dtype == torch.float32 and ws.is_contiguous()
    a.C, a.eps, a.stats, a.ws, a.ws_floats = C_, eps, stats.data_ptr(), ws.data_ptr(), ws.numel()
    _launch("mi355x_lineart_in_stats", (C.byref(a),), "mi355x_lineart_in_stats", keep=(x, stats, ws))
    return stats


def lineart_in_apply(x: Tensor, B: int, H: int, W: int, C_: int, stats: Tensor, out: Tensor, layout: int = LINEART_ROWS, pad: int = 0, relu: bool = False,
                     res: Optional[Tensor] = None, res_pad: int = 0, ring: int = 0) -> Tensor:
    """out = (x - mean) rstd [ReLU] [+ interior of res], written as rows of (H + 2 ring) x (W + 2 ring) images whose ring is ReflectionPad2d(ring)."""
    assert stats.dtype == torch.float32 and tuple(stats.shape) == (B, C_, 2) and stats.is_contiguous()
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == lineart_rows(B, H, W, LINEART_PADDED, ring) and out.shape[1] >= C_ and out.dtype == x.dtype
    a = LineartInApplyArgs()
    _lineart_src(a, x, B, H, W, C_, layout, pad)
    a.C, a.stats, a.relu, a.ring, a.out, a.ldo = C_, stats.data_ptr(), int(relu), ring, out.data_ptr(), out.stride(0)
    if res is not None:
        assert res.dim() == 2 and res.stride(1) == 1 and res.shape[0] == lineart_rows(B, H, W, LINEART_PADDED, res_pad) and res.shape[1] >= C_ and res.dtype == x.dtype
        a.res, a.ldr, a.res_pad = res.data_ptr(), res.stride(0), res_pad
    _launch("mi355x_lineart_in_apply", (C.byref(a),), "mi355x_lineart_in_apply", keep=(x, stats, res, out))
    return out


def lineart_head(x: Tensor, B: int, H: int, W: int, stats: Tensor, w: Tensor, bias: float, out: Tensor, layout: int = LINEART_ROWS, pad: int = 0) -> Tensor:
    """out [B, 1, H, W] = Sigmoid(Conv2d(64 -> 1, 7)(ReflectionPad2d(3)(ReLU(InstanceNorm2d(x)))) + bias); w = lineart_pack_head(weight)."""
    assert stats.dtype == torch.float32 and tuple(stats.shape) == (B, 64, 2) and stats.is_contiguous()
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (49, 64)
    assert out.dim() == 4 and tuple(out.shape) == (B, 1, H, W) and out.stride(3) == 1 and out.stride(2) == W and out.dtype == x.dtype
    a = LineartHeadArgs()
    _lineart_src(a, x, B, H, W, 64, layout, pad)
    a.stats, a.w, a.bias, a.out, a.out_batch_stride = stats.data_ptr(), w.data_ptr(), float(bias), out.data_ptr(), out.stride(0)
    _launch("mi355x_lineart_head", (C.byref(a),), "mi355x_lineart_head", keep=(x, stats, w, out))
    return out


# ------------------------------------------------------------------------------------------------ HQ-SAM mask prediction (csrc/sam_hq.hip)
def ln2d_gelu_wide(x: Tensor, C_: int, gamma: Tensor, beta: Tensor, eps: float, out: Tensor, scatter_hw: tuple[int, int]) -> Tensor:
    """convt2x2_ln_gelu with scatter_hw for C_ = 128 or 256: x [M, >= 4*C_] (four groups (dy, dx) of C_ columns) -> out [4*M, >= C_] NHWC rows."""
    assert x.dim() == 2 and out.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1 and x.dtype == out.dtype
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C_ == beta.numel()
    M = x.shape[0]
    assert x.shape[1] >= 4 * C_ and out.shape[0] == 4 * M and out.shape[1] >= C_
    _launch("mi355x_ln2d_gelu_wide", (dtype_code(x.dtype), x.data_ptr(), x.stride(0), M, C_, gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(), out.stride(0),
                                     scatter_hw[0], scatter_hw[1]), "mi355x_ln2d_gelu_wide", keep=(gamma, beta))
    return out


def sam_mask_head_up(x: Tensor, P: int, Hin: int, Win: int, w: Tensor, bias: Tensor, hyper: Tensor, out: Tensor, u: Tensor) -> Tensor:
    """sam_mask_head that also stores the upscaled embedding: u [P*2Hin*2Win, >= 32] rows (columns 32.. of a wider row are left alone)."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == P * Hin * Win and x.shape[1] >= 64 and w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (64, 128)
    assert bias.dtype == torch.float32 and bias.numel() == 32 and hyper.dim() == 3 and hyper.stride(2) == 1 and hyper.shape[0] == P
    nk = hyper.shape[1]
    assert out.dim() == 4 and tuple(out.shape[1:]) == (nk, 2 * Hin, 2 * Win) and out.stride(3) == 1 and out.stride(2) == 2 * Win and out.stride(1) == 4 * Hin * Win
    assert u.dim() == 2 and u.stride(1) == 1 and u.shape[0] == 4 * P * Hin * Win and u.shape[1] >= 32 and u.dtype == x.dtype
    a = SamMaskHeadUpArgs()
    a.dtype = dtype_code(x.dtype)
    a.P, a.Hin, a.Win, a.nk = P, Hin, Win, nk
    a.x, a.ldx, a.w, a.bias = x.data_ptr(), x.stride(0), w.data_ptr(), bias.data_ptr()
    a.hyper, a.ld_hyper, a.hyper_batch_stride = hyper.data_ptr(), hyper.stride(1), hyper.stride(0)
    a.out, a.out_batch_stride = out.data_ptr(), out.stride(0)
    a.u, a.ldu = u.data_ptr(), u.stride(0)
    _launch("mi355x_sam_mask_head_up", (C.byref(a),), "mi355x_sam_mask_head_up", keep=(w, bias))
    return out


def sam_hq_mask_head(y: Tensor, P: int, H: int, W: int, gamma: Tensor, beta: Tensor, eps: float, w2: Tensor, b2: Tensor, h: Tensor, fq: Tensor, out: Tensor) -> Tensor:
    """y [P*H*W, >= 64] rows; gamma / beta float32 [64]; w2 float32 [32, 9, 64]; b2 float32 [32]; h [P, 32] (a view, unit column stride);
    fq [(H/2)*(W/2), >= 128] in quadrant layout; out [P, 1, H, W]."""
    assert y.dim() == 2 and y.stride(1) == 1 and y.shape[0] == P * H * W and y.shape[1] >= 64
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == 64 == beta.numel()
    assert w2.dtype == torch.float32 and w2.is_contiguous() and tuple(w2.shape) == (32, 9, 64) and b2.dtype == torch.float32 and b2.numel() == 32
    assert h.dim() == 2 and tuple(h.shape) == (P, 32) and h.stride(1) == 1 and h.dtype == y.dtype
    assert fq.dim() == 2 and fq.stride(1) == 1 and fq.shape[0] == (H // 2) * (W // 2) and fq.shape[1] >= 128 and fq.dtype == y.dtype
    assert out.dim() == 4 and tuple(out.shape) == (P, 1, H, W) and out.stride(3) == 1 and out.stride(2) == W and out.dtype == y.dtype
    a = SamHqMaskHeadArgs()
    a.dtype = dtype_code(y.dtype)
    a.P, a.H, a.W = P, H, W
    a.y, a.ldy = y.data_ptr(), y.stride(0)
    a.gamma, a.beta, a.eps = gamma.data_ptr(), beta.data_ptr(), eps
    a.w2, a.b2 = w2.data_ptr(), b2.data_ptr()
    a.h, a.h_stride = h.data_ptr(), h.stride(0)
    a.fq, a.ldf = fq.data_ptr(), fq.stride(0)
    a.out, a.out_batch_stride = out.data_ptr(), out.stride(0)
    _launch("mi355x_sam_hq_mask_head", (C.byref(a),), "mi355x_sam_hq_mask_head", keep=(gamma, beta, w2, b2))
    return out


# ------------------------------------------------------------------------------------------------ StyleAligned shared self-attention (csrc/style_aligned.hip)
def adain_stats_ws_floats(B: int, L: int, C_: int) -> int:
    """Floats of the scratch mi355x_adain_stats needs for [B, L, C_] (0 when one slab of tokens per workgroup column is enough)."""
    return int(load().mi355x_adain_stats_ws_floats(B, L, C_))


def adain_stats(x: Tensor, stats: Tensor, ws: Optional[Tensor] = None) -> Tensor:
    """x [B, L, C] view (contiguous channels; may be a column slice of a wider buffer) -> stats float32 [B, C, 2] = (mean, unbiased std) over
    the L tokens.  ws: float32 scratch of adain_stats_ws_floats(B, L, C) elements."""
    assert x.dim() == 3 and x.stride(2) == 1 and stats.dtype == torch.float32 and stats.is_contiguous() and tuple(stats.shape) == (x.shape[0], x.shape[2], 2)
    a = AdainStatsArgs()
    a.dtype = dtype_code(x.dtype)
    a.B, a.L, a.C = x.shape
    a.x, a.ldx, a.x_batch_stride, a.stats = x.data_ptr(), x.stride(1), x.stride(0), stats.data_ptr()
    need = adain_stats_ws_floats(a.B, a.L, a.C)
    if need:
        assert ws is not None and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= need
        a.ws, a.ws_floats = ws.data_ptr(), ws.numel()
    _launch("mi355x_adain_stats", (C.byref(a),), "mi355x_adain_stats", keep=(ws, stats))
    return stats


def style_aligned_pack(q: Tensor, k: Tensor, vt: Tensor, q_stats: Tensor, k_stats: Tensor, group: int, scale: Tensor, eps: float, k_sh: Tensor, vt_sh: Tensor) -> None:
    """q, k [B, L, C] views (q is rewritten in place), vt [C, B, Lp] view; q_stats / k_stats float32 [B, C, 2] views (batch stride free: column
    halves of one [B, 2C, 2] table); group = rows per reference group; scale: one float32 on the device; k_sh [B, Lkp, C], vt_sh [C, B, Lkp],
    Lkp >= 2L, padding zeroed by the caller.  See mi355x_style_aligned_pack in the header."""
    B, L, C_ = q.shape
    for t in (q, k, vt, k_sh, vt_sh):
        assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == q.dtype
    assert tuple(k.shape) == (B, L, C_) and vt.shape[0] == C_ and vt.shape[1] == B and vt.shape[2] >= L
    assert k_sh.shape[0] == B and k_sh.shape[1] >= 2 * L and k_sh.shape[2] == C_ and vt_sh.shape[0] == C_ and vt_sh.shape[1] == B and vt_sh.shape[2] >= 2 * L
    for st in (q_stats, k_stats):
        assert st.dtype == torch.float32 and tuple(st.shape) == (B, C_, 2) and st.stride(2) == 1 and st.stride(1) == 2
    assert q_stats.stride(0) == k_stats.stride(0) and scale.dtype == torch.float32 and scale.numel() >= 1
    a = StyleAlignedArgs()
    a.dtype = dtype_code(q.dtype)
    a.B, a.L, a.C, a.n = B, L, C_, group
    a.q, a.ldq, a.q_batch_stride = q.data_ptr(), q.stride(1), q.stride(0)
    a.k, a.ldk, a.k_batch_stride = k.data_ptr(), k.stride(1), k.stride(0)
    a.vt, a.ldvt, a.vt_batch_stride = vt.data_ptr(), vt.stride(0), vt.stride(1)
    a.q_stats, a.k_stats, a.stats_batch_stride = q_stats.data_ptr(), k_stats.data_ptr(), q_stats.stride(0)
    a.scale, a.eps = scale.data_ptr(), eps
    a.k_sh, a.ld_ksh, a.ksh_batch_stride = k_sh.data_ptr(), k_sh.stride(1), k_sh.stride(0)
    a.vt_sh, a.ld_vtsh, a.vtsh_batch_stride = vt_sh.data_ptr(), vt_sh.stride(0), vt_sh.stride(1)
    _launch("mi355x_style_aligned_pack", (C.byref(a),), "mi355x_style_aligned_pack", keep=(q_stats, k_stats, scale, k_sh, vt_sh))


# ------------------------------------------------------------------------------------------------ MultiDiffusion (csrc/multi_diffusion.hip)
MD_MAX_TARGETS = _K["MI355X_MD_MAX_TARGETS"]
MD_SRC_CANVAS, MD_SRC_INIT = _K["MI355X_MD_SRC_CANVAS"], _K["MI355X_MD_SRC_INIT"]
MD_GATHER_DESC_BYTES, MD_BLEND_DESC_BYTES = C.sizeof(MdGatherDesc), C.sizeof(MdBlendDesc)


def _md_rows(arr, n: int, row_bytes: int) -> Tensor:
    """A ctypes descriptor array as a uint8 CPU tensor [n, row_bytes]; no rows give an empty table (torch.frombuffer refuses an empty buffer)."""
    if n == 0:
        return torch.empty(0, row_bytes, dtype=torch.uint8)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).view(n, row_bytes)


def md_gather_rows(rows: list) -> Tensor:
    """[(kind, top, left, init_row, a, b, s)] -> the descriptor rows of mi355x_md_gather as a uint8 CPU tensor [T, 32] (copy it to the device table)."""
    arr = (MdGatherDesc * len(rows))()
    for d, (kind, top, left, init_row, a, b, s) in zip(arr, rows):
        d.kind, d.top, d.left, d.init_row, d.a, d.b, d.s = int(kind), int(top), int(left), int(init_row), float(a), float(b), float(s)
    return _md_rows(arr, len(rows), MD_GATHER_DESC_BYTES)


def md_blend_rows(rows: list) -> Tensor:
    """[(top, left, h, w, weight, stepped_off, mask or None)] -> the descriptor rows of mi355x_md_blend as a uint8 CPU tensor [n, 64].  A mask is a float32
    device tensor that broadcasts to [C, h, w] (or [1, C, h, w]): `.expand()` it first, its strides go into the row; keep it alive as long as the rows are used."""
    arr = (MdBlendDesc * len(rows))()
    for d, (top, left, h, w, weight, off, mask) in zip(arr, rows):
        d.top, d.left, d.h, d.w, d.weight, d.stepped_off = int(top), int(left), int(h), int(w), float(weight), int(off)
        if mask is not None:
            assert mask.dtype == torch.float32 and mask.dim() in (3, 4) and tuple(mask.shape[-2:]) == (h, w) and (mask.dim() == 3 or mask.shape[0] == 1)
            d.mask, (d.mask_sc, d.mask_sh, d.mask_sw) = mask.data_ptr(), mask.stride()[-3:]
    return _md_rows(arr, len(rows), MD_BLEND_DESC_BYTES)


def md_gather(canvas: Tensor, noise: Optional[Tensor], init: Optional[Tensor], desc: Tensor, desc_host: Tensor, view: Tensor, model_in: Tensor) -> None:
    """canvas (noise) [1, C, H, W]; init [n_init, C, h, w] or None; desc: device uint8 [T, 32], desc_host: the same rows on the host (md_gather_rows);
    view [T, C, h, w], model_in [2T, C, h, w].  See mi355x_md_gather in the header."""
    T, C_, h, w = view.shape
    assert canvas.dim() == 4 and canvas.shape[0] == 1 and canvas.shape[1] == C_ and tuple(model_in.shape) == (2 * T, C_, h, w)
    for t in (canvas, noise, init, view, model_in):
        assert t is None or (t.is_contiguous() and t.dtype == canvas.dtype)
    assert noise is None or noise.shape == canvas.shape
    assert init is None or tuple(init.shape[1:]) == (C_, h, w)
    assert desc.dtype == torch.uint8 and desc.is_contiguous() and desc.numel() >= T * MD_GATHER_DESC_BYTES and desc.device == canvas.device
    assert desc_host.dtype == torch.uint8 and desc_host.is_contiguous() and desc_host.numel() >= T * MD_GATHER_DESC_BYTES and desc_host.device.type == "cpu"
    a = MdGatherArgs()
    a.dtype = dtype_code(canvas.dtype)
    a.T, a.C, a.h, a.w, a.H, a.W, a.n_init = T, C_, h, w, canvas.shape[2], canvas.shape[3], 0 if init is None else init.shape[0]
    a.canvas, a.noise, a.init = canvas.data_ptr(), None if noise is None else noise.data_ptr(), None if init is None else init.data_ptr()
    a.desc, a.desc_host, a.view, a.model_in = desc.data_ptr(), desc_host.data_ptr(), view.data_ptr(), model_in.data_ptr()
    _launch("mi355x_md_gather", (C.byref(a),), "mi355x_md_gather", keep=(a, canvas, noise, init, desc, desc_host, view, model_in))


def md_target_step(view: Tensor, unet_out: Tensor, stepped: Tensor, hist: Optional[Tensor], coef: Tensor, linear: bool) -> None:
    """view, stepped (, hist) [T, ...]; unet_out [2T, ...] = (unconditional, conditional); coef: float32 [T, 8] on the device, one row per target:
    (cfg, sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), noise factor, 0, 0, 0) or, `linear`, (cfg, hx, he, kx, ke, kd, kp, -).  See mi355x_md_target_step."""
    T = view.shape[0]
    for t in (view, unet_out, stepped, hist):
        assert t is None or (t.is_contiguous() and t.dtype == view.dtype)
    assert unet_out.numel() == 2 * view.numel() and stepped.shape == view.shape and (hist is None or hist.shape == view.shape)
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.numel() >= 8 * T and coef.device == view.device
    a = MdStepArgs()
    a.dtype, a.form, a.T, a.n = dtype_code(view.dtype), _K["MI355X_MD_FORM_LINEAR" if linear else "MI355X_MD_FORM_DDIM"], T, view.numel() // T
    a.view, a.unet_out, a.stepped, a.hist, a.coef = view.data_ptr(), unet_out.data_ptr(), stepped.data_ptr(), None if hist is None else hist.data_ptr(), coef.data_ptr()
    _launch("mi355x_md_target_step", (C.byref(a),), "mi355x_md_target_step", keep=(a, view, unet_out, stepped, hist, coef))


def md_blend(canvas: Tensor, stepped: Tensor, desc: Tensor, desc_host: Tensor, n_targets: int) -> Tensor:
    """canvas [1, C, H, W], updated in place; stepped: any contiguous tensor of the canvas dtype that holds every target's [C, h, w] tile at its row's
    offset; desc / desc_host: device / host uint8 rows of md_blend_rows.  See mi355x_md_blend in the header."""
    assert canvas.dim() == 4 and canvas.shape[0] == 1 and canvas.is_contiguous() and stepped.is_contiguous() and stepped.dtype == canvas.dtype
    assert desc.dtype == torch.uint8 and desc.is_contiguous() and desc.numel() >= n_targets * MD_BLEND_DESC_BYTES and desc.device == canvas.device
    assert desc_host.dtype == torch.uint8 and desc_host.is_contiguous() and desc_host.numel() >= n_targets * MD_BLEND_DESC_BYTES and desc_host.device.type == "cpu"
    a = MdBlendArgs()
    a.dtype, a.n_targets, (a.C, a.H, a.W) = dtype_code(canvas.dtype), n_targets, canvas.shape[1:]
    a.canvas, a.stepped, a.stepped_elems, a.desc, a.desc_host = canvas.data_ptr(), stepped.data_ptr(), stepped.numel(), desc.data_ptr(), desc_host.data_ptr()
    _launch("mi355x_md_blend", (C.byref(a),), "mi355x_md_blend", keep=(a, canvas, stepped, desc, desc_host))
    return canvas


# ------------------------------------------------------------------------------------------------ tiled VAE (csrc/norm.hip, csrc/tiled_vae.hip)
VAE_POS_BYTES, VAE_AXIS_BYTES, VAE_BLEND_TILE_BYTES = C.sizeof(VaeTilePos), C.sizeof(VaeAxis), C.sizeof(VaeBlendTile)
VAE_MAX_AXIS = _K["MI355X_VAE_MAX_AXIS"]


def groupnorm_table(x: Tensor, gamma: Tensor, groups: int, eps: float, tab: Tensor, raw: Optional[Tensor] = None, ws: Optional[Tensor] = None) -> Tensor:
    """x [B, HW, C] (contiguous channels) -> tab float32 [B, C, 2] = (group mean, rstd * gamma), the table GroupNorm's apply pass reads; raw float32
    [B, G, 2] = (mean, biased variance) per group when given.  See mi355x_groupnorm_table."""
    B, HW, Cc = x.shape
    assert x.stride(2) == 1 and x.stride(0) == HW * x.stride(1) and gamma.dtype == x.dtype and gamma.numel() == Cc
    assert tab.dtype == torch.float32 and tab.is_contiguous() and tab.numel() == B * Cc * 2
    assert raw is None or (raw.dtype == torch.float32 and raw.is_contiguous() and raw.numel() == B * groups * 2)
    need = load().mi355x_groupnorm_ws_floats(B, HW, Cc)
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=x.device)
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= need
    a = GroupNormTableArgs()
    a.dtype, a.B, a.HW, a.C, a.G = dtype_code(x.dtype), B, HW, Cc, groups
    a.x, a.ldx, a.gamma, a.eps, a.ws, a.tab, a.raw = x.data_ptr(), x.stride(1), gamma.data_ptr(), eps, ws.data_ptr(), tab.data_ptr(), None if raw is None else raw.data_ptr()
    _launch("mi355x_groupnorm_table", (C.byref(a),), "mi355x_groupnorm_table", keep=(a, x, gamma, ws, tab, raw))
    return tab


def groupnorm_fixed(x: Tensor, tab: Tensor, beta: Tensor, silu: bool, out: Tensor) -> Tensor:
    """out = (x - tab[c, 0]) * tab[c, 1] + beta[c] (+ SiLU) with ONE float32 table [C, 2] for every sample of x [B, HW, C].  See mi355x_groupnorm_fixed."""
    B, HW, Cc = x.shape
    assert x.stride(2) == 1 and out.stride(2) == 1 and x.stride(0) == HW * x.stride(1) and out.stride(0) == HW * out.stride(1) and out.shape == x.shape and out.dtype == x.dtype
    assert tab.dtype == torch.float32 and tab.is_contiguous() and tab.numel() == Cc * 2 and beta.dtype == x.dtype and beta.numel() == Cc
    a = GroupNormFixedArgs()
    a.dtype, a.B, a.HW, a.C, a.silu = dtype_code(x.dtype), B, HW, Cc, int(silu)
    a.x, a.ldx, a.tab, a.beta, a.out, a.ldo = x.data_ptr(), x.stride(1), tab.data_ptr(), beta.data_ptr(), out.data_ptr(), out.stride(1)
    _launch("mi355x_groupnorm_fixed", (C.byref(a),), "mi355x_groupnorm_fixed", keep=(a, x, tab, beta, out))
    return out


def vae_pos_rows(rows: list) -> Tensor:
    """[(top, left)] -> the position rows of mi355x_vae_tile_gather as a uint8 CPU tensor [T, 8]."""
    arr = (VaeTilePos * len(rows))()
    for d, (top, left) in zip(arr, rows):
        d.top, d.left = int(top), int(left)
    return _md_rows(arr, len(rows), VAE_POS_BYTES)


def vae_axis_rows(xs: list, ys: list) -> Tensor:
    """[(start, extent)] of the columns, then of the rows -> the axis table of mi355x_vae_tile_blend as a uint8 CPU tensor [nx + ny, 8]."""
    arr = (VaeAxis * (len(xs) + len(ys)))()
    for d, (start, extent) in zip(arr, list(xs) + list(ys)):
        d.start, d.extent = int(start), int(extent)
    return _md_rows(arr, len(xs) + len(ys), VAE_AXIS_BYTES)


def vae_blend_rows(rows: list) -> Tensor:
    """[(off, s_c, s_y, s_x, ramp_off, ramp_len)] in list order (ix * ny + iy) -> the tile rows of mi355x_vae_tile_blend as a uint8 CPU tensor [T, 40]."""
    arr = (VaeBlendTile * len(rows))()
    for d, (off, s_c, s_y, s_x, ramp_off, ramp_len) in zip(arr, rows):
        d.off, d.s_c, d.s_y, d.s_x, d.ramp_off, d.ramp_len = int(off), int(s_c), int(s_y), int(s_x), int(ramp_off), int(ramp_len)
    return _md_rows(arr, len(rows), VAE_BLEND_TILE_BYTES)


def _table_pair(dev: Tensor, host: Tensor, nbytes: int, like: Tensor) -> None:
    assert dev.dtype == torch.uint8 and dev.is_contiguous() and dev.numel() >= nbytes and dev.device == like.device
    assert host.dtype == torch.uint8 and host.is_contiguous() and host.numel() >= nbytes and host.device.type == "cpu"


def vae_tile_gather(canvas: Tensor, pos: Tensor, pos_host: Tensor, dst: Tensor, T: int, hw: tuple[int, int], strides: tuple[int, int, int, int], cpad: Optional[int] = None) -> None:
    """canvas [1, C, H, W] (contiguous); T tiles of hw = (h, w) at the (top, left) rows of pos / pos_host (device / host, vae_pos_rows) -> dst, any contiguous
    tensor of the canvas dtype, written at t * s_tile + c * s_c + y * s_y + x * s_x for strides = (s_tile, s_c, s_y, s_x); channels [C, cpad) are zeros.
    See mi355x_vae_tile_gather."""
    assert canvas.dim() == 4 and canvas.shape[0] == 1 and canvas.is_contiguous() and dst.is_contiguous() and dst.dtype == canvas.dtype
    _table_pair(pos, pos_host, T * VAE_POS_BYTES, canvas)
    a = VaeGatherArgs()
    a.dtype, a.T, a.C, a.cpad, (a.h, a.w), (a.H, a.W) = dtype_code(canvas.dtype), T, canvas.shape[1], canvas.shape[1] if cpad is None else cpad, hw, canvas.shape[2:]
    a.canvas, a.pos, a.pos_host, a.dst, a.dst_elems = canvas.data_ptr(), pos.data_ptr(), pos_host.data_ptr(), dst.data_ptr(), dst.numel()
    a.s_tile, a.s_c, a.s_y, a.s_x = strides
    _launch("mi355x_vae_tile_gather", (C.byref(a),), "mi355x_vae_tile_gather", keep=(a, canvas, pos, pos_host, dst))


def vae_tile_blend(canvas: Tensor, src: Tensor, ramps: Tensor, axis: Tensor, axis_host: Tensor, tiles: Tensor, tiles_host: Tensor, nxy: tuple[int, int],
                   stride_xy: tuple[int, int], tile_wh: tuple[int, int]) -> Tensor:
    """canvas [1, C, H, W] <- the ramp-weighted mean of the grid's tiles, read from src (any contiguous tensor of the canvas dtype) at each tile row's offset
    and strides.  ramps: float32 device tensor of the linspace tables; axis / tiles: device uint8 tables of vae_axis_rows / vae_blend_rows with their host
    copies.  See mi355x_vae_tile_blend."""
    assert canvas.dim() == 4 and canvas.shape[0] == 1 and canvas.is_contiguous() and src.is_contiguous() and src.dtype == canvas.dtype
    assert ramps.dtype == torch.float32 and ramps.is_contiguous() and ramps.device == canvas.device
    nx, ny = nxy
    _table_pair(axis, axis_host, (nx + ny) * VAE_AXIS_BYTES, canvas)
    _table_pair(tiles, tiles_host, nx * ny * VAE_BLEND_TILE_BYTES, canvas)
    a = VaeBlendArgs()
    a.dtype, (a.C, a.H, a.W), (a.nx, a.ny), (a.stride_x, a.stride_y), (a.tile_w, a.tile_h) = dtype_code(canvas.dtype), canvas.shape[1:], nxy, stride_xy, tile_wh
    a.canvas, a.src, a.src_elems, a.ramps, a.ramp_elems = canvas.data_ptr(), src.data_ptr(), src.numel(), ramps.data_ptr() if ramps.numel() else None, ramps.numel()
    a.axis, a.axis_host, a.tiles, a.tiles_host = axis.data_ptr(), axis_host.data_ptr(), tiles.data_ptr(), tiles_host.data_ptr()
    _launch("mi355x_vae_tile_blend", (C.byref(a),), "mi355x_vae_tile_blend", keep=(a, canvas, src, ramps, axis, axis_host, tiles, tiles_host))
    return canvas


def set_glds(enabled: bool) -> None:
    """A/B switch: global_load_lds staging (default) vs register staging, for the GEMM and attention tile loaders."""
    lib = load()
    lib.mi355x_set_option(b"glds", int(enabled))
    lib.mi355x_attention_set_glds(int(enabled))
