"""The ctypes binding is read from the headers under include/ that native.ABI_HEADERS lists (refiners_amd/abi.py).  These CPU tests hold the
reader to the C compiler's view of every header (every size and offset), to its own strictness, and to the names, prototypes and constants
written out here by hand; they hold the built library and the build's dependency lists to the same table."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from refiners_amd import abi, build_native, native
from tests import support as S

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "mi355x_refiners.h"

PUBLIC_STRUCTS = """GemmSeg GemmArgs KvStream AttnArgs AttnGeneralArgs LayerNormArgs GroupNormArgs SamAttnArgs SamMaskHeadArgs SamPostprocessArgs AdainStatsArgs
StyleAlignedArgs MdGatherDesc MdGatherArgs MdStepArgs MdBlendDesc MdBlendArgs GroupNormTableArgs GroupNormFixedArgs VaeTilePos VaeGatherArgs VaeAxis VaeBlendTile
VaeBlendArgs""".split()
#: key -> (header, its Python struct names, its function names; None = the core header's 39, pinned by count), as the headers stand
PINNED = {
    "core": ("mi355x_refiners.h", PUBLIC_STRUCTS, None),
    "sam_hq": ("mi355x_refiners_sam_hq.h", ["SamHqMaskHeadArgs", "SamMaskHeadUpArgs"], ["mi355x_sam_hq_mask_head", "mi355x_sam_mask_head_up", "mi355x_ln2d_gelu_wide"]),
    "solver_step": ("mi355x_refiners_solver_step.h", [], ["mi355x_ddim_step", "mi355x_linear_step"]),
    "swin": ("mi355x_refiners_swin.h", ["WindowAttentionArgs"], ["mi355x_window_attention"]),
    "mvanet": ("mi355x_refiners_mvanet.h", ["MvanetPoolArgs", "MvanetGateArgs", "MvanetResizeAddArgs"],
               ["mi355x_mvanet_pool", "mi355x_mvanet_gate", "mi355x_mvanet_resize_add", "mi355x_mvanet_prelu", "mi355x_mvanet_split_views"]),
    "dinov2": ("mi355x_refiners_dinov2.h", ["Dinov2PosResampleArgs", "Dinov2TokensArgs"], ["mi355x_dinov2_pos_resample", "mi355x_dinov2_tokens", "mi355x_glu_silu"]),
    "ella": ("mi355x_refiners_ella.h", ["EllaAdaLnArgs"], ["mi355x_ella_adaln"]),
    "lineart": ("mi355x_refiners_lineart.h", ["LineartStemArgs", "LineartInStatsArgs", "LineartInApplyArgs", "LineartHeadArgs"],
                ["mi355x_lineart_stem", "mi355x_lineart_in_stats", "mi355x_lineart_in_stats_ws_floats", "mi355x_lineart_in_apply", "mi355x_lineart_head"]),
    "reference_only": ("mi355x_refiners_reference_only.h", ["AttnJointArgs"], ["mi355x_attention_joint"]),
    "cond_input": ("mi355x_refiners_cond_input.h", [], ["mi355x_cond_step", "mi355x_cond_fill", "mi355x_inpaint_conditions"]),
    "xattn": ("mi355x_refiners_xattn.h", [], ["mi355x_gemm_attention"]),
    "sde_step": ("mi355x_refiners_sde_step.h", [], ["mi355x_cfg_sde_step", "mi355x_sde_step"]),
}
#: key -> the sources that include the header (every source includes the core header, which has no entry in build_native.DEPS)
INCLUDED_BY = {"core": [], "sam_hq": ["sam_hq.hip"], "solver_step": ["solver_step.hip"], "swin": ["window_attention.hip"], "mvanet": ["mvanet.hip"], "dinov2": ["dinov2.hip"],
               "ella": ["ella.hip"], "lineart": ["lineart.hip"], "reference_only": ["reference_only.hip"], "cond_input": ["cond_input.hip"], "xattn": ["gemm_xattn.hip"],
               "sde_step": ["solver_step.hip"]}
every_header =pytest.mark.parametrize("key, fname", [(key, fname) for key, fname, _names in native.ABI_HEADERS], ids=[h[0] for h in native.ABI_HEADERS])


def _code(fname: str) -> str:
    """The header without its comments: they mention calls such as mi355x_groupnorm_ws_floats() and words such as "doubles"."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", (HEADER.parent / fname).read_text(), flags=re.S)


def test_every_header_declares_the_pinned_names():
    assert [(key, fname) for key, fname, _names in native.ABI_HEADERS] == [(key, pin[0]) for key, pin in PINNED.items()]
    for key, (_fname, structs, functions) in PINNED.items():
        got = native.ABIS[key]
        assert [cls.__name__ for cls in got.structs.values()] == structs and all(getattr(native, cls.__name__) is cls for cls in got.structs.values()), key
        assert list(got.functions) == functions or (functions is None and len(got.functions) == 39), key
    assert native.EXPORTS == list(native.ABIS["core"].functions) and native.ALL_EXPORTS[:39] == native.EXPORTS
    assert len(native.ALL_EXPORTS) == len(set(native.ALL_EXPORTS)) == 66


@every_header
def test_c_compiler_agrees_with_ctypes_on_every_layout(key, fname, tmp_path):
    """The header compiles alone as strict C99 (for a header without structs that is the whole check), and the compiler gives every struct
    the size, and every field the offset and the size, that ctypes gives the class read from it."""
    structs = native.ABIS[key].structs
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER.parent / fname}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'    printf("{cname} - %zu %zu\\n", (size_t)0, sizeof({cname}));')
        for field in cls._c_fields_:
            lines.append(f'    printf("{cname} {field} %zu %zu\\n", offsetof({cname}, {field}), sizeof((({cname}*)0)->{field}));')
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([S.c_compiler(), "-std=c99", "-Wall", "-Werror", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    compiled = {(s, f): (int(off), int(size)) for s, f, off, size in (line.split() for line in out.splitlines())}

    ours = {}
    for cname, cls in structs.items():
        assert issubclass(cls, C.Structure) and len(cls._c_fields_) == len(cls._fields_) > 0
        ours[(cname, "-")] = (0, C.sizeof(cls))
        for field, (name, _) in zip(cls._c_fields_, cls._fields_):
            ours[(cname, field)] = (getattr(cls, name).offset, getattr(cls, name).size)
    assert len(structs) == len(PINNED[key][1]) and len(ours) >= 2 * len(structs)
    assert ours == compiled, {k: (ours.get(k), compiled.get(k)) for k in set(ours) | set(compiled) if ours.get(k) != compiled.get(k)}
    if key == "core":
        assert len(structs) == 24 and len(ours) > 24
        assert compiled[("mi355x_gemm_args", "-")] == (0, 560) and compiled[("mi355x_gemm_args", "sk_slots")] == (552, 4)
        assert compiled[("mi355x_gemm_args", "seg")][1] == 3 * C.sizeof(native.GemmSeg) and compiled[("mi355x_gemm_args", "prefetch_bytes")][1] == 16  # array fields


GOOD = """
#define N 2
enum { A = 0, B = -3 };
typedef struct { const void* x; int32_t H, W; float s[N]; int64_t t[3]; } inner_t;   /* a comment with typedef struct { and mi355x_no( in it */
typedef struct tag { inner_t in[N]; int32_t* p; const inner_t* q; } outer_t;
int mi355x_a(void);
int64_t mi355x_b(const outer_t* a, inner_t* b, char* buf, const float* f, int32_t n, int64_t m, float s, int k,
                 void* stream);
"""
NAMES = {"inner_t": "Inner", "outer_t": "Outer"}


def test_reader_translates_the_forms_it_knows():
    got = abi.parse(GOOD, NAMES)
    assert got.constants == {"N": 2, "A": 0, "B": -3} and got.enums == [{"A": 0, "B": -3}]
    inner, outer = got.structs["inner_t"], got.structs["outer_t"]
    assert (inner.__name__, outer.__name__) == ("Inner", "Outer")
    assert [(n, t) for n, t in inner._fields_] == [("x", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("s", C.c_float * 2), ("t", C.c_int64 * 3)]
    assert [(n, t) for n, t in outer._fields_] == [("in_", inner * 2), ("p", C.c_void_p), ("q", C.c_void_p)] and outer._c_fields_ == ("in", "p", "q")
    assert got.functions["mi355x_a"] == (C.c_int, [])
    assert got.functions["mi355x_b"] == (C.c_int64, [C.POINTER(outer), C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_int, C.c_void_p])


@pytest.mark.parametrize("bad, names, what", [
    ("typedef struct { uint16_t x; } s_t;", {"s_t": "S"}, "unknown type"),
    ("typedef struct { double x; } s_t;", {"s_t": "S"}, "unknown type"),
    ("int mi355x_f(size_t n);", {}, "unknown type"),
    ("typedef struct { int32_t x[2][2]; } s_t;", {"s_t": "S"}, "declarator"),
    ("typedef struct { int32_t (*fn)(int); } s_t;", {"s_t": "S"}, "declarator"),
    ("typedef struct { int32_t x : 3; } s_t;", {"s_t": "S"}, "declarator"),
    ("typedef struct { int32_t x[M]; } s_t;", {"s_t": "S"}, "array dimension"),
    ("typedef struct { int32_t *a, *b; } s_t;", {"s_t": "S"}, "pointer field"),
    ("typedef struct { void x; } s_t;", {"s_t": "S"}, "behind a pointer"),
    ("typedef struct { int32_t x; } s_t;", {}, "no Python name"),
    ("typedef struct { int32_t x; } a_t;\ntypedef struct { b_t y; } c_t;", {"a_t": "A", "c_t": "C"}, "unknown type"),
    ("typedef struct { int32_t x; } a_t;\nint mi355x_f(a_t a);", {"a_t": "A"}, "by value"),
    ("int mi355x_f(int32_t);", {}, "unparseable parameter"),
    ("void mi355x_f(int32_t n);", {}, "prototype"),
    ("int other_f(int32_t n);", {}, "prototype"),
    ("enum { A, B };", {}, "enumerator"),
    ("#define A (1 << 3)", {}, "preprocessor"),
    ("#if 0\n#endif", {}, "preprocessor"),
    ("struct s { int32_t x; };", {}, "not an enum"),
    ("extern int mi355x_x;", {}, "not an enum"),
])
def test_reader_is_strict(bad, names, what):
    with pytest.raises(abi.AbiError, match=what) as e:
        abi.parse("/* line 1 */\n" + bad, names, where="t.h")
    assert re.match(r"t\.h:[23]: ", str(e.value)), str(e.value)  # the message names the header line


def test_reader_skips_nothing_of_the_forms_it_knows():
    got = abi.parse(GOOD, NAMES)
    code = re.sub(r"/\*.*?\*/", "", GOOD, flags=re.S)
    assert len(got.structs) == len(re.findall(r"typedef\s+struct", code)) > 0
    assert len(got.functions) == len(re.findall(r"mi355x_\w+\s*\(", code)) > 0
    short = dict(list(native.STRUCT_NAMES.items())[:-1])
    with pytest.raises(abi.AbiError, match="mi355x_vae_blend_args has no Python name"):
        abi.parse(HEADER.read_text(), short)


@every_header
def test_reader_skips_nothing(key, fname):
    """Counted without the reader, on the text without comments: every struct and every function of the header is bound, and no `double`."""
    got, code = native.ABIS[key], _code(fname)
    assert len(got.structs) == len(re.findall(r"typedef\s+struct", code)) == len(PINNED[key][1])
    assert list(got.functions) == re.findall(r"\b(mi355x_\w+)\s*\(", code) and len(got.functions) > 0
    assert not re.search(r"\bdouble\b", code)
    if key == "core":
        assert (len(got.structs), len(got.functions)) == (24, 39)


def test_a_name_that_two_headers_declare_fails_the_import(tmp_path):
    first = [("a", "a.h", {"a_t": "A"})]
    (tmp_path / "a.h").write_text("typedef struct { int32_t x; } a_t;\nint mi355x_f(const a_t* a);\n")
    (tmp_path / "b.h").write_text("int mi355x_g(const a_t* a, void* stream);\n")  # disjoint, and it may name the first header's struct
    got = abi.read_all(first + [("b", "b.h", {})], tmp_path)
    assert list(got) == ["a", "b"] and got["b"].functions["mi355x_g"] == (C.c_int, [C.POINTER(got["a"].structs["a_t"]), C.c_void_p])
    for text, names, twice in [("int mi355x_f(int32_t n);", {}, "mi355x_f"), ("typedef struct { float y; } a_t;", {"a_t": "B"}, "a_t"),
                               ("typedef struct { float y; } b_t;", {"b_t": "A"}, "A")]:
        (tmp_path / "b.h").write_text(text + "\n")
        with pytest.raises(abi.AbiError, match=rf"^b\.h: {twice} is already declared by a\.h$"):
            abi.read_all(first + [("b", "b.h", names)], tmp_path)


@every_header
def test_build_lists_hold_the_header(key, fname):
    spelt = "../../include/" + fname
    assert spelt in build_native.HEADERS and len(build_native.HEADERS) == len(set(build_native.HEADERS))
    users = [src for src, deps in build_native.DEPS.items() if spelt in deps]
    assert set(users) <= set(build_native.SOURCES) and (users or key == "core") and users == INCLUDED_BY[key]


def test_deps_are_what_the_compiler_includes():
    """DEPS decides which objects an incremental build recompiles: for every source it is the project's own files in the compiler's -MM list."""
    try:
        hipcc = build_native.hipcc_path()
    except RuntimeError as e:
        pytest.skip(str(e))
    assert list(build_native.DEPS) == build_native.SOURCES
    procs = {src: subprocess.Popen([hipcc, f"--offload-arch={build_native.ARCH}", "--cuda-host-only", "-std=c++17", "-MM", str(build_native.CSRC / src)],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for src in build_native.SOURCES}
    for src, p in procs.items():
        out, err = p.communicate()
        assert p.returncode == 0, err
        listed = {Path(f).resolve() for f in out.replace("\\\n", " ").split()[1:]}  # `<object>: <source> <included file> ...`
        ours = {(build_native.CSRC / h).resolve() for h in build_native.DEPS[src] + [build_native.CORE_HEADER]}
        assert {f for f in listed if ROOT in f.parents} == ours | {build_native.CSRC / src}, src


@pytest.fixture(scope="module")
def lib():
    from refiners_amd.build_native import build_native

    build_native()
    return native.load()


@every_header
def test_library_exports_the_header_with_its_types(lib, key, fname):
    for name, (restype, argtypes) in native.ABIS[key].functions.items():
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes, name


def test_prototypes_and_constants_match_pins_written_here(lib):
    i32, i64, ptr = C.c_int32, C.c_int64, C.c_void_p
    assert lib.mi355x_relpos_pack.argtypes == [i32, ptr, i64, ptr, i64, i64, i32, i32, i32, i32, i32, i32, ptr] and lib.mi355x_relpos_pack.restype is C.c_int
    assert lib.mi355x_groupnorm_ws_floats.argtypes == [i32, i32, i32] and lib.mi355x_groupnorm_ws_floats.restype is C.c_int64
    assert lib.mi355x_gemm.argtypes == [C.POINTER(native.GemmArgs), ptr] and lib.mi355x_gemm.restype is C.c_int
    assert lib.mi355x_set_option.argtypes == [C.c_char_p, C.c_int] and lib.mi355x_get_stat.argtypes == [C.c_char_p]  # the unstable entry points, native.UNSTABLE
    assert not set(native.UNSTABLE) & set(native.EXPORTS) and len(native.EXPORTS) == 39
    k = abi.read(native.STRUCT_NAMES).constants
    assert k == {"MI355X_ABI_VERSION": 7, "MI355X_F32": 0, "MI355X_BF16": 1, "MI355X_OK": 0, "MI355X_EDTYPE": -1, "MI355X_ESHAPE": -2, "MI355X_ELAUNCH": -3,
                 "MI355X_EARG": -4, "MI355X_MAX_SEG": 3, "MI355X_MAX_PREFETCH": 2, "MI355X_MD_MAX_TARGETS": 64, "MI355X_MD_SRC_CANVAS": 0, "MI355X_MD_SRC_INIT": 1,
                 "MI355X_MD_FORM_DDIM": 0, "MI355X_MD_FORM_LINEAR": 1, "MI355X_VAE_MAX_AXIS": 1024}
    assert (native.ABI_VERSION, native.MI355X_F32, native.MI355X_BF16, native.MAX_SEG, native.MAX_PREFETCH) == (7, 0, 1, 3, 2)
    assert (native.MD_MAX_TARGETS, native.MD_SRC_CANVAS, native.MD_SRC_INIT, native.VAE_MAX_AXIS) == (64, 0, 1, 1024)
    assert native._ERR == {0: "OK", -1: "EDTYPE", -2: "ESHAPE", -3: "ELAUNCH", -4: "EARG"}


def test_public_names_stay():
    for name in PUBLIC_STRUCTS:
        cls = getattr(native, name)
        assert issubclass(cls, C.Structure) and cls.__name__ == name
    assert sorted(PUBLIC_STRUCTS) == sorted(native.STRUCT_NAMES.values()) and isinstance(native.EXPORTS, list)
    assert "in_" in [n for n, _ in native.SamPostprocessArgs._fields_] and native.SamPostprocessArgs.in_.size == 8
    a = native.GemmArgs()
    a.weight_is_x = True  # recorded programs hang Python-side attributes on the argument structs
    a._sk_keep = (1, 2)
    assert a.weight_is_x is True and a._sk_keep == (1, 2) and C.byref(a)._obj is a
    a.seg[1].k, a.prefetch[1], a.sk_slots = 640, 4096, 256
    assert (a.seg[1].k, a.prefetch[1], a.sk_slots, a.seg[0].x, a.out) == (640, 4096, 256, None, None)
