"""The ctypes binding is read from include/mi355x_refiners.h (refiners_amd/abi.py).  These CPU tests hold the reader to the C compiler's
view of the same header (every size and offset), to its own strictness, and to a few prototypes and constants written out here by hand."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from refiners_amd import abi, native

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "mi355x_refiners.h"

PUBLIC_STRUCTS = """GemmSeg GemmArgs KvStream AttnArgs AttnGeneralArgs LayerNormArgs GroupNormArgs SamAttnArgs SamMaskHeadArgs SamPostprocessArgs AdainStatsArgs
StyleAlignedArgs MdGatherDesc MdGatherArgs MdStepArgs MdBlendDesc MdBlendArgs GroupNormTableArgs GroupNormFixedArgs VaeTilePos VaeGatherArgs VaeAxis VaeBlendTile
VaeBlendArgs""".split()


def _c_compiler() -> str:
    """The host C compiler, or the clang that hipcc drives; none at all fails the test."""
    from refiners_amd.build_native import hipcc_path

    rocm = Path(hipcc_path()).resolve().parent.parent
    for cc in ("cc", "gcc", "clang", rocm / "llvm/bin/clang", rocm / "lib/llvm/bin/clang"):
        if shutil.which(str(cc)):
            return shutil.which(str(cc))
    pytest.fail("no C compiler found (cc, gcc, clang, or the clang next to hipcc)")


def test_c_compiler_agrees_with_ctypes_on_every_layout(tmp_path):
    structs = abi.read(native.STRUCT_NAMES).structs
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'    printf("{cname} - %zu %zu\\n", (size_t)0, sizeof({cname}));')
        for field in cls._c_fields_:
            lines.append(f'    printf("{cname} {field} %zu %zu\\n", offsetof({cname}, {field}), sizeof((({cname}*)0)->{field}));')
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([_c_compiler(), "-std=c99", "-Wall", "-Werror", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    compiled = {(s, f): (int(off), int(size)) for s, f, off, size in (line.split() for line in out.splitlines())}

    ours = {}
    for cname, cls in structs.items():
        assert issubclass(cls, C.Structure) and len(cls._c_fields_) == len(cls._fields_)
        ours[(cname, "-")] = (0, C.sizeof(cls))
        for field, (name, _) in zip(cls._c_fields_, cls._fields_):
            ours[(cname, field)] = (getattr(cls, name).offset, getattr(cls, name).size)
    assert len(structs) == 24 and len(ours) > 24
    assert ours == compiled, {k: (ours.get(k), compiled.get(k)) for k in set(ours) | set(compiled) if ours.get(k) != compiled.get(k)}
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


def test_reader_skips_nothing():
    for text, names in ((GOOD, NAMES), (HEADER.read_text(), native.STRUCT_NAMES)):
        got = abi.parse(text, names)
        code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # counted without the reader: comments mention calls such as mi355x_groupnorm_ws_floats()
        assert len(got.structs) == len(re.findall(r"typedef\s+struct", code)) > 0
        assert len(got.functions) == len(re.findall(r"mi355x_\w+\s*\(", code)) > 0
    assert (len(got.structs), len(got.functions)) == (24, 39)
    short = dict(list(native.STRUCT_NAMES.items())[:-1])
    with pytest.raises(abi.AbiError, match="mi355x_vae_blend_args has no Python name"):
        abi.parse(HEADER.read_text(), short)


@pytest.fixture(scope="module")
def lib():
    from refiners_amd.build_native import build_native

    build_native()
    return native.load()


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
