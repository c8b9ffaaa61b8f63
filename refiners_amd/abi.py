"""The C ABI as ctypes, read from include/mi355x_refiners.h: its integer constants, one `ctypes.Structure` per `typedef struct`
and (restype, argtypes) of every prototype.  The header is the only description of the ABI; refiners_amd.native binds what this
module reads and restates none of it.

The reader knows the C the header is written in and nothing more: `#define NAME <integer>`, `enum { NAME = <integer>, ... };`,
`typedef struct [tag] { <fields> } name;` and `int | int64_t mi355x_name(<parameters>);`.  It is strict: text that is none of
these, or a field / parameter it cannot translate completely, raises AbiError with the header line.  Nothing is skipped.
"""
from __future__ import annotations

import ctypes as C
import keyword
import re
from pathlib import Path
from typing import NamedTuple, Optional

HEADER = Path(__file__).resolve().parent / "../include/mi355x_refiners.h"

_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "int": C.c_int}
_INT = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)"
_STATEMENT = re.compile(
    r"enum\s*\{(?P<enum>[^{}]*)\}\s*;"
    r"|typedef\s+struct\s*\w*\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)\s*;"
    r"|(?P<ret>\w+)\s+(?P<func>\w+)\s*\((?P<params>[^()]*)\)\s*;"
)
_PREPROCESSOR = re.compile(rf'#\s*(?:define\s+(?P<name>\w+)\s+(?P<value>{_INT})|define\s+\w+|ifndef\s+\w+|endif|include\s*<\w+\.h>|include\s*"mi355x_refiners\.h")\s*')
_FIELD = re.compile(r"(?P<const>const\s+)?(?P<type>\w+)(?:\s*(?P<ptr>\*)\s*|\s+)(?P<names>[^*\s].*)", re.S)
_DECLARATOR = re.compile(r"(?P<name>[A-Za-z_]\w*)\s*(?:\[\s*(?P<dim>\w+)\s*\])?")
_SPACE = re.compile(r"\s*")
_PARAM = re.compile(r"(?P<const>const\s+)?(?P<type>\w+)(?:\s*(?P<ptr>\*)\s*|\s+)(?P<name>[A-Za-z_]\w*)")


class AbiError(ValueError):
    """The header holds something the reader cannot translate."""


class Abi(NamedTuple):
    constants: dict  # NAME -> int, every #define and enumerator
    enums: list  # one {NAME: int} per enum, in header order
    structs: dict  # C name -> ctypes.Structure subclass, in header order
    functions: dict  # C name -> (restype, [argtypes]), in header order


def _blank(m: re.Match) -> str:
    return " " + "\n" * m.group().count("\n")  # the text keeps its lines, so a position still names the header line


def parse(text: str, names: dict, where: str = "header", base: Optional[Abi] = None) -> Abi:
    """`names`: C struct name -> name of the Python class; a struct the header declares and `names` lacks is an error.
    `base`: what the reader got from mi355x_refiners.h, for an extension header that includes it: its structs and constants may be
    used (the same classes, so that a pointer to one is the type the main header's prototypes take) and are not listed again."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", _blank, text, flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", _blank, text, flags=re.S)  # `extern "C" {` and its `}`: not C
    abi = Abi({}, [], {}, {})
    structs = dict(base.structs) if base else {}  # every struct a field or parameter may name: the base header's, then this header's own
    constants = dict(base.constants) if base else {}

    def fail(pos: int, why: str) -> AbiError:
        return AbiError(f"{where}:{text.count(chr(10), 0, pos) + 1}: {why}")

    def directive(m: re.Match) -> str:
        d = _PREPROCESSOR.fullmatch(m.group())
        if not d:
            raise fail(m.start(), f"unknown preprocessor line {m.group().strip()!r}")
        if d["name"]:
            abi.constants[d["name"]] = constants[d["name"]] = int(d["value"], 0)
        return _blank(m)

    text = re.sub(r"^[ \t]*#[^\n]*", directive, text, flags=re.M)

    def known(tname: str, pos: int) -> None:
        if tname not in _SCALARS and tname not in structs and tname not in ("void", "char"):
            raise fail(pos, f"unknown type {tname!r}")

    def fields(body: str, at: int) -> tuple[list, list]:
        out, c_names = [], []
        for d in re.finditer(r"[^;]+", body):
            if not d.group().strip():
                continue
            pos = at + d.start() + len(d.group()) - len(d.group().lstrip())
            f = _FIELD.fullmatch(d.group().strip())
            if not f:
                raise fail(pos, f"unparseable field {d.group().strip()!r}")
            known(f["type"], pos)
            declarators = [s.strip() for s in f["names"].split(",")]
            if (f["ptr"] and len(declarators) > 1) or (not f["ptr"] and f["type"] in ("void", "char")):
                raise fail(pos, "a pointer field is declared alone, and void / char only behind a pointer")
            for s in declarators:
                n = _DECLARATOR.fullmatch(s)
                if not n:
                    raise fail(pos, f"unparseable declarator {s!r}")
                t = C.c_void_p if f["ptr"] else _SCALARS.get(f["type"]) or structs[f["type"]]
                if n["dim"]:
                    if not n["dim"].isdigit() and n["dim"] not in constants:
                        raise fail(pos, f"array dimension {n['dim']!r} is neither a literal nor a #define")
                    t = t * (int(n["dim"]) if n["dim"].isdigit() else constants[n["dim"]])
                c_names.append(n["name"])
                out.append((n["name"] + "_" * keyword.iskeyword(n["name"]), t))
        return out, c_names

    def params(body: str, pos: int) -> list:
        out = []
        for s in [] if body.strip() == "void" else body.split(","):
            p = _PARAM.fullmatch(s.strip())
            if not p:
                raise fail(pos, f"unparseable parameter {s.strip()!r}")
            known(p["type"], pos)
            if p["ptr"]:
                out.append(C.c_char_p if p["type"] == "char" else C.POINTER(structs[p["type"]]) if p["const"] and p["type"] in structs else C.c_void_p)
            elif p["type"] in _SCALARS:
                out.append(_SCALARS[p["type"]])
            else:
                raise fail(pos, f"parameter {s.strip()!r} is passed by value and is no scalar")
        return out

    pos = 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return abi
        m = _STATEMENT.match(text, pos)
        if not m:
            raise fail(pos, f"not an enum, a typedef struct or a prototype: {text[pos:].split(chr(10), 1)[0].strip()!r}")
        if m["enum"] is not None:
            abi.enums.append({})
            for e in filter(str.strip, m["enum"].split(",")):
                em = re.fullmatch(rf"\s*(\w+)\s*=\s*({_INT})\s*", e)
                if not em:
                    raise fail(pos, f"enumerator {e.strip()!r} has no integer value")
                abi.constants[em[1]] = abi.enums[-1][em[1]] = constants[em[1]] = int(em[2], 0)
        elif m["struct"]:
            if m["struct"] not in names:
                raise fail(pos, f"struct {m['struct']} has no Python name")
            fl, c_names = fields(m["fields"], m.start("fields"))
            abi.structs[m["struct"]] = structs[m["struct"]] = type(names[m["struct"]], (C.Structure,), {"_fields_": fl, "_c_fields_": tuple(c_names)})
        else:
            if m["ret"] not in ("int", "int64_t") or not m["func"].startswith("mi355x_"):
                raise fail(pos, f"prototype {m['ret']} {m['func']}(...) is not `int | int64_t mi355x_*`")
            abi.functions[m["func"]] = (_SCALARS[m["ret"]], params(m["params"], pos))
        pos = m.end()


def read(names: dict, path: Optional[Path] = None, base: Optional[Abi] = None) -> Abi:
    path = Path(path or HEADER)
    return parse(path.read_text(), names, where=path.name, base=base)


def read_all(headers: list, include: Path = HEADER.parent) -> dict:
    """`headers`: rows (key, file name, {C struct: Python class name}), mi355x_refiners.h first -> {key: Abi}; every later header is read
    with the first as `base`.  A C struct, a Python class or a function that two headers declare raises AbiError with both headers' names:
    the binding merges what the headers declare, and the later one would silently win."""
    abis: dict = {}
    owner: dict = {}
    for key, fname, names in headers:
        got = abis[key] = read(names, include / fname, base=next(iter(abis.values()), None))
        for name in [*got.structs, *(cls.__name__ for cls in got.structs.values()), *got.functions]:
            if owner.setdefault(name, fname) != fname:
                raise AbiError(f"{fname}: {name} is already declared by {owner[name]}")
    return abis
