"""The C ABI as include/espm_mu.h declares it - the layout of `espm_mu_state`, the #define constants, the enums and the prototype
of every function: the one parser the ctypes binding (espm_amd/_lib.py), the integration notes and the tests
share.  The header is the single description of the ABI; nothing of it is copied by hand.

    python -m espm_amd._abi            # the ctypes field list of the header, as Python source (INTEGRATION.md's block)
    python -m espm_amd._abi --c-names  # the field names, for espm_mu_state_layout() in csrc/mu_api.hip
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

# The repository's include/espm_mu.h (the one hand-kept copy); an installed package carries a copy of it next to the library
# (espm_amd/include/espm_mu.h, placed there by __graft_entry__.build() and listed in pyproject.toml's package-data).
_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO_HEADER = os.path.join(os.path.dirname(_HERE), "include", "espm_mu.h")
HEADER = _REPO_HEADER if os.path.exists(_REPO_HEADER) else os.path.join(_HERE, "include", "espm_mu.h")

_SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
            "double": C.c_double, "int": C.c_int, "size_t": C.c_size_t}


@functools.lru_cache(maxsize=2)   # every reader below starts here: the binding strips its one header text once
def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _int_expr(expr, names):
    """An integer expression over the names seen so far -> int, or None for anything else."""
    if not re.fullmatch(r"[\w\s()+\-*/<>]+", expr):
        return None
    try:
        return int(eval(expr, {"__builtins__": {}}, dict(names)))
    except Exception:
        return None


def parse_defines(text, predefined=None):
    """#define NAME <integer expression of earlier defines> -> {NAME: int}; everything else is skipped.  A name in `predefined`
    keeps that value whatever the header defines it as, which is what -DNAME=value does to an #ifndef NAME: the sizes that
    follow ESPM_KP in a wide build are parse_defines(text, {"ESPM_KP": 16})."""
    fixed = dict(predefined or {})
    out = dict(fixed)
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(.+?)[ \t]*$", _strip_comments(text), flags=re.M):
        value = None if m.group(1) in fixed else _int_expr(m.group(2), out)
        if value is not None:
            out[m.group(1)] = value
    return out


def parse_enums(text):
    """{enumerator: int} of every enum of the header, named or anonymous; an enumerator without a value is its predecessor + 1."""
    out = {}
    for body in re.findall(r"\benum\b\s*\w*\s*\{(.*?)\}", _strip_comments(text), flags=re.S):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            m = re.fullmatch(r"(\w+)\s*(?:=(.+))?", item, flags=re.S)
            if m:
                value = value + 1 if m.group(2) is None else _int_expr(m.group(2), out)
            if not m or value is None:
                raise ValueError(f"cannot parse enumerator {item!r}")
            out[m.group(1)] = value
    return out


def parse_prototypes(text, state_pointer):
    """{function: (restype, [argtypes])} in declaration order, for every function the header declares: what ctypes needs to call it.
    Scalars are themselves and espm_stream_t is c_void_p; a void return is None and a `const char*` return c_char_p; a pointer to
    espm_mu_state is `state_pointer` and every other pointer, `T**` and `T* name[]` included, is c_void_p.  A declaration that
    looks like one of the library's functions and cannot be read - an unknown type, a function-pointer argument - is a ValueError."""
    text = re.sub(r"^[ \t]*#[^\n]*", " ", _strip_comments(text), flags=re.M)            # preprocessor lines
    text = re.sub(r"\{[^{}]*\}", " ", re.sub(r'extern\s*"C"\s*\{', " ", text))          # bodies of struct {...} / enum {...}
    structs = re.findall(r"\btypedef\s+struct\s+(\w+)", text)                            # espm_xchg: opaque, only ever pointed to
    pointees = set(_SCALARS) | {"void", "char", "uint8_t", "espm_stream_t", "espm_mu_state"} | set(structs)

    def ctype(spelling, decl, returned=False):
        spaced = " ".join(re.sub(r"\[\s*\]", " [] ", spelling.replace("*", " * ")).split())   # "const T * * name []"
        m = re.fullmatch(r"(const )?(\w+)((?: \*)*)(?: \w+)?( \[\])?", spaced)
        if not m:
            raise ValueError(f"cannot parse {spelling.strip()!r} in the declaration {decl!r}")
        const, base, stars = m.group(1), m.group(2), m.group(3).count("*") + bool(m.group(4))
        if stars and base in pointees:
            if stars == 1 and base == "espm_mu_state":
                return state_pointer
            return C.c_char_p if returned and const and base == "char" and stars == 1 else C.c_void_p
        if not stars and base in _SCALARS:
            return _SCALARS[base]
        if not stars and base == "espm_stream_t":
            return C.c_void_p
        if not stars and base == "void" and returned:
            return None
        raise ValueError(f"unknown type {base!r} in the declaration {decl!r}")

    out = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not re.search(r"\bespm_\w+ ?\(", decl):
            continue
        m = re.fullmatch(r"(.+?) ?\b(espm_\w+) ?\(([^()]*)\)", decl)
        if not m:
            raise ValueError(f"cannot parse the declaration {decl!r}")
        args = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        out[m.group(2)] = (ctype(m.group(1), decl, returned=True), [ctype(a, decl) for a in args])
    return out


def parse_struct(text, name="espm_mu_state"):
    """[(field, ctypes type)] in declaration order.  Pointers of any kind are c_void_p; `T* f[2]` is c_void_p * 2."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), _strip_comments(text), flags=re.S)
    if not body:
        raise ValueError(f"struct {name} not found")
    fields = []
    for decl in body.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"(const )?(\w+)( ?\*)? ?(.+)", decl)
        if not m:
            raise ValueError(f"cannot parse declaration {decl!r}")
        base, is_ptr = m.group(2), bool(m.group(3))
        for item in m.group(4).split(","):
            item = item.strip()
            ptr = is_ptr
            if item.startswith("*"):
                ptr, item = True, item[1:].strip()
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", item)
            fname, count = (arr.group(1), int(arr.group(2))) if arr else (item, 0)
            if not re.fullmatch(r"\w+", fname):
                raise ValueError(f"cannot parse declarator {item!r} in {decl!r}")
            if ptr:
                ct = C.c_void_p
            elif base in _SCALARS:
                ct = _SCALARS[base]
            else:
                raise ValueError(f"unknown type {base!r} in {decl!r}")
            fields.append((fname, ct * count if count else ct))
    return fields


def header_text(path=HEADER):
    with open(path) as f:
        return f.read()


def layout_string(struct_type):
    """The same text espm_mu_state_layout() returns, from a ctypes Structure."""
    return "".join(f"{n}:{getattr(struct_type, n).offset}:{getattr(struct_type, n).size};" for n, _ in struct_type._fields_)


def ctypes_source(fields):
    names = {C.c_int: "c_int", C.c_size_t: "c_size_t", C.c_void_p: "c_void_p", C.c_int32: "c_int32", C.c_uint32: "c_uint32",
             C.c_int64: "c_int64", C.c_uint64: "c_uint64", C.c_float: "c_float", C.c_double: "c_double"}
    lines = ["class MUState(ctypes.Structure):", "    _fields_ = ["]
    for n, t in fields:
        if hasattr(t, "_length_"):
            lines.append(f'        ("{n}", ctypes.{names[t._type_]} * {t._length_}),')
        else:
            lines.append(f'        ("{n}", ctypes.{names[t]}),')
    lines.append("    ]")
    return "\n".join(lines)


if __name__ == "__main__":
    import sys
    fs = parse_struct(header_text())
    if "--c-names" in sys.argv:
        print(" ".join(f"F({n})" for n, _ in fs))
    else:
        print(ctypes_source(fs))
