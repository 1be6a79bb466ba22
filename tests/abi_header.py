"""The tests' own reading of the function declarations in include/espm_mu.h: one regex per declaration and a table from the
C spellings to ctypes.  It shares no code with espm_amd/_abi.py (parse_prototypes), which the binding is derived with: the
two readings of the header must agree (tests/test_host_cpu.py), and that is only worth something while they stay separate."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "espm_mu.h")
_PROTOTYPE = r"^(\w[\w \*]*?) *\b(%s)\s*\(([^)]*)\)\s*;"


def _text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _spelling(arg):
    """`const double *  h` -> `const double*`: the type of one parameter, stars attached, without its name."""
    *words, last = arg.split()
    return " ".join(words) + "*" * last.count("*") + ("[]" if last.endswith("]") else "")


def declared_functions():
    """Every function the header declares, in its order."""
    return [m.group(2) for m in re.finditer(_PROTOTYPE % r"espm_\w+", _text(), flags=re.M)]


def _declared(name):
    """(return type, [parameter types]) of ``name`` in include/espm_mu.h, as C spellings."""
    m = re.search(_PROTOTYPE % re.escape(name), _text(), flags=re.M)
    assert m, name
    args = m.group(3).strip()
    return m.group(1).strip(), [] if args in ("", "void") else [_spelling(a) for a in args.split(",")]


# every spelling of a type in the header's declarations but the two of the state (`signature` below); a new one is a KeyError here
CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float,
         "double": C.c_double, "espm_stream_t": C.c_void_p, "const char*": C.c_char_p,
         **{pointer: C.c_void_p for pointer in (
             "void*", "const void*", "float*", "const float*", "double*", "const double*", "int*", "int32_t*", "const int32_t*",
             "uint32_t*", "const uint32_t*", "int64_t*", "const int64_t*", "uint64_t*", "uint8_t*", "const uint8_t*",
             "espm_xchg*", "const espm_xchg*", "espm_xchg**")}}


def signature(name, state_pointer):
    """(restype, [argtypes]) that ctypes must hold for ``name``: CTYPE, and ``state_pointer`` for a pointer to espm_mu_state."""
    ctype = dict(CTYPE, **{"espm_mu_state*": state_pointer, "const espm_mu_state*": state_pointer})
    res, args = _declared(name)
    return ctype[res], [ctype[a] for a in args]
