"""The header readers of espm_amd/_abi.py on small header texts (no library, no device): what a declaration may look like and
still be read, what is refused, and that a changed declaration changes the derived ctypes prototype at that argument."""
import ctypes as C
import importlib.util
import os

import pytest

# the module by its path, as tools/gen_integration.py loads it: importing the package would ask for the built library
_spec = importlib.util.spec_from_file_location("_espm_abi", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "espm_amd", "_abi.py"))
_abi = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_abi)


class _State(C.Structure):
    _fields_ = [("n", C.c_int32)]


SP = C.POINTER(_State)
VP = C.c_void_p


def test_a_prototype_over_three_lines_with_a_comment_between_arguments():
    text = """
    int espm_f(const espm_mu_state* st, int64_t ld, /* leading dimension
                  (elements) */ double tol,   // of the search
               espm_stream_t stream);
    """
    assert _abi.parse_prototypes(text, SP) == {"espm_f": (C.c_int, [SP, C.c_int64, C.c_double, VP])}


def test_stars_on_the_type_on_the_name_and_twice():
    text = "int espm_f(float *a, float* b, espm_xchg** c, const double  * *d, uint8_t * e, espm_mu_state *st, espm_mu_state** sts);"
    res, args = _abi.parse_prototypes("typedef struct espm_xchg espm_xchg;\n" + text, SP)["espm_f"]
    assert res is C.c_int and args == [VP, VP, VP, VP, VP, SP, VP]


def test_an_array_declarator_is_a_pointer():
    res, args = _abi.parse_prototypes("size_t espm_f(const float* rows[], int n_rows, const uint32_t * lists [ ]);", SP)["espm_f"]
    assert res is C.c_size_t and args == [VP, C.c_int, VP]


def test_no_arguments_and_the_return_types():
    text = """
    const char* espm_name(void);
    int espm_count();
    void espm_reset(espm_mu_state* st);
    void* espm_buffer(const espm_mu_state* st, uint32_t which);
    const void *espm_records(int parity);
    int64_t espm_doubles(int n, int64_t count, uint64_t seed, float a, size_t bytes);
    """
    assert _abi.parse_prototypes(text, SP) == {
        "espm_name": (C.c_char_p, []), "espm_count": (C.c_int, []), "espm_reset": (None, [SP]), "espm_buffer": (VP, [SP, C.c_uint32]),
        "espm_records": (VP, [C.c_int]), "espm_doubles": (C.c_int64, [C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_size_t])}
    assert list(_abi.parse_prototypes(text, SP)) == ["espm_name", "espm_count", "espm_reset", "espm_buffer", "espm_records", "espm_doubles"]


def test_struct_and_enum_bodies_and_macros_contribute_nothing():
    text = """
    #define ESPM_DETAIL(d) espm_unpack(d)
    typedef void* espm_stream_t;
    typedef enum espm_status { ESPM_OK = 0, ESPM_EINVAL = -1 } espm_status;
    typedef struct espm_mu_state {
      int32_t espm_n;           /* as in espm_mu_query(st) */
      float* espm_w[2];
      double espm_tol, espm_eps;
    } espm_mu_state;
    int espm_mu_query(espm_mu_state* st);
    """
    assert _abi.parse_prototypes(text, SP) == {"espm_mu_query": (C.c_int, [SP])}


@pytest.mark.parametrize("decl", ["int espm_f(const espm_mu_state* st, unsigned n)",          # a scalar that is not in the vocabulary
                                  "int espm_f(long long n)",
                                  "int espm_f(espm_other* x)",                                 # a struct the header does not declare
                                  "espm_status espm_f(int n)",                                 # an enum by value
                                  "int espm_f(void (*done)(int), int n)",                      # a function pointer
                                  "int espm_f(void x)",
                                  "static inline int espm_f(int n)"])
def test_a_declaration_that_cannot_be_read_is_an_error_that_names_it(decl):
    text = "int espm_before(int n);\n" + decl + ";\nint espm_after(int n);\n"
    with pytest.raises(ValueError, match="espm_f") as err:
        _abi.parse_prototypes(text, SP)
    assert "espm_before" not in str(err.value) and "espm_after" not in str(err.value)


def test_enums_named_and_anonymous():
    text = """
    typedef enum espm_status {
      ESPM_OK = 0,
      ESPM_EINVAL = -1,       /* bad argument */
      ESPM_EHIP = -3,
      ESPM_EUNSUPPORTED = -4  // not built
    } espm_status;
    enum { ESPM_A = 4 /* four */, ESPM_B, ESPM_C, ESPM_D = ESPM_A + 16, ESPM_E, };
    enum { ESPM_FIRST, ESPM_SECOND };
    """
    assert _abi.parse_enums(text) == {"ESPM_OK": 0, "ESPM_EINVAL": -1, "ESPM_EHIP": -3, "ESPM_EUNSUPPORTED": -4,
                                      "ESPM_A": 4, "ESPM_B": 5, "ESPM_C": 6, "ESPM_D": 20, "ESPM_E": 21, "ESPM_FIRST": 0, "ESPM_SECOND": 1}
    with pytest.raises(ValueError, match="ESPM_BAD"):
        _abi.parse_enums("enum { ESPM_BAD = sizeof(int) };")


def test_the_headers_enums():
    e = _abi.parse_enums(_abi.header_text())
    assert [e["ESPM_" + n] for n in ("OK", "EINVAL", "ENOSOLUTION", "EHIP", "EUNSUPPORTED")] == [0, -1, -2, -3, -4]
    assert [e["ESPM_X_" + n] for n in ("F32", "BF16", "U8", "ELL")] == [0, 1, 2, 3]
    assert (e["ESPM_SRC_F32"], e["ESPM_SRC_F64"], e["ESPM_LAYOUT_CM"], e["ESPM_LAYOUT_PM"]) == (0, 1, 0, 1)


def test_predefined_names_win_over_the_headers_defines():
    text = "#ifndef ESPM_KP\n#define ESPM_KP 8\n#endif\n#define ESPM_HS_STRIDE (2 * ESPM_KP)\n"
    assert _abi.parse_defines(text) == {"ESPM_KP": 8, "ESPM_HS_STRIDE": 16}
    assert _abi.parse_defines(text, predefined={"ESPM_KP": 32}) == {"ESPM_KP": 32, "ESPM_HS_STRIDE": 64}
    real = _abi.header_text()
    for kp, strides in ((8, (24, 16, 8)), (16, (40, 32, 16)), (32, (72, 64, 32))):
        d = _abi.parse_defines(real, predefined={"ESPM_KP": kp})
        assert (d["ESPM_HP_STRIDE"], d["ESPM_HS_STRIDE"], d["ESPM_HS_MAX"]) == strides and d["ESPM_MAX_K"] == kp
    assert _abi.parse_defines(real, predefined={"ESPM_KP": 16})["ESPM_HP_STRIDE"] == 40
    assert _abi.parse_defines(real) == _abi.parse_defines(real, predefined={})


def test_a_drifted_declaration_changes_the_prototype_at_that_argument():
    """`int64_t ld` read as `int ld` would hand the launcher half a leading dimension: the derived prototype must follow the header."""
    real = _abi.header_text()
    old = "int espm_mu_laplacian(const float* h, int k, int nx, int ny, int64_t ld, float* out,"
    assert real.count(old) == 1
    before = _abi.parse_prototypes(real, SP)
    after = _abi.parse_prototypes(real.replace(old, old.replace("int64_t ld", "int ld")), SP)
    assert list(before) == list(after)
    changed = [(name, i) for name in before for i, (a, b) in enumerate(zip(before[name][1], after[name][1])) if a is not b]
    assert changed == [("espm_mu_laplacian", 4)]
    assert before["espm_mu_laplacian"][1][4] is C.c_int64 and after["espm_mu_laplacian"][1][4] is C.c_int
    assert all(before[name][0] is after[name][0] and len(before[name][1]) == len(after[name][1]) for name in before)
