"""Which form the W update takes (include/espm_mu.h: espm_mu_w_update_form) - host arithmetic, checked without a GPU.

The launch switches on the same plan the query returns (csrc/mu_w_plan.hpp: plan_w_finish; csrc/mu_api.hip: w_form_ahead), so
what these tests pin is the dispatch itself: one below and one above every boundary of DESIGN.md's table "forms of the W update",
in the three builds, and the `expect` column of tests/w_form_cases.py, which tests/test_gpu_w_update_forms.py then runs.

A state is filled as in tests/test_host_abi_validation.py; its pointers are never read by the plan (any non-NULL value stands for
"given")."""
import ctypes as C

import pytest

import w_form_cases as wc
from w_form_cases import COLUMNS, GENERAL, LOCAL, REGS, SPLIT, TWO

GIVEN = 0x1000   # a pointer that is set; nothing dereferences it


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


def _state(lib, k, n, m=None, simplex_W=False, rows=False, pg=False, bmd=False, no_scratch=False, no_fused=0, p=42):
    st = lib.MUState()
    st.n, st.p, st.k, st.x_dtype = n, p, k, lib.X_F32
    handle = lib.variant(k).lib
    assert handle.espm_mu_query(C.byref(st)) == 0
    st.xscale, st.log_shift, st.no_fused = 1.0, 1e-14, no_fused
    if m:
        st.m, st.g, st.g_t, st.colsum_g = m, GIVEN, GIVEN, GIVEN
    st.simplex_w = int(simplex_W)
    st.simplex_rows = GIVEN if rows else None
    st.pg_gamma_w = 3.0 if pg else 0.0
    if bmd:
        st.breg_sr_px = st.breg_sr_ch = GIVEN
    st.w_scratch = None if no_scratch else GIVEN
    return handle, st


def _form(lib, k, n, m=None, **kw):
    handle, st = _state(lib, k, n, m, **kw)
    detail = C.c_int(-1)
    rc = handle.espm_mu_w_update_form(C.byref(st), C.byref(detail))
    assert rc > 0, (rc, handle.espm_mu_last_error())
    assert handle.espm_mu_w_update_form(C.byref(st), None) == rc          # detail may be NULL
    assert (rc == lib.W_FORMS_BY_NAME[LOCAL]) == (handle.espm_mu_w_update_is_local(C.byref(st)) == 1)
    d = lib.w_form_detail(detail.value)
    return lib.W_FORMS[rc], (d["threads"], d["rows"], d["channels"], d["gta_all_threads"]) if d else None


def _opts(opt):
    return dict(simplex_W=opt.get("simplex_W", False), rows=opt.get("rows", False), pg=opt.get("algo") == "pg",
                bmd=opt.get("algo") == "bmd", no_scratch=opt.get("no_scratch", False))


@pytest.mark.parametrize("case", wc.CASES, ids=[c["id"] for c in wc.CASES])
def test_the_gpu_table_expects_what_the_plan_answers(lib, case):
    assert _form(lib, case["k"], case["n"], case["m"], **_opts(case["opt"])) == (case["form"], case["detail"])


def test_the_gpu_table_reaches_every_form_of_every_build():
    """The same completeness the GPU file asserts, here on the table alone."""
    for kp in (8, 16, 32):
        seen = {(c["form"], c["detail"]) for c in wc.CASES if wc.build_of(c["k"]) == kp}
        assert seen == wc.reachable(kp), (kp, wc.reachable(kp) ^ seen)


def test_detail_packing(lib):
    """include/espm_mu.h: bits 0..11 threads, 12..15 rows, 16..19 channels, bit 20 the all-threads G^T A; 0 for every other form."""
    handle, st = _state(lib, 3, 1500, 9, simplex_W=True)
    detail = C.c_int(-1)
    assert handle.espm_mu_w_update_form(C.byref(st), C.byref(detail)) == lib.W_FORMS_BY_NAME[REGS]
    assert detail.value == 1024 | 1 << 12 | 2 << 16 | 1 << 20
    handle, st = _state(lib, 5, 1030, 17)
    assert handle.espm_mu_w_update_form(C.byref(st), C.byref(detail)) == lib.W_FORMS_BY_NAME[COLUMNS] and detail.value == 0
    assert sorted(lib.W_FORMS) == [1, 2, 3, 4, 5, 6]


def test_refused_states(lib):
    """A negative status, not a form: a struct the library cannot read, and the two combinations the state check refuses - which is why the
    GPU table has no Bregman row at 4097 channels and no projected-gradient row with the simplex over W."""
    handle, st = _state(lib, 5, 4097, bmd=True, no_scratch=True)
    assert handle.espm_mu_w_update_form(C.byref(st), None) == lib.EINVAL and b"Bregman" in handle.espm_mu_last_error()
    handle, st = _state(lib, 5, 1000, pg=True, simplex_W=True)
    assert handle.espm_mu_w_update_form(C.byref(st), None) == lib.EINVAL and b"projected-gradient" in handle.espm_mu_last_error()
    # the general one-workgroup finish keeps the numerators and denominators of an update in w_scratch: a state that withholds the
    # workspace (which takes G = identity off the local update) is refused there BEFORE the launch - it used to write through NULL
    for kk, n in ((5, 4097), (20, 63)):
        handle, st = _state(lib, kk, n, pg=True, no_scratch=True)
        assert handle.espm_mu_w_update_form(C.byref(st), None) == lib.W_FORMS_BY_NAME[GENERAL]
        assert handle.espm_mu_w_finish(C.byref(st), 0, 0, -1, None) == lib.EINVAL and b"needs w_scratch" in handle.espm_mu_last_error()
    st = lib.MUState()
    st.struct_size += 8
    assert lib.lib.espm_mu_w_update_form(C.byref(st), None) == lib.EINVAL
    handle, st = _state(lib, 5, 100)
    assert lib.variant(12).lib.espm_mu_w_update_form(C.byref(st), None) == lib.EUNSUPPORTED   # k = 5 handed to the 9..16 build


# k of the build under test: 1..8, 9..16, 17..32
BUILDS = [pytest.param(8, 5, id="kp8"), pytest.param(16, 12, id="kp16"), pytest.param(32, 20, id="kp32")]


@pytest.mark.parametrize("kp,k", BUILDS)
def test_edges_of_the_forms_ahead_of_the_finish(lib, kp, k):
    """Local update and simplex split (mu_api.hip: w_form_ahead): n = 63 / 64, n_pad % 32, the constraints that leave the split, the
    workspace, no_fused = 1.  Below them the one-workgroup finish: register-resident where built, else general."""
    one_wg = GENERAL if kp == 32 else REGS
    assert _form(lib, k, 64)[0] == LOCAL and _form(lib, k, 63)[0] == one_wg
    assert _form(lib, k, 64, no_scratch=True)[0] == one_wg
    assert _form(lib, k, 64, pg=True)[0] == LOCAL and _form(lib, k, 64, bmd=True)[0] == LOCAL
    assert _form(lib, k, 64, no_fused=1)[0] == LOCAL
    assert _form(lib, k, 64, simplex_W=True)[0] == SPLIT and _form(lib, k, 63, simplex_W=True)[0] == one_wg
    assert _form(lib, k, 96, simplex_W=True)[0] == SPLIT           # n_pad = 96
    assert _form(lib, k, 97, simplex_W=True)[0] == one_wg          # n_pad = 104
    assert _form(lib, k, 70, simplex_W=True)[0] == one_wg          # n_pad = 72
    assert _form(lib, k, 96, simplex_W=True, rows=True)[0] == one_wg
    assert _form(lib, k, 96, simplex_W=True, no_scratch=True)[0] == one_wg
    assert _form(lib, k, 96, simplex_W=True, no_fused=1)[0] == one_wg
    assert _form(lib, k, 5024, simplex_W=True)[0] == SPLIT         # (no upper edge)


@pytest.mark.parametrize("kp,k", BUILDS)
def test_edges_of_the_dictionary_forms(lib, kp, k):
    """Column form: m <= 32 and n_pad <= 2048.  Two launches: no simplex / projected gradient, m k <= 8192, and 2 m k floats of workspace
    that hold ceil(n_pad / 256) KP doubles + 16 bytes."""
    assert _form(lib, k, 2048, 32)[0] == COLUMNS and _form(lib, k, 2049, 32)[0] == TWO
    assert _form(lib, k, 2048, 33)[0] == TWO
    assert _form(lib, k, 2041, 32)[0] == COLUMNS                   # n_pad = 2048
    for kw in (dict(simplex_W=True), dict(pg=True), dict(no_scratch=True)):
        assert _form(lib, k, 300, 20, **kw)[0] in (REGS, GENERAL), kw
    # m k = 8192 / above (k = 8: m = 1024 / 1025; k = 16: 512 / 513; k = 32: 256 / 257)
    kk = kp
    assert _form(lib, kk, 300, 8192 // kk)[0] == TWO and _form(lib, kk, 300, 8192 // kk + 1)[0] == GENERAL
    # the workspace condition 8 m k >= nwg KP 8 + 16 at m = 33 (no column form), k as small as the build has
    kmin = {8: 1, 16: 9, 32: 17}[kp]
    nwg = (8 * 33 * kmin - 16) // (8 * kp)                          # the most row workgroups whose partials fit
    assert _form(lib, kmin, 256 * nwg, 33)[0] == TWO
    assert _form(lib, kmin, 256 * nwg + 1, 33)[0] in (REGS, GENERAL)
    if kp == 8:   # the two rows of the issue: 5000 channels
        assert _form(lib, 5, 5000, 33)[0] == TWO and _form(lib, 3, 5000, 9)[0] == GENERAL


@pytest.mark.parametrize("kp,k", BUILDS[:2])
def test_edges_of_the_register_resident_finish(lib, kp, k):
    """Threads, rows and channels per thread, the G^T A switch at m k = 512, the 64 KB of LDS, m k = 8192, n_cm = 4096 / 4112."""
    sw = dict(simplex_W=True)
    few = 512 if kp == 8 else 1024                                  # G = identity, k <= 8, n_cm <= 2048: 512 threads
    R = dict(simplex_W=True, rows=True)
    assert _form(lib, k, few, **R) == (REGS, (few, 1, 1, False)) and _form(lib, k, few + 1, **R) == (REGS, (few, 2, 2, False))
    assert _form(lib, k, 2 * few, **R) == (REGS, (few, 2, 2, False)) and _form(lib, k, 2 * few + 1, **R) == (REGS, (few, 4, 4, False))
    assert _form(lib, k, 2048, **R)[1][0] == few and _form(lib, k, 2049, **R) == (REGS, (1024, 4, 4, False))
    assert _form(lib, k, 4096, **R) == (REGS, (1024, 4, 4, False)) and _form(lib, k, 4097, **R) == (GENERAL, None)
    # dictionary: channels per thread by n_cm, one row of W per thread
    all_t = kp == 8
    for n, c in ((1024, 1), (1025, 2), (2048, 2), (2049, 4), (4096, 4)):
        assert _form(lib, k, n, 9, **sw) == (REGS, (1024, 1, c, all_t)), n
    assert _form(lib, k, 4097, 9, **sw) == (GENERAL, None)
    if kp == 8:
        assert _form(lib, 8, 300, 64, **sw) == (REGS, (1024, 1, 1, True)) and _form(lib, 8, 300, 65, **sw) == (REGS, (1024, 1, 1, False))
        assert _form(lib, 5, 300, 1260, **sw) == (REGS, (1024, 2, 2, False)) and _form(lib, 5, 300, 1261, **sw) == (GENERAL, None)
        assert _form(lib, 3, 300, 2049, **sw) == (REGS, (1024, 4, 4, False))     # 57372 bytes
        assert _form(lib, 3, 3000, 1500, **sw) == (REGS, (1024, 4, 4, False))    # two rows, three channels per thread: the instance of four
        assert _form(lib, 8, 300, 1024, **sw) == (REGS, (1024, 1, 1, False))     # m k = 8192 and exactly 64 KB of LDS
        assert _form(lib, 8, 300, 1025, **sw) == (GENERAL, None)                 # m k = 8200
        assert _form(lib, 1, 300, 3276, **sw) == (REGS, (1024, 4, 4, False)) and _form(lib, 1, 300, 3277, **sw) == (GENERAL, None)   # 65520 / 65540 bytes
    else:
        assert _form(lib, 9, 300, 56, **sw) == (REGS, (1024, 1, 1, False))       # m k = 504 <= 512 but k > 8: one wave per entry


def test_the_widest_build_has_the_general_finish_only(lib):
    for n, m, kw in ((63, None, {}), (300, None, dict(simplex_W=True, rows=True)), (150, 9, dict(simplex_W=True)), (4097, 9, dict(simplex_W=True))):
        assert _form(lib, 20, n, m, **kw) == (GENERAL, None)
