"""Pixel binning without a device: the numpy reference against the reference's own form of the estimate (tests/binning_reference.py),
the binding, the argument checks of the entry points that come before any launch, the wide builds' stubs, and what ``fit_binned``
refuses before anything is uploaded."""
import ctypes as C

import numpy as np
import pytest

from abi_header import CTYPE, _declared
import binning_reference as br


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


# ---- the reference itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bin", [(1, 1), (2, 2), (4, 4), (8, 3), (2, 12), (16, 24)])
def test_closed_form_equals_the_direct_form(bin):
    """The four sums give what eds_spim.py:782-793 computes on explicit arrays, for factors that divide the image: relative 1e-10
    (of the terms the bias is made of: it cancels to 0 for (1, 1))."""
    shape = (16, 24)
    for seed in range(3):
        X, _, _ = br.block_image(70, shape, 4, seed=seed)
        T1, T2, A, Cs = br.sums(X, shape, [bin])
        var, bias, risk = (v[0] for v in br.risk(T1, T2, A, Cs, 70, shape))
        dvar, dbias, drisk = br.direct(X, shape, bin)
        scale = (T2 + T1 + A[0] + Cs[0]) / (70 * 16 * 24)
        assert abs(var - dvar) <= 1e-10 * dvar
        assert abs(bias - dbias) <= 1e-10 * scale
        assert abs(risk - drisk) <= 1e-10 * (scale + abs(drisk))


def test_reference_rebin_ragged():
    X = np.arange(2 * 15, dtype=np.float64).reshape(2, 15)   # 3 x 5 pixels
    S, ng = br.rebin(X, (3, 5), (2, 2))
    assert S.shape == (2, 6) and list(ng) == [4, 4, 2, 2, 2, 1]
    assert S[0, 0] == 0 + 1 + 5 + 6 and S[0, 2] == 4 + 9 and S[0, 5] == 14 and S[1, 5] == 29
    assert np.array_equal(br.rebin_exact(X.astype(np.uint8), (3, 5), (2, 2)), S.astype(np.int64))
    S, ng = br.rebin(X, (3, 5), (64, 128))
    assert S.shape == (2, 1) and ng[0] == 15 and S[1, 0] == X[1].sum()


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["espm_rebin_pixels", "espm_binning_sums", "espm_binning_sums_scratch"])
def test_symbols_are_bound_with_the_headers_signatures(lib, name):
    res, args = lib.SYMBOLS[name]
    cres, cargs = _declared(name)
    assert res is CTYPE[cres]
    assert list(args) == [CTYPE[a] for a in cargs]
    assert hasattr(lib.lib, name)


def test_header_and_packaged_copy_carry_the_tile_sizes(lib):
    import os

    from espm_amd import _abi
    d = _abi.parse_defines(_abi.header_text())
    assert d["ESPM_BIN_BLOCK"] == lib.BIN_BLOCK == 256 and d["ESPM_BIN_PARTS"] == lib.BIN_PARTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert open(os.path.join(root, "include", "espm_mu.h")).read() == open(os.path.join(root, "espm_amd", "include", "espm_mu.h")).read()


def test_scratch_query(lib):
    q = lib.lib.espm_binning_sums_scratch
    slabs = 128 * lib.BIN_PARTS   # the buffer of the pixel-major slabs, behind the slots
    assert q(70, 13, 10, 1) == (4 * lib.BIN_PARTS + slabs) * 8
    assert q(2048, 512, 512, 256) == ((2 + 512) * lib.BIN_PARTS + slabs) * 8
    assert q(0, 13, 10, 1) == 0 and q(70, 0, 10, 1) == 0 and q(70, 13, 0, 1) == 0 and q(70, 13, 10, 0) == 0


def _rebin(f, x, dtype, layout, ld, n, ny, nx, by, bx, out, odt, old):
    return f(x, dtype, layout, ld, n, ny, nx, by, bx, out, odt, old, None)


def test_rebin_argument_errors_need_no_device(lib):
    f = lib.lib.espm_rebin_pixels
    one = C.c_void_p(8)   # (never dereferenced: every call below is refused on the host)
    F32, F64 = lib.DIAG_X_F32, lib.DIAG_X_F64
    assert _rebin(f, None, 0, 0, 80, 8, 8, 10, 2, 2, None, F32, 20) == lib.EINVAL      # the null call
    assert _rebin(f, None, 0, 0, 80, 8, 8, 10, 2, 2, one, F32, 20) == lib.EINVAL
    assert _rebin(f, one, 0, 0, 80, 8, 8, 10, 2, 2, None, F32, 20) == lib.EINVAL
    assert _rebin(f, one, 0, 0, 80, 8, 8, 10, 0, 2, one, F32, 20) == lib.EINVAL        # by < 1
    assert b"(0, 2)" in lib.lib.espm_mu_last_error()
    assert _rebin(f, one, 0, 0, 80, 8, 8, 10, 2, -1, one, F32, 20) == lib.EINVAL
    assert _rebin(f, one, 4, 0, 80, 8, 8, 10, 2, 2, one, F32, 20) == lib.EINVAL        # a dtype code that does not exist
    assert b"x_dtype 4" in lib.lib.espm_mu_last_error()
    assert _rebin(f, one, -1, 0, 80, 8, 8, 10, 2, 2, one, F32, 20) == lib.EINVAL
    assert _rebin(f, one, 0, 0, 80, 8, 8, 10, 2, 2, one, lib.DIAG_X_U8, 20) == lib.EINVAL   # the output is f32 or f64
    assert _rebin(f, one, 0, 2, 80, 8, 8, 10, 2, 2, one, F64, 20) == lib.EINVAL        # layout
    assert _rebin(f, one, 0, 0, 79, 8, 8, 10, 2, 2, one, F64, 20) == lib.EINVAL        # ld below the 80 pixels of a row
    assert b"ld=79" in lib.lib.espm_mu_last_error()
    assert _rebin(f, one, 0, 1, 7, 8, 8, 10, 2, 2, one, F64, 8) == lib.EINVAL          # pixel-major: rows of n
    assert _rebin(f, one, 0, 0, 80, 8, 8, 10, 2, 2, one, F64, 19) == lib.EINVAL        # out_ld below the 4 x 5 bins
    assert b"out_ld=19" in lib.lib.espm_mu_last_error()
    assert _rebin(f, one, 0, 0, 80, 0, 8, 10, 2, 2, one, F64, 20) == lib.EINVAL
    assert _rebin(f, one, 0, 0, 80, 8, 0, 10, 2, 2, one, F64, 20) == lib.EINVAL
    assert _rebin(f, one, 0, 0, 1 << 40, 8, 1 << 16, 1 << 15, 2, 2, one, F64, 1 << 40) == lib.EINVAL   # 2^31 pixels


def _sums(f, x, dtype, layout, ld, n, ny, nx, bins, n_bins, out, scratch, nbytes):
    arr = None if bins is None else (C.c_int32 * (2 * len(bins)))(*[v for b in bins for v in b])
    return f(x, dtype, layout, ld, n, ny, nx, arr, n_bins, out, scratch, nbytes, None)


def test_binning_sums_argument_errors_need_no_device(lib):
    f = lib.lib.espm_binning_sums
    one = C.c_void_p(8)
    big = 1 << 30
    bins = [(1, 1), (2, 3)]
    assert _sums(f, None, 0, 0, 80, 8, 8, 10, None, 0, None, None, 0) == lib.EINVAL    # the null call
    assert _sums(f, None, 0, 0, 80, 8, 8, 10, bins, 2, one, one, big) == lib.EINVAL
    assert _sums(f, one, 0, 0, 80, 8, 8, 10, None, 2, one, one, big) == lib.EINVAL
    assert _sums(f, one, 0, 0, 80, 8, 8, 10, bins, 2, None, one, big) == lib.EINVAL
    assert _sums(f, one, 0, 0, 80, 8, 8, 10, bins, 2, one, None, big) == lib.EINVAL
    assert _sums(f, one, 0, 0, 80, 8, 8, 10, bins, 0, one, one, big) == lib.EINVAL     # n_bins < 1
    assert b"n_bins=0" in lib.lib.espm_mu_last_error()
    assert _sums(f, one, 0, 0, 80, 8, 8, 10, [(1, 1), (0, 3)], 2, one, one, big) == lib.EINVAL   # by < 1
    assert b"bin 1 is (0, 3)" in lib.lib.espm_mu_last_error()
    assert _sums(f, one, 0, 0, 80, 8, 8, 10, [(2, 0)], 1, one, one, big) == lib.EINVAL
    assert _sums(f, one, 7, 0, 80, 8, 8, 10, bins, 2, one, one, big) == lib.EINVAL     # dtype code
    assert _sums(f, one, 0, 3, 80, 8, 8, 10, bins, 2, one, one, big) == lib.EINVAL     # layout
    assert _sums(f, one, 0, 0, 79, 8, 8, 10, bins, 2, one, one, big) == lib.EINVAL     # ld
    need = lib.lib.espm_binning_sums_scratch(8, 8, 10, 2)
    assert _sums(f, one, 0, 0, 80, 8, 8, 10, bins, 2, one, one, need - 1) == lib.EINVAL   # a short scratch
    msg = lib.lib.espm_mu_last_error()
    assert str(need).encode() in msg and str(need - 1).encode() in msg
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL)


def test_the_wide_builds_export_stubs(lib):
    for k in (12, 20):
        v = lib.variant(k)
        rc = v.lib.espm_rebin_pixels(None, 0, 0, 8, 8, 2, 4, 1, 1, None, lib.DIAG_X_F32, 8, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)
        assert v.lib.espm_binning_sums(None, 0, 0, 8, 8, 2, 4, None, 1, None, None, 0, None) == lib.EUNSUPPORTED
        assert v.lib.espm_binning_sums_scratch(8, 2, 4, 1) == 0


# ---- the Python module, before the device ------------------------------------------------------------------------------------------------
def test_module_checks_come_before_the_device(lib, monkeypatch):
    from espm_amd import binning
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.zeros((6, 20), np.uint8)
    with pytest.raises(ValueError, match="layout"):
        binning.rebin(X, (4, 5), (2, 2), layout="rows")
    with pytest.raises(ValueError, match="does not match"):
        binning.rebin(X, (4, 6), (2, 2))
    with pytest.raises(ValueError, match="does not match"):
        binning.rebin(X, (4, 5), (2, 2), layout="pm")
    with pytest.raises(ValueError, match="2-D"):
        binning.rebin(np.zeros(6), (2, 3), (1, 1))
    for bad in ((0, 2), (2, -1), (1.5, 2), 3, (1, 2, 3)):
        with pytest.raises(ValueError, match="pair of positive integers"):
            binning.rebin(X, (4, 5), bad)
        with pytest.raises(ValueError, match="pair of positive integers"):
            binning.binning_sums(X, (4, 5), [(1, 1), bad])
    with pytest.raises(ValueError, match="at least one"):
        binning.binning_sums(X, (4, 5), [])
    assert binning.binned_shape((13, 10), (3, 4)) == (5, 3) and binning.binned_shape((13, 10), (64, 128)) == (1, 1)
    assert binning.default_bins((16, 24)) == [(b, b) for b in range(1, 9)] and binning.default_bins((1, 7)) == [(1, 1)]
    # the risk from the four sums is the reference's
    T = br.sums(br.block_image(30, (8, 12), 4)[0], (8, 12), [(1, 1), (4, 4)])
    for mine, ref in zip(binning.risk_from_sums(*T, 30, 8, 12), br.risk(*T, 30, (8, 12))):
        assert np.array_equal(mine, ref)


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import binning
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X = np.zeros((6, 20), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        binning.rebin(X, (4, 5), (2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        binning.estimate_best_binning(X, (4, 5))


def _est(**kw):
    from espm_amd.estimators import SmoothNMF
    args = dict(n_components=3, shape_2d=(8, 12), max_iter=5, verbose=0)
    args.update(kw)
    return SmoothNMF(**args)


def test_fit_binned_refuses_before_any_upload(lib, monkeypatch):
    from espm_amd import binning
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.ones((10, 96), np.float32)
    with pytest.raises(ValueError, match=r"does not divide.*crop it to \(6, 10\)"):
        _est().fit_binned(X, (3, 5))
    with pytest.raises(ValueError, match="does not divide"):
        _est().fit_binned(X, (4, 5))
    with pytest.raises(ValueError, match="positive integers"):
        _est().fit_binned(X, (0, 4))
    with pytest.raises(NotImplementedError, match="fixed_H"):
        _est(fixed_H=-np.ones((3, 96))).fit_binned(X, (4, 4))
    with pytest.raises(NotImplementedError, match="linesearch"):
        _est(linesearch=True).fit_binned(X, (4, 4))
    with pytest.raises(NotImplementedError, match="projected_gradient"):
        _est(algo="projected_gradient").fit_binned(X, (4, 4))
    with pytest.raises(NotImplementedError, match="l2"):
        _est(l2=True, algo="l2_surrogate").fit_binned(X, (4, 4))
    with pytest.raises(NotImplementedError, match="fp64"):
        _est().set_precision("fp64").fit_binned(X, (4, 4))
    with pytest.raises(ValueError, match="shape_2d"):
        _est(shape_2d=None).fit_binned(X, (4, 4))


def test_adapter_routes_bin_to_fit_binned(lib):
    from espm_amd import hyperspy_adapter as ha

    class Est:
        hspy_comp, shape_2d = True, None

        def fit_binned(self, X, bin):
            self.seen = (X.shape, bin)
            self.components_ = np.zeros((2, X.shape[1]))
            return np.zeros((X.shape[0], 2))

        def fit_transform(self, X):
            raise AssertionError("bin was given")

    sig, est = ha.SpectrumImage(np.zeros((8, 12, 7), np.uint8)), Est()
    lr = ha.decompose(sig, est, bin=(4, 4))
    assert est.seen == ((96, 7), (4, 4)) and est.shape_2d == (8, 12)
    assert lr.loadings.shape == (96, 2) and lr.factors.shape == (7, 2) and sig.get_decomposition_loadings().shape == (2, 8, 12)


def test_adapter_fills_the_results_of_a_foreign_signal(lib):
    """A signal that is no SpectrumImage (hyperspy's own: its decomposition knows no bin): decompose(bin=) calls fit_binned on the
    unfolded data and fills learning_results as a custom algorithm's are filled."""
    import types

    from espm_amd import hyperspy_adapter as ha

    class Est:
        hspy_comp, shape_2d = True, None

        def fit_binned(self, X, bin):
            self.seen = (X.shape, bin, X[13, 2])
            self.components_ = np.arange(2 * X.shape[1], dtype=np.float64).reshape(2, X.shape[1])
            return np.ones((X.shape[0], 2))

    cube = np.arange(8 * 12 * 7).reshape(8, 12, 7)
    sig = types.SimpleNamespace(data=cube, shape_2d=(8, 12), learning_results=ha.LearningResults(),
                                decomposition=lambda **k: pytest.fail("hyperspy's decomposition knows no bin"))
    est = Est()
    lr = ha.decompose(sig, est, bin=(2, 3))
    assert est.seen == ((96, 7), (2, 3), cube[1, 1, 2]) and est.shape_2d == (8, 12)
    assert lr is sig.learning_results and lr.decomposition_algorithm is est and lr.output_dimension == 2
    assert lr.loadings.shape == (96, 2) and np.array_equal(lr.factors, est.components_.T)
    with pytest.raises(TypeError, match="unsupported decomposition arguments"):
        ha.decompose(sig, Est(), bin=(2, 3), output_dimension=2)
