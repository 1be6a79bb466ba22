"""pixel_diagnostics without a device: the binding, the argument checks that come before any upload, the refusal to run without a
GPU, and the self-consistency of the numpy reference the GPU tests compare against (tests/diag_reference.py) and of its bounds."""
import ctypes as C

import numpy as np
import pytest

import diag_reference as dr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


def test_entry_point_is_bound_and_the_wide_builds_refuse(lib):
    res, args = lib.SYMBOLS["espm_pixel_diagnostics"]
    assert res is C.c_int and len(args) == 15
    assert (lib.DIAG_X_U8, lib.DIAG_X_U16, lib.DIAG_X_F32, lib.DIAG_X_F64) == (0, 1, 2, 3)
    assert lib.DIAG_MAX_K == 8 and lib.DIAG_BLOCK == 256
    for k in (12, 20):   # the 9..16 and the 17..32 component builds export a stub
        v = lib.variant(k)
        rc = v.lib.espm_pixel_diagnostics(None, 0, 0, 8, 8, 8, None, None, 3, 1e-14, 0, None, None, None, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)


def test_host_side_argument_errors_need_no_device(lib):
    """Status codes of the narrow build's entry point for arguments it refuses before any launch."""
    f = lib.lib.espm_pixel_diagnostics
    one = C.c_void_p(8)   # (never dereferenced: every call below is refused on the host)
    assert f(one, 0, 0, 8, 8, 8, one, one, 9, 1e-14, 0, one, one, None, None) == lib.EUNSUPPORTED
    assert f(one, 0, 0, 8, 8, 8, one, one, 0, 1e-14, 0, one, one, None, None) == lib.EUNSUPPORTED
    assert f(None, 0, 0, 8, 8, 8, one, one, 3, 1e-14, 0, one, one, None, None) == lib.EINVAL
    assert f(one, 0, 2, 8, 8, 8, one, one, 3, 1e-14, 0, one, one, None, None) == lib.EINVAL          # layout
    assert f(one, 0, 0, 7, 8, 8, one, one, 3, 1e-14, 0, one, one, None, None) == lib.EINVAL          # ld below the row length
    assert b"ld=7" in lib.lib.espm_mu_last_error()
    assert f(one, 0, 1, 7, 8, 16, one, one, 3, 1e-14, 0, one, one, None, None) == lib.EINVAL         # pixel-major: rows of n
    assert f(one, 0, 0, 8, 0, 8, one, one, 3, 1e-14, 0, one, one, None, None) == lib.EINVAL


def test_shape_checks_come_before_the_device(lib, monkeypatch):
    from espm_amd import measures
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X, D, H = np.zeros((6, 10), np.float32), np.ones((6, 2)), np.ones((2, 10))
    with pytest.raises(ValueError, match="layout"):
        measures.pixel_diagnostics(X, D, H, layout="rows")
    with pytest.raises(ValueError, match="channels"):
        measures.pixel_diagnostics(X, np.ones((5, 2)), H)
    with pytest.raises(ValueError, match="pixels"):
        measures.pixel_diagnostics(X, D, np.ones((2, 9)))
    with pytest.raises(ValueError, match="channels"):
        measures.pixel_diagnostics(X, D, H, layout="pm")            # (10, 6) read as (pixels, channels): 6 pixels, 10 channels
    with pytest.raises(ValueError):
        measures.pixel_diagnostics(X, np.ones((6, 3)), H)
    with pytest.raises(ValueError, match="2-D"):
        measures.pixel_diagnostics(np.zeros(6), D, H)
    with pytest.raises(ValueError, match="log_shift"):
        measures.pixel_diagnostics(X, D, H, log_shift=0.0)
    with pytest.raises(NotImplementedError, match="9 components"):
        measures.pixel_diagnostics(X, np.ones((6, 9)), np.ones((9, 10)))


def test_host_dtypes_go_up_exactly(lib):
    from espm_amd._image_args import measured_dtype
    same = (np.uint8, np.uint16, np.float32, np.float64)
    assert all(measured_dtype(d) == np.dtype(d) for d in same)
    assert measured_dtype(np.bool_) == np.uint8
    assert all(measured_dtype(d) == np.float32 for d in (np.int8, np.int16, np.float16))
    assert all(measured_dtype(d) == np.float64 for d in (np.int32, np.uint32, np.int64, np.uint64))
    with pytest.raises(TypeError):
        measured_dtype(np.complex64)


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import measures
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X, D, H, _ = dr.image(70, 64, 2, "float64", False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        measures.pixel_diagnostics(X, D, H)


def test_estimator_method_refuses_an_unfitted_estimator(lib):
    from sklearn.exceptions import NotFittedError

    from espm_amd.estimators import SmoothNMF
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=3).pixel_diagnostics(np.zeros((6, 10)))


def test_navigation_shape_helper(lib):
    import types

    from espm_amd import hyperspy_adapter as ha
    est = types.SimpleNamespace(shape_2d=(4, 5))
    with pytest.raises(AttributeError):
        ha.diagnostic_maps(est)
    est.deviance_, est.H_std_ = np.arange(20.0), np.arange(60.0).reshape(3, 20)
    dev, std = ha.diagnostic_maps(est)
    assert dev.shape == (4, 5) and std.shape == (3, 4, 5)
    assert dev[2, 3] == est.deviance_[2 * 5 + 3] and std[1, 2, 3] == est.H_std_[1, 2 * 5 + 3]
    assert ha.diagnostic_maps(est, (5, 4))[1].shape == (3, 5, 4)


# ---- the reference itself -------------------------------------------------------------------------------------------------------
CASES = [(70, 667, 3, "float32"), (70, 667, 1, "float32"), (70, 667, 8, "uint8"), (308, 300, 5, "uint16"), (70, 64, 2, "float64")]


@pytest.mark.parametrize("n,p,k,dtype", CASES)
def test_reference_images_meet_their_conditions(n, p, k, dtype):
    for simplex in (False, True):
        X, D, H, facts = dr.image(n, p, k, dtype, simplex)
        assert X.shape == (n, p) and X.dtype == np.dtype(dtype) and (H > 0).all()
        assert not X[:, facts["empty_pixel"]].any() and not X[facts["zero_channel"]].any()
        assert ((D @ H) < dr.LOG_SHIFT).any() and X[facts["floor_channel"], facts["floor_pixel"]] > 0
        if simplex:
            np.testing.assert_allclose(H.sum(axis=0), 1.0, rtol=1e-14)
        if dtype == "uint16":
            assert X.max() > 255
        if dtype == "float64":
            assert (X != np.round(X)).any()
        ref = dr.reference(X, D, H, simplex=simplex)
        assert ref["cond"].max() < 1e8, "the parity images must stay away from the NaN rule"
        assert np.isfinite(ref["deviance"]).all() and (ref["deviance"] >= 0).all() and np.isfinite(ref["H_std"]).all()


def test_constrained_covariance_has_no_component_along_ones():
    """1^T C 1 = 0 (and C 1 = 0) to rounding: the simplex bound allows no change of sum_i h_i."""
    for n, p, k, dtype in CASES:
        if k == 1:
            continue
        X, D, H, _ = dr.image(n, p, k, dtype, True)
        ref = dr.reference(X, D, H, simplex=True)
        C_, scale = ref["C"], np.abs(np.linalg.inv(ref["F"])).sum(axis=(1, 2))
        assert (np.abs(C_.sum(axis=(1, 2))) <= 64 * k * k * dr.EPS * ref["cond"] * scale).all()
        assert (np.abs(C_.sum(axis=2)).max(axis=1) <= 64 * k * k * dr.EPS * ref["cond"] * scale).all()
        free = dr.reference(X, D, H, simplex=False)
        assert (ref["H_std"] <= free["H_std"] * (1 + 1e-12)).all(), "a constraint cannot widen an error bar"
    X, D, H, _ = dr.image(70, 667, 1, "float32", True)
    assert not dr.reference(X, D, H, simplex=True)["H_std"].any()


def test_reference_deviance_is_the_kl_divergence():
    """2 KL(x || y) by another route (scipy's rel_entr), and the singular rule's threshold on a rank-deficient D."""
    from scipy.special import rel_entr
    X, D, H, _ = dr.image(70, 64, 2, "float64", False)
    ref = dr.reference(X, D, H)
    Y = np.maximum(D @ H, dr.LOG_SHIFT)
    other = 2.0 * (rel_entr(X.astype(np.float64), Y) - X + Y).sum(axis=0)
    assert (np.abs(other - ref["deviance"]) <= 8 * 70 * dr.EPS * ref["abs_terms"]).all()
    D2 = np.repeat(dr.spectra(70, 1, 500.0), 2, axis=1)
    assert dr.reference(X, D2, H)["cond"].min() > 1e15


@pytest.mark.parametrize("n,p,k,dtype", CASES)
def test_deviance_bound_holds_for_the_kernels_order_of_evaluation(n, p, k, dtype):
    """8 n eps sum_c |t_c| has room for an fp64 evaluation: the kernel's own (t = y - x + x ln(x (1 / y)), added channel by channel),
    emulated here in numpy, against the reference; and both against an extended-precision evaluation where numpy has one."""
    for simplex in (False, True):
        X, D, H, _ = dr.image(n, p, k, dtype, simplex)
        ref = dr.reference(X, D, H, simplex=simplex)
        x = X.astype(np.float64)
        Y = np.maximum(D @ H, dr.LOG_SHIFT)
        t = Y - x
        pos = x > 0
        t[pos] += x[pos] * np.log(x[pos] * (1.0 / Y[pos]))
        emulated = 2.0 * np.cumsum(t, axis=0)[-1]   # (cumsum adds in order, as the kernel's loop does)
        bound = 8 * n * dr.EPS * ref["abs_terms"]
        print(f"n={n} k={k} {dtype}: kernel order vs reference {np.max(np.abs(emulated - ref['deviance']) / bound):.3g} of the bound")
        assert (np.abs(emulated - ref["deviance"]) <= bound).all()
        if np.finfo(np.longdouble).eps < 2.0 ** -60:
            xl, Dl, Hl = (a.astype(np.longdouble) for a in (X, D, H))
            Yl = np.maximum(Dl @ Hl, np.longdouble(dr.LOG_SHIFT))
            tl = Yl - xl
            tl[pos] += xl[pos] * np.log(xl[pos] / Yl[pos])
            exact = 2 * tl.sum(axis=0)
            for name, got in (("reference", ref["deviance"]), ("kernel order", emulated)):
                r = np.max(np.abs(got - exact).astype(np.float64) / bound)
                print(f"    {name} vs extended precision {r:.3g} of the bound")
                assert r <= 1
