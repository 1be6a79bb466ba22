"""Pixel ML and the presence maps without a device: the binding, the refusals that come before any launch or upload, and the
self-consistency of the numpy reference (tests/pixel_ml_reference.py) on the images the GPU tests use - its certificate, the nesting
of its models, and the condition that keeps the GPU tests honest: the reference alone converges everywhere well inside their cap."""
import ctypes as C

import numpy as np
import pytest

import pixel_ml_reference as pr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


def _s(*v):
    return (C.c_double * 8)(*v)


def test_entry_point_is_bound_and_the_wide_builds_refuse(lib):
    res, args = lib.SYMBOLS["espm_pixel_ml"]
    assert res is C.c_int and len(args) == 20
    assert lib.PML_MAX_K == 8 and (lib.PML_NOT_DONE, lib.PML_UNMODELLED, lib.PML_NONFINITE, lib.PML_COUNTERS) == (0, 1, 2, 3)
    one = C.c_void_p(8)
    for k in (12, 20):   # the 9..16 and the 17..32 component builds export a stub
        v = lib.variant(k)
        rc = v.lib.espm_pixel_ml(one, 0, 0, 8, 8, 8, one, _s(1, 1, 1), 3, 7, 1e-14, 1e-3, 1, one, one, one, one, one, one, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)


def test_host_side_argument_errors_need_no_device(lib):
    """Status codes of the narrow build's entry point for arguments it refuses before any launch."""
    f = lib.lib.espm_pixel_ml
    one = C.c_void_p(8)   # (never dereferenced: every call below is refused on the host)
    s = _s(1, 1, 1)

    def call(x=one, layout=0, ld=8, n=8, p=8, s=s, k=3, mask=7, log_shift=1e-14, tol=1e-3, n_pass=1, h=one):
        return f(x, 0, layout, ld, n, p, one, s, k, mask, log_shift, tol, n_pass, h, one, one, one, one, one, None)

    assert call(k=9, mask=1) == lib.EUNSUPPORTED
    assert call(k=0, mask=1) == lib.EUNSUPPORTED
    assert call(x=None) == lib.EINVAL
    assert call(h=None) == lib.EINVAL
    assert call(s=None) == lib.EINVAL
    assert call(layout=2) == lib.EINVAL
    assert call(ld=7) == lib.EINVAL                     # ld below the row length
    assert b"ld=7" in lib.lib.espm_mu_last_error()
    assert call(layout=1, ld=7, p=16) == lib.EINVAL     # pixel-major: rows of n
    assert call(n=0) == lib.EINVAL
    assert call(log_shift=0.0) == lib.EINVAL
    assert call(tol=0.0) == lib.EINVAL and call(tol=-1.0) == lib.EINVAL
    assert b"tol" in lib.lib.espm_mu_last_error()
    assert call(n_pass=0) == lib.EINVAL
    assert call(mask=0) == lib.EINVAL                   # the empty set
    assert call(mask=8) == lib.EINVAL                   # a bit beyond the k components
    assert call(s=_s(1, 0, 1)) == lib.EINVAL            # a component of the set whose spectrum is all zero
    assert b"component 1" in lib.lib.espm_mu_last_error()
    assert call(s=_s(1, float("nan"), 1)) == lib.EINVAL
    with pytest.raises(ValueError):
        lib.check(call(s=_s(1, 0, 1)))


def test_shape_checks_come_before_the_device(lib, monkeypatch):
    from espm_amd import presence
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X, D = np.zeros((6, 10), np.float32), np.ones((6, 2))
    for f in (presence.ml_unmix, presence.presence):
        with pytest.raises(ValueError, match="layout"):
            f(X, D, layout="rows")
        with pytest.raises(ValueError, match="channels"):
            f(X, np.ones((5, 2)))
        with pytest.raises(ValueError, match="channels"):
            f(X, D, layout="pm")                # (10, 6) read as (pixels, channels)
        with pytest.raises(ValueError, match="2-D"):
            f(np.zeros(6), D)
        with pytest.raises(ValueError, match="log_shift"):
            f(X, D, log_shift=0.0)
        with pytest.raises(ValueError, match="tol"):
            f(X, D, tol=0.0)
        with pytest.raises(ValueError, match="max_pass"):
            f(X, D, max_pass=0)
        with pytest.raises(ValueError, match="chunk"):
            f(X, D, chunk=1.5)
        with pytest.raises(ValueError, match="H0"):
            f(X, D, H0=np.ones((2, 9)))
        with pytest.raises(ValueError, match="not finite"):
            f(X, D, H0=np.full((2, 10), np.nan))
        with pytest.raises(ValueError, match="negative"):
            f(X, -D)
        with pytest.raises(ValueError, match="finite"):
            f(X, np.full((6, 2), np.inf))
        with pytest.raises(ValueError, match="finite"):
            f(np.full((6, 10), np.nan), D)
        with pytest.raises(NotImplementedError, match="9 components"):
            f(X, np.ones((6, 9)))
    Dz = np.ones((6, 3))
    Dz[:, 1] = 0.0
    with pytest.raises(ValueError, match="component 1"):
        presence.ml_unmix(X, Dz)
    with pytest.raises(ValueError, match="component 1"):
        presence.presence(X, Dz)
    for bad in ([], [3], [0, 0], [-1], [0.5]):
        with pytest.raises(ValueError, match="components"):
            presence.ml_unmix(X, Dz, components=bad)


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import presence
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X, D = pr.case("planted")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        presence.ml_unmix(X, D)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        presence.presence(X, D)


def test_estimator_method_refuses_an_unfitted_estimator(lib):
    from sklearn.exceptions import NotFittedError

    from espm_amd.estimators import SmoothNMF
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=3).presence_maps(np.zeros((6, 10)))


def test_navigation_shape_helper(lib):
    import types

    from espm_amd import hyperspy_adapter as ha
    est = types.SimpleNamespace(shape_2d=(4, 5))
    with pytest.raises(AttributeError):
        ha.presence_maps(est)
    est.H_ml_, est.presence_lr_, est.presence_pvalue_ = (np.arange(60.0).reshape(3, 20) + i for i in range(3))
    h, lr, pv = ha.presence_maps(est)
    assert h.shape == lr.shape == pv.shape == (3, 4, 5)
    assert lr[1, 2, 3] == est.presence_lr_[1, 2 * 5 + 3] and pv[2, 0, 4] == est.presence_pvalue_[2, 4]
    assert ha.presence_maps(est, (5, 4))[0].shape == (3, 5, 4)


def test_pvalue_is_the_boundary_mixture():
    from scipy.stats import chi2

    from espm_amd import presence
    lr = np.array([0.0, 1e-12, 0.5, 2.705543454095404, 10.0, 40.0])
    np.testing.assert_allclose(presence.pvalue(lr)[1:], 0.5 * chi2.sf(lr[1:], 1), rtol=1e-12)
    assert presence.pvalue(lr)[0] == 1.0 and abs(presence.pvalue(lr)[3] - 0.05) < 1e-12
    assert np.array_equal(presence.pvalue(lr), pr.pvalue(lr))


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.CASES)
def test_reference_converges_within_half_the_cap_the_gpu_tests_pass(name):
    """The condition that keeps the GPU tests honest: on every image they use, at the tolerances they use, the numpy reference alone
    converges on every pixel within half of their max_pass - a GPU pixel that fails to is a finding, not a slow pixel."""
    ref = pr.solved(name)
    print(f"{name}: at most {ref['n_pass'].max()} passes at tol = 1e-3")
    assert ref["converged"].all() and ref["n_pass"].max() <= pr.MAX_PASS // 2
    assert np.isfinite(ref["H"]).all() and (ref["H"] >= 0).all()


def test_reference_nested_models_converge_within_half_the_cap():
    """The same for the k + 1 nested fits of ``presence`` on the planted image (the one the GPU tests run it on), at both tolerances."""
    X, D = pr.case("planted")
    for tol in (1e-3, 1e-6):
        out = pr.presence(X, D, None, tol, pr.MAX_PASS)
        print(f"tol = {tol:g}: at most {out['n_pass'].max(axis=1)} passes")
        assert out["converged"].all() and out["n_pass"].max() <= pr.MAX_PASS // 2
        # lr >= 0, and the nesting before the clip: a model without j cannot fit better than the model with it, up to the gap of the full fit
        assert (out["lr"] >= 0).all()
        assert (out["deviance_without"] >= out["deviance_ml"][None, :] - tol).all()
        assert (out["pvalue"][out["lr"] == 0] == 1.0).all() and (out["pvalue"] <= 1.0).all() and (out["pvalue"] > 0).all()


@pytest.mark.parametrize("name", pr.CASES)
def test_certified_gap_bounds_the_true_excess(name):
    """Over the long run (tol = 1e-10) the deviance of every pass is above the run's final deviance by at most that pass's gap: the
    certificate, checked against the trajectory's own end (which is itself within its last gap of the minimum)."""
    opt = pr.optimum(name)
    slack = 1e-9 * np.maximum(1.0, opt["deviance"])   # fp64 rounding of two deviances of <= 300 terms
    assert (opt["certificate_excess"] <= slack).all(), opt["certificate_excess"].max()
    ref = pr.solved(name)
    assert (ref["deviance"] >= opt["deviance"] - slack).all()                 # monotone: the longer run is lower
    assert (ref["deviance"] <= opt["deviance"] + opt["gap"].clip(0) + ref["gap"] + slack).all()
    assert (ref["gap"] <= 1e-3).all()


@pytest.mark.parametrize("name", pr.CASES)
def test_two_summation_orders_agree_on_the_pass_counts(name):
    """The cap the GPU tests put on pass counts that differ (1 % of the pixels, by one pass) holds between two orders of summation on
    the host: the images do not sit on the threshold."""
    X, D = pr.case(name)
    a, b = pr.solved(name), pr.flipped(X, D, pr.start_from(X, D))
    differ = a["n_pass"] != b["n_pass"]
    print(f"{name}: {differ.sum()} of {differ.size} pixels stop a pass apart")
    assert differ.mean() <= 0.01 and (np.abs(a["n_pass"] - b["n_pass"]) <= 1).all()


def test_evaluate_reproduces_the_run_and_the_planted_image_its_conditions():
    X, D, H, gone = pr.planted()
    assert X.shape == (48, 300) and X.dtype == np.uint8 and 25 < X.sum(axis=0).mean() < 35
    assert 0.3 < gone.mean() < 0.5 and not gone.all(axis=0).any() and (H[gone] == 0).all()
    assert not X[:, 5].any()
    ref = pr.solved("planted")
    assert ref["n_pass"][5] == 0 and ref["converged"][5] and not ref["H"][:, 5].any() and ref["deviance"][5] == 0 and ref["gap"][5] == 0
    ev = pr.evaluate(X, D, ref["H"])
    live = ev["N"] > 0
    np.testing.assert_allclose(ev["deviance"][live], ref["deviance"][live], rtol=1e-12)
    assert (np.abs(ev["gap"] - ref["gap"])[live] <= 1e-10 * ev["N"][live]).all()
    np.testing.assert_allclose((D.sum(axis=0) @ ref["H"])[live], ev["N"][live], rtol=1e-14)
    # masked-out rows stay 0, and a start that is not positive is replaced by the rule
    sub = pr.ml_unmix(X, D, np.zeros((4, 300)), [0, 2])
    assert not sub["H"][[1, 3]].any() and sub["converged"].all() and (sub["H"][[0, 2]][:, live] > 0).any()
    assert pr.empty_model_deviance(X)[5] == 0 and (pr.empty_model_deviance(X)[live] > ref["deviance"][live]).all()
