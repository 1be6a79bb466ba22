"""The pinned rule of the pixel ML and the interval root finder without a device: the conditions the GPU tests
(test_gpu_abundance_intervals.py) rest on, held by the numpy restatement alone (tests/pixel_ml_pinned_reference.py); the binding of
espm_pixel_ml_pinned and its refusals before any launch; and the argument errors of ``presence.ml_unmix_pinned``,
``presence.intervals`` and ``est.abundance_intervals`` before any upload."""
import ctypes as C

import numpy as np
import pytest

import pixel_ml_pinned_reference as pn

TOL = 1e-3
LR_TOL = 1e-2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


_pinned, LABELS = pn.pinned, pn.LABELS


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pn.CASES)
def test_every_pinned_fit_converges_within_half_the_cap(name):
    """On every image the GPU tests use, every pinned fit - those of the root finder and those at the four tested values - converges
    within 64 passes, half of max_pass = 128 (measured: at most 48, in the root finder on ``collinear``)."""
    most = pn.solved(name)["max_fit_pass"]
    for label in LABELS:
        fit = _pinned(name, label)
        assert fit["converged"].all() and fit["nonfinite"] == 0 and (fit["gap"] <= TOL).all()
        assert np.isfinite(fit["H"]).all() and (fit["H"] >= 0).all()
        most = max(most, int(fit["n_pass"].max()))
    print(f"{name}: at most {most} passes in a pinned fit")
    assert pn.MAX_PASS == 128 and most <= pn.MAX_PASS // 2


@pytest.mark.parametrize("name", pn.CASES)
def test_every_endpoint_finishes_within_half_the_cap(name):
    """Every end of every interval is found within 32 evaluations, half of max_eval = 64 (measured: at most 8 evaluations and 90
    passes in all per end)."""
    out = pn.solved(name)
    k = out["H_ml"].shape[0]
    print(f"{name}: evaluations per end <= {out['n_eval'].max()}, lower {out['n_eval'][:, 0].max()}, upper {out['n_eval'][:, 1].max()}; "
          f"passes per end <= {out['n_pass'].max()}; lower == 0 in {np.mean(out['lower'] == 0):.3f} of the entries")
    assert pn.MAX_EVAL == 64
    assert out["converged"].all() and out["n_eval"].max() <= pn.MAX_EVAL // 2
    assert out["lower"].shape == out["upper"].shape == (k, out["deviance_ml"].size)
    assert np.isfinite(out["lower"]).all() and np.isfinite(out["upper"]).all()
    assert (out["lower"] <= out["H_ml"]).all() and (out["H_ml"] <= out["upper"]).all() and (out["lower"] >= 0).all()


@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("name", pn.CASES)
def test_certificate_holds_against_the_long_run(name, label):
    """dev - dev_opt - gap <= 1e-9 max(1, dev) against a pinned run at tol = 1e-10, and the reported values are those of the
    returned h."""
    X, D = pn.case(name)
    fit, opt = _pinned(name, label), _pinned(name, label, 1e-10)
    assert opt["converged"].all()
    excess = fit["deviance"] - opt["deviance"] - fit["gap"]
    print(f"{name} {label}: dev - dev_opt - gap <= {excess.max():.3g}; dev - dev_opt in [{(fit['deviance'] - opt['deviance']).min():.3g}, "
          f"{(fit['deviance'] - opt['deviance']).max():.3g}]")
    assert (excess <= 1e-9 * np.maximum(1.0, fit["deviance"])).all()
    ev = pn.evaluate(X, D, fit["H"], D.shape[1] - 1)
    np.testing.assert_allclose(ev["deviance"], fit["deviance"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ev["slope"], fit["slope"], rtol=1e-9, atol=1e-9)
    assert np.array_equal(fit["H"][-1], pn.pins(name)[label])


@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("name", pn.CASES)
def test_accepted_deviances_never_increase(name, label):
    assert _pinned(name, label)["monotone"].all()


def test_the_far_value_drives_every_free_abundance_to_the_boundary():
    X, D = pn.case("planted")
    fit = _pinned("planted", "far")
    live = fit["N"] > 0
    s = D.sum(axis=0)
    assert ((s[:-1, None] * fit["H"][:-1])[:, live].sum(axis=0) <= 1e-2 * fit["N"][live]).all()


def test_a_pixel_without_counts_and_the_empty_free_set():
    X, D = pn.case("planted")
    out, q = pn.solved("planted"), pn.threshold(0.95)
    s = D.sum(axis=0)
    assert not X[:, 5].any() and (out["lower"][:, 5] == 0).all()
    assert (np.abs(out["upper"][:, 5] - q / (2 * s)) <= LR_TOL / (2 * s)).all()
    one = pn.solved("img96_k1")
    X1, D1 = pn.case("img96_k1")
    N, s1 = X1.sum(axis=0).astype(np.float64), D1.sum()
    assert not one["n_pass"].any()   # nothing is fitted: every evaluation is done in its first pass
    for end in (one["lower"][0], one["upper"][0]):
        assert (np.abs(2.0 * (end * s1 - N - N * np.log(end * s1 / N)) - q) <= LR_TOL).all()
    assert abs(pn.threshold(0.68) - 0.98895) <= 1e-4


@pytest.mark.parametrize("name", pn.CASES)
def test_two_summation_orders_agree_on_the_counts(name):
    """The margin the GPU tests leave for accept / reject ties and for an end that meets lr_tol an evaluation apart: under a second
    order of every sum the pass counts and ``n_eval`` differ in at most 1 % of the pixels."""
    X, D = pn.case(name)
    a, b = pn.solved(name), pn.flipped_intervals(X, D)
    de, dp = (a["n_eval"] != b["n_eval"]).any(axis=(0, 1)), (a["n_pass"] != b["n_pass"]).any(axis=(0, 1))
    print(f"{name}: {de.sum()} of {de.size} pixels differ in n_eval, {dp.sum()} in n_pass")
    assert de.mean() <= 0.01 and dp.mean() <= 0.01
    fa = _pinned(name, "twice")
    fb = pn.flipped_pinned(X, D, D.shape[1] - 1, pn.pins(name)["twice"], a["H_ml"])
    assert (fa["n_pass"] != fb["n_pass"]).mean() <= 0.01


def test_a_value_that_is_negative_or_not_finite_stops_the_pixel():
    X, D = pn.case("planted")
    t = np.ones(X.shape[1])
    t[3], t[7], t[11] = -1.0, np.nan, np.inf
    fit = pn.ml_unmix_pinned(X, D, 0, t)
    bad = np.zeros(t.size, dtype=bool)
    bad[[3, 7, 11]] = True
    assert fit["nonfinite"] == 3 and not fit["converged"][bad].any() and fit["converged"][~bad].all() and not fit["n_pass"][bad].any()


# ---- the binding and the refusals before any launch ---------------------------------------------------------------------------------------
def _s(*v):
    return (C.c_double * 8)(*v)


def test_entry_point_is_bound_and_the_wide_builds_refuse(lib):
    res, args = lib.SYMBOLS["espm_pixel_ml_pinned"]
    nw = lib.SYMBOLS["espm_pixel_ml_newton"][1]
    assert res is C.c_int and len(args) == 25
    # espm_pixel_ml_newton's, with pin and t after the mask and slope after gap
    assert args[:10] == nw[:10] and args[10:12] == [C.c_int, C.c_void_p] and args[12:18] == nw[10:16] and args[18] == C.c_void_p
    assert args[19:] == nw[16:]
    one = C.c_void_p(8)
    for k in (12, 20):   # the 9..16 and the 17..32 component builds export a stub
        v = lib.variant(k)
        rc = v.lib.espm_pixel_ml_pinned(one, 0, 0, 8, 8, 8, one, _s(1, 1, 1), 3, 3, 2, one, 1e-14, 1e-3, 1, one, one, one, one, one, one, one, one, 1 << 20, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)


def test_host_side_argument_errors_need_no_device(lib):
    """Status codes of the narrow build's entry point for arguments it refuses before any launch."""
    f = lib.lib.espm_pixel_ml_pinned
    one = C.c_void_p(8)   # (never dereferenced: every call below is refused on the host)
    s = _s(1, 1, 1)
    need = (3 + lib.PMLN_STATE_EXTRA) * 8 * 8   # k = 3, p = 8

    def call(x=one, layout=0, ld=8, n=8, p=8, s=s, k=3, mask=3, pin=2, t=one, log_shift=1e-14, tol=1e-3, n_pass=1, h=one, slope=one, state=one,
             nbytes=need):
        return f(x, 0, layout, ld, n, p, one, s, k, mask, pin, t, log_shift, tol, n_pass, h, one, one, slope, one, one, one, state, nbytes, None)

    assert call(k=9, mask=1, pin=1) == lib.EUNSUPPORTED
    assert call(k=0, mask=0, pin=0) == lib.EUNSUPPORTED
    assert call(x=None) == lib.EINVAL
    assert call(h=None) == lib.EINVAL
    assert call(s=None) == lib.EINVAL
    assert call(t=None) == lib.EINVAL
    assert b"t (nil)" in lib.lib.espm_mu_last_error() or b"t 0" in lib.lib.espm_mu_last_error()
    assert call(slope=None) == lib.EINVAL
    assert call(layout=2) == lib.EINVAL
    assert call(ld=7) == lib.EINVAL
    assert b"ld=7" in lib.lib.espm_mu_last_error()
    assert call(n=0) == lib.EINVAL
    assert call(log_shift=0.0) == lib.EINVAL
    assert call(tol=0.0) == lib.EINVAL and call(tol=-1.0) == lib.EINVAL
    assert call(n_pass=0) == lib.EINVAL
    assert call(mask=8) == lib.EINVAL                   # a bit beyond the k components
    assert call(pin=3) == lib.EINVAL and call(pin=-1) == lib.EINVAL   # no component
    assert b"pin" in lib.lib.espm_mu_last_error()
    assert call(mask=7) == lib.EINVAL and call(mask=4) == lib.EINVAL   # the pinned component inside the mask
    assert b"in the mask" in lib.lib.espm_mu_last_error()
    assert call(s=_s(1, 1, 0)) == lib.EINVAL            # the pinned spectrum is all zero
    assert b"component 2 is pinned" in lib.lib.espm_mu_last_error()
    assert call(s=_s(1, 0, 1)) == lib.EINVAL            # a component of the set whose spectrum is all zero
    assert b"component 1" in lib.lib.espm_mu_last_error()
    assert call(s=_s(1, float("nan"), 1)) == lib.EINVAL
    assert call(state=None) == lib.EINVAL
    assert call(nbytes=need - 1) == lib.EINVAL
    assert b"state" in lib.lib.espm_mu_last_error()
    with pytest.raises(ValueError):
        lib.check(call(nbytes=0))


def test_argument_errors_come_before_the_upload(lib, monkeypatch):
    from espm_amd import _image, presence
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X, D = np.zeros((6, 10), np.float32), np.ones((6, 2))
    for level in (0.0, 1.0, -0.5, 1.5, True):
        with pytest.raises(ValueError, match="level"):
            presence.intervals(X, D, level=level)
    with pytest.raises(ValueError, match="lr_tol"):
        presence.intervals(X, D, lr_tol=0.0)
    with pytest.raises(ValueError, match="max_eval"):
        presence.intervals(X, D, max_eval=0)
    with pytest.raises(ValueError, match="components"):
        presence.intervals(X, D, components=[2])
    with pytest.raises(ValueError, match="channels"):
        presence.intervals(X, np.ones((5, 2)))
    with pytest.raises(ValueError, match="tol"):
        presence.intervals(X, D, tol=0.0)
    with pytest.raises(NotImplementedError, match="9 components"):
        presence.intervals(X, np.ones((6, 9)))
    Dz = np.ones((6, 2))
    Dz[:, 1] = 0.0
    with pytest.raises(ValueError, match="component 1"):
        presence.intervals(X, Dz, components=[0])     # the fits are over all components
    with pytest.raises(ValueError, match="H0"):
        presence.intervals(X, D, H0=np.ones((2, 9)))
    for pin in (2, -1, 0.5, True):
        with pytest.raises(ValueError, match="pin"):
            presence.ml_unmix_pinned(X, D, pin, 1.0)
    with pytest.raises(ValueError, match="pinned component 0 is in"):
        presence.ml_unmix_pinned(X, D, 0, 1.0, components=[0, 1])
    with pytest.raises(ValueError, match="pinned component 1 is all zero"):
        presence.ml_unmix_pinned(X, Dz, 1, 1.0)
    for t in (-1.0, np.nan, np.inf, np.ones(9), np.ones((10, 1))):
        with pytest.raises(ValueError, match="t must"):
            presence.ml_unmix_pinned(X, D, 0, t)
    with pytest.raises(ValueError, match="channels"):
        presence.ml_unmix_pinned(X, np.ones((5, 2)), 0, 1.0)
    with pytest.raises(NotImplementedError, match="9 components"):
        presence.ml_unmix_pinned(X, np.ones((6, 9)), 0, 1.0)


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import presence
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X, D = pn.case("planted")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        presence.ml_unmix_pinned(X, D, 0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        presence.intervals(X, D)


def test_estimator_refuses_before_the_image(lib):
    import types

    from espm_amd.estimators import SmoothNMF
    with pytest.raises(Exception, match="not fitted"):
        SmoothNMF(n_components=2).abundance_intervals()
    est = SmoothNMF(n_components=2)
    est.W_, est.H_ = np.ones((6, 2)), np.ones((2, 10))
    est._image_argument = types.MethodType(lambda self, *a: pytest.fail("the image was reached"), est)
    for level in (0.0, 1.0, 2.0):
        with pytest.raises(ValueError, match="level"):
            est.abundance_intervals(level, np.zeros((6, 10)))
    with pytest.raises(ValueError, match="components"):
        est.abundance_intervals(X=np.zeros((6, 10)), components=[5])
    big = SmoothNMF(n_components=9)
    big.W_, big.H_ = np.ones((6, 9)), np.ones((9, 10))
    big._image_argument = est._image_argument
    with pytest.raises(NotImplementedError, match="9 components"):
        big.abundance_intervals(X=np.zeros((6, 10)))
    assert not hasattr(est, "H_lower_")


def test_estimator_refuses_the_fits_own_image_after_fit_binned(lib):
    """``X=None`` after ``fit_binned`` is refused as ``presence_maps`` refuses it: by ``_image_argument``, before anything is uploaded."""
    from espm_amd.estimators import SmoothNMF
    est = SmoothNMF(n_components=2)
    est.W_, est.H_, est.G_ = np.ones((6, 2)), np.ones((2, 10)), np.eye(6)
    est.bin_ = 2
    est._fitted_binned = lambda: True
    with pytest.raises(ValueError):
        est.abundance_intervals()


def test_adapter_needs_the_intervals(lib):
    from espm_amd import hyperspy_adapter as ha
    from espm_amd.estimators import SmoothNMF
    with pytest.raises(AttributeError, match="abundance_intervals"):
        ha.abundance_interval_maps(SmoothNMF(n_components=2))
