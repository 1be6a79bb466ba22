"""The Newton rule of the pixel ML without a device: the conditions the GPU tests (test_gpu_pixel_ml_newton.py) rest on, held by the
numpy restatement of the rule alone (tests/pixel_ml_newton_reference.py); the binding of espm_pixel_ml_newton and its refusals before
any launch; and the refusal of a method that does not exist before any upload."""
import ctypes as C

import numpy as np
import pytest

import pixel_ml_newton_reference as nr
import pixel_ml_reference as pr

TOL = 1e-3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nr.CASES)
def test_reference_converges_within_half_the_cap_the_gpu_tests_pass(name):
    """On every image the GPU tests use, the reference alone converges every pixel within 64 passes, half of their max_pass = 128
    (measured: at most 29) - a GPU pixel that fails to is a finding, not a slow pixel."""
    ref = nr.solved(name)
    n = ref["n_pass"]
    print(f"{name}: passes median {np.median(n):.0f}, 99 % {np.percentile(n, 99):.0f}, max {n.max()}, sum {n.sum()}; {ref['n_reject'].sum()} rejected trials")
    assert nr.MAX_PASS == 128
    assert ref["converged"].all() and n.max() <= nr.MAX_PASS // 2
    assert np.isfinite(ref["H"]).all() and (ref["H"] >= 0).all() and (ref["gap"] <= TOL).all()


@pytest.mark.parametrize("name", ["planted", "img96_k3", "img96_k8"])
def test_reference_nested_fits_converge_within_half_the_cap(name):
    """The same for the k + 1 nested fits of ``presence`` (measured: at most 32 passes in a reduced fit)."""
    X, D = nr.case(name)
    out = nr.presence(X, D, None, TOL)
    print(f"{name}: at most {out['n_pass'].max(axis=1)} passes")
    assert out["converged"].all() and out["n_pass"].max() <= nr.MAX_PASS // 2
    assert (out["deviance_without"] >= out["deviance_ml"][None, :] - TOL).all()   # nested: up to the gap of the full fit


@pytest.mark.parametrize("name", nr.CASES)
def test_accepted_deviances_never_increase(name):
    assert nr.solved(name)["monotone"].all()


@pytest.mark.parametrize("name", nr.CASES)
def test_final_deviance_is_within_tol_of_the_optimum(name):
    """Both points are certified: the reference's by gap <= tol, the long run's by its own gap (EM's at tol = 1e-10 where EM gets
    there, else whatever its cap left it) - the two deviances differ by at most the larger of the two gaps."""
    ref, opt = nr.solved(name), nr.optimum(name)
    diff = ref["deviance"] - opt["deviance"]
    slack = 1e-9 * np.maximum(1.0, opt["deviance"])
    print(f"{name}: dev - dev_opt in [{diff.min():.3g}, {diff.max():.3g}], the long run's gap <= {opt['gap'].max():.3g}")
    assert (diff <= TOL + slack).all() and (diff >= -opt["gap"].clip(0) - slack).all()
    ev = pr.evaluate(*nr.case(name), ref["H"])
    live = ev["N"] > 0
    np.testing.assert_allclose(ev["deviance"][live], ref["deviance"][live], rtol=1e-12)   # the reported point is the returned h


@pytest.mark.parametrize("name", nr.CASES)
def test_two_summation_orders_agree_on_the_pass_counts(name):
    """The margin the GPU tests leave for accept / reject ties under the kernel's own order of summation, against a second order on the
    host: the pass counts differ in at most 1 % of the pixels (measured: in none)."""
    X, D = nr.case(name)
    a, b = nr.solved(name), nr.flipped(X, D, nr.start_from(X, D))
    differ = a["n_pass"] != b["n_pass"]
    print(f"{name}: {differ.sum()} of {differ.size} pixels differ in their pass count")
    assert differ.mean() <= 0.01


def test_em_does_not_converge_the_planted_image_within_the_cap():
    """What makes ``ml_unmix(method="newton", max_pass=128)`` on ``planted`` a call that the EM rule cannot answer."""
    X, D = nr.case("planted")
    em = pr.ml_unmix(X, D, nr.start_from(X, D), None, TOL, nr.MAX_PASS)
    print(f"EM: {em['converged'].sum()} of {em['converged'].size} pixels converged within {nr.MAX_PASS} passes")
    assert not em["converged"].all() and nr.solved("planted")["converged"].all()


def test_the_new_images_are_what_the_rule_exists_for():
    X, D = nr.case("low8")
    assert X.shape == (64, 400) and X.dtype == np.uint8 and D.shape == (64, 8) and 7 < X.sum(axis=0).mean() < 9
    X, D = nr.case("collinear")
    assert X.shape == (64, 300) and D.shape == (64, 4) and np.allclose(D[:, 3], 0.999 * D[:, 2] + 0.001 * D[:, 0], rtol=0, atol=0)
    # a tol no pixel can reach but by a gap that rounds to 0, to a cap of 100 passes: everything stays finite
    out = nr.ml_unmix(*nr.case("low8"), nr.start_from(*nr.case("low8")), None, 1e-300, 100)
    assert not out["converged"].all() and np.isfinite(out["H"]).all() and np.isfinite(out["deviance"]).all() and (out["H"] >= 0).all()


# ---- the binding and the refusals before any launch ---------------------------------------------------------------------------------------
def _s(*v):
    return (C.c_double * 8)(*v)


def test_entry_point_is_bound_and_the_wide_builds_refuse(lib):
    res, args = lib.SYMBOLS["espm_pixel_ml_newton"]
    em = lib.SYMBOLS["espm_pixel_ml"][1]
    assert res is C.c_int and len(args) == 22
    assert args[:19] == em[:19] and args[19:] == [C.c_void_p, C.c_size_t, C.c_void_p]   # espm_pixel_ml's, then state, its size, the stream
    assert lib.PMLN_STATE_EXTRA == 3
    one = C.c_void_p(8)
    for k in (12, 20):   # the 9..16 and the 17..32 component builds export a stub
        v = lib.variant(k)
        rc = v.lib.espm_pixel_ml_newton(one, 0, 0, 8, 8, 8, one, _s(1, 1, 1), 3, 7, 1e-14, 1e-3, 1, one, one, one, one, one, one, one, 1 << 20, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)


def test_host_side_argument_errors_need_no_device(lib):
    """Status codes of the narrow build's entry point for arguments it refuses before any launch: espm_pixel_ml's, and the state's."""
    f = lib.lib.espm_pixel_ml_newton
    one = C.c_void_p(8)   # (never dereferenced: every call below is refused on the host)
    s = _s(1, 1, 1)
    need = (3 + lib.PMLN_STATE_EXTRA) * 8 * 8   # k = 3, p = 8

    def call(x=one, layout=0, ld=8, n=8, p=8, s=s, k=3, mask=7, log_shift=1e-14, tol=1e-3, n_pass=1, h=one, state=one, nbytes=need):
        return f(x, 0, layout, ld, n, p, one, s, k, mask, log_shift, tol, n_pass, h, one, one, one, one, one, state, nbytes, None)

    assert call(k=9, mask=1) == lib.EUNSUPPORTED
    assert call(k=0, mask=1) == lib.EUNSUPPORTED
    assert call(x=None) == lib.EINVAL
    assert call(h=None) == lib.EINVAL
    assert call(s=None) == lib.EINVAL
    assert call(layout=2) == lib.EINVAL
    assert call(ld=7) == lib.EINVAL                     # ld below the row length
    assert b"ld=7" in lib.lib.espm_mu_last_error()
    assert call(layout=1, ld=7, p=16, nbytes=2 * need) == lib.EINVAL     # pixel-major: rows of n
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
    assert call(state=None) == lib.EINVAL
    assert call(nbytes=need - 1) == lib.EINVAL          # a state too small for (k + 3, p) doubles
    assert b"state" in lib.lib.espm_mu_last_error()
    with pytest.raises(ValueError):
        lib.check(call(nbytes=0))


def test_a_method_that_does_not_exist_is_refused_before_the_upload(lib, monkeypatch):
    from espm_amd import presence
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X, D = np.zeros((6, 10), np.float32), np.ones((6, 2))
    for f in (presence.ml_unmix, presence.presence):
        with pytest.raises(ValueError, match="method"):
            f(X, D, method="bogus")
        with pytest.raises(ValueError, match="method"):
            f(X, D, method=None)
        for method in presence.METHODS:   # the other refusals come first or after, whatever the method
            with pytest.raises(ValueError, match="channels"):
                f(X, np.ones((5, 2)), method=method)
    assert presence.METHODS == ("em", "newton")


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import presence
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X, D = pr.case("planted")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        presence.ml_unmix(X, D, method="newton")


def test_estimator_refuses_the_method_before_the_image(lib):
    import types

    from espm_amd.estimators import SmoothNMF
    est = SmoothNMF(n_components=2)
    est.W_, est.H_ = np.ones((6, 2)), np.ones((2, 10))
    est._image_argument = types.MethodType(lambda self, *a: pytest.fail("the image was reached"), est)
    with pytest.raises(ValueError, match="method"):
        est.presence_maps(np.zeros((6, 10)), method="bogus")
    assert not hasattr(est, "ml_method_")
