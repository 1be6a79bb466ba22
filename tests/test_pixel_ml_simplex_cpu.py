"""The simplex rule of the pixel ML and its capped interval root finder without a device: the conditions the GPU tests
(test_gpu_pixel_ml_simplex.py) rest on, held by the numpy restatement alone (tests/pixel_ml_simplex_reference.py); the binding of
espm_pixel_ml_simplex and its refusals before any launch; and the new argument errors of ``espm_amd.presence``, the estimator and the
adapter before any upload."""
import ctypes as C

import numpy as np
import pytest

import pixel_ml_newton_reference as nr
import pixel_ml_simplex_reference as sr

TOL = 1e-3
LR_TOL = 1e-2
FITTED = tuple(n for n in sr.CASES if n != "img96_k1")   # the cases where something is fitted: k >= 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
def test_the_cases_are_at_the_datas_dose():
    for name in sr.CASES:
        X, D = sr.case(name)
        ratio = X.sum(axis=0, dtype=np.float64).mean() / D.sum(axis=0).mean()
        want = {"bright3": 1.0 / 3.0, "dim03": 1.0 / 0.3}.get(name, 1.0)
        assert abs(ratio - want) <= 1e-12 * want, name
    X, D = sr.case("zero_row")
    assert not D[0].any() and X[0, -1] > 0 and not X[1:, -1].any() and not X[0, :-1].any()
    assert sr.case("img96_k8")[1].shape[1] == 8


@pytest.mark.parametrize("name", sr.CASES)
def test_every_fit_converges_within_half_the_cap(name):
    """Every full fit, and every pinned fit at t in {0, h_ml, the midpoint to 1, 1}, converges within 64 passes, half of
    max_pass = 128 (measured: at most 35, the full fit of ``low8``), on the simplex to the stated bound, every value finite."""
    X, D = sr.case(name)
    k = D.shape[1]
    full = sr.solved(name)
    fits = [(full, None)] + ([(sr.pinned(name, label), k - 1) for label in sr.LABELS] if k > 1 else [])
    most = 0
    for fit, pin in fits:
        assert fit["converged"].all() and fit["nonfinite"] == 0 and (fit["gap"] <= TOL).all()
        assert np.isfinite(fit["H"]).all() and (fit["H"] >= 0).all() and fit["monotone"].all()
        ev = sr.evaluate(X, D, fit["H"], pin)
        assert (np.abs(ev["sum"] - fit["total"]) <= sr.sum_bound(k, fit["total"])).all()
        np.testing.assert_allclose(ev["deviance"], fit["deviance"], rtol=1e-12, atol=1e-12)
        most = max(most, int(fit["n_pass"].max()))
    print(f"{name}: at most {most} passes in a fit")
    assert sr.MAX_PASS == 128 and most <= sr.MAX_PASS // 2


@pytest.mark.parametrize("name", sr.CASES)
def test_every_endpoint_finishes_within_half_the_cap(name):
    """Every end of every interval is found within 32 evaluations, half of max_eval = 64 (measured: at most 9), every pinned fit of
    the root finder within 64 passes (at most 35), and 0 <= lower <= H_ml <= upper <= 1."""
    out = sr.intervals_solved(name)
    print(f"{name}: evaluations per end <= {out['n_eval'].max()}, a pinned fit <= {out['max_fit_pass']} passes; upper == 1 in "
          f"{(out['upper'] == 1).sum()} entries, lower == 0 in {(out['lower'] == 0).sum()}")
    assert sr.MAX_EVAL == 64 and out["converged"].all() and out["n_eval"].max() <= sr.MAX_EVAL // 2
    assert out["max_fit_pass"] <= sr.MAX_PASS // 2
    assert (0 <= out["lower"]).all() and (out["lower"] <= out["H_ml"]).all() and (out["H_ml"] <= out["upper"]).all() and (out["upper"] <= 1).all()


def test_the_cap_is_reached_exactly_and_the_boundary_too():
    """``planted`` has pixels that could be all one phase (upper == 1 exactly) and abundances on the boundary (lower == 0 exactly, and
    exactly where the simplex presence statistic is within the threshold)."""
    out, pres = sr.intervals_solved("planted"), sr.presence_solved("planted")
    assert (out["upper"] == 1).any() and (out["lower"] == 0).any()
    clear = np.abs(pres["lr"] - out["threshold"]) > 2 * TOL   # (two certified deviances on either side)
    assert np.array_equal((out["lower"] == 0)[clear], (pres["lr"] <= out["threshold"])[clear])
    one = sr.intervals_solved("img96_k1")   # one component: h = 1, nothing to fit, the interval ends at the cap
    assert (one["H_ml"] == 1).all() and (one["upper"] == 1).all() and not one["n_eval"][:, 1].any()


@pytest.mark.parametrize("name", sr.CASES)
def test_certificate_holds_against_the_long_run(name):
    """dev - dev_opt - gap <= 1e-9 max(1, dev) against runs at tol = 1e-10, for the full fit and the four pinned ones.  The last pixel
    of ``zero_row`` has its counts under the floor (``unmodelled``): there the certificate is of the floored problem, and it is
    left out as documented."""
    k = sr.case(name)[1].shape[1]
    pairs = [(sr.solved(name), sr.solved(name, 1e-10))]
    if k > 1:
        pairs += [(sr.pinned(name, label), sr.pinned(name, label, 1e-10)) for label in sr.LABELS]
    keep = np.ones(pairs[0][0]["deviance"].size, dtype=bool)
    if name == "zero_row":
        keep[-1] = False
        assert sr.solved(name)["unmodelled"] == 1
    for fit, opt in pairs:
        assert opt["converged"].all()
        excess = fit["deviance"] - opt["deviance"] - fit["gap"]
        print(f"{name}: dev - dev_opt - gap <= {excess[keep].max():.3g}")
        assert (excess <= 1e-9 * np.maximum(1.0, fit["deviance"]))[keep].all()


@pytest.mark.parametrize("name", ("planted", "low8", "dim03", "img96_k5"))
def test_slope_is_the_derivative_of_the_profile(name):
    """The slope 2 (g_pin - lin / total) against a central difference of the profile deviance in t, both sides solved to 1e-10, at the
    midpoint between h_ml and 1 (away from both ends of [0, 1]).  The profile is convex with second derivative of the order of the
    counts N, so a step d leaves an error of about N d^2 in the quotient: d = 1e-4 and the bound 5e-6 (1 + |slope|) + 1e-5 N."""
    X, D = sr.case(name)
    k = D.shape[1]
    d = 1e-4
    t = np.minimum(sr.pins(name)["mid"], 1.0 - 2 * d)   # (a pixel that is all the last phase has its midpoint at the cap)
    at, lo, hi = (sr.ml_unmix(X, D, sr.solved(name)["H"], None, k - 1, t + e, 1e-10, 20000) for e in (0.0, -d, d))
    assert at["converged"].all() and lo["converged"].all() and hi["converged"].all()
    fd = (hi["deviance"] - lo["deviance"]) / (2 * d)
    N = X.sum(axis=0, dtype=np.float64)
    err = np.abs(fd - at["slope"])
    print(f"{name}: |slope - central difference| <= {err.max():.3g}, relative {(err / (1 + np.abs(at['slope']))).max():.3g}")
    assert (err <= 5e-6 * (1.0 + np.abs(at["slope"])) + 1e-5 * N).all()


@pytest.mark.parametrize("name", sr.CASES)
def test_the_simplex_costs_deviance(name):
    """The simplex model is a sub-model of the free-scale one: its minimum is not below the Newton rule's (both at tol = 1e-10)."""
    X, D = sr.case(name)
    free = nr.ml_unmix(X, D, None, None, 1e-10, 20000)
    con = sr.solved(name, 1e-10)
    assert free["converged"].all() and con["converged"].all()
    diff = con["deviance"] - free["deviance"]
    print(f"{name}: simplex - free deviance in [{diff.min():.3g}, {diff.max():.3g}]")
    assert (diff >= -1e-9 * np.maximum(1.0, free["deviance"])).all()
    if name in sr.MISFIT:   # a dose that is off costs every pixel with counts
        assert (diff[X.sum(axis=0) > 0] > 0.1).all()


def test_the_special_pixels():
    """An empty pixel and a pixel whose counts no component reaches go to the vertex of the least s (the lowest index on ties) in one
    pass and certify there with gap exactly 0; one component fits nothing; t = 1 and an empty set are done in the first pass."""
    X, D = sr.case("zero_row")
    fit = sr.solved("zero_row")
    s = D.sum(axis=0)
    best = int(np.argmin(s))
    for q in (5, X.shape[1] - 1):
        assert not X[1:, q].any()
        want = np.zeros(4)
        want[best] = 1.0
        assert np.array_equal(fit["H"][:, q], want) and fit["gap"][q] == 0 and fit["n_pass"][q] == 1 and fit["converged"][q]
    assert abs(fit["deviance"][5] - 2.0 * (D @ fit["H"][:, 5]).clip(sr.LOG_SHIFT).sum()) <= 1e-12 * fit["deviance"][5]
    one = sr.solved("img96_k1")
    assert (one["H"] == 1).all() and not one["n_pass"].any() and (one["gap"] == 0).all()
    sub = sr.ml_unmix(X, D, components=[2])
    assert (sub["H"][2] == 1).all() and not sub["H"][[0, 1, 3]].any() and not sub["n_pass"].any() and (sub["gap"] == 0).all()
    top = sr.pinned("planted", "one")
    assert not top["H"][:-1].any() and (top["H"][-1] == 1).all() and not top["n_pass"].any() and (top["gap"] == 0).all()
    Xp, Dp = sr.case("planted")
    lone = sr.ml_unmix(Xp, Dp, None, [], 0, 0.25)
    assert lone["converged"].all() and not lone["n_pass"].any() and (lone["H"][0] == 0.25).all() and not lone["H"][1:].any()
    with pytest.raises(ValueError):
        sr.ml_unmix(Xp, Dp, components=[])
    with pytest.raises(ValueError):
        sr.presence(*sr.case("img96_k1"))


def test_a_value_outside_the_unit_interval_stops_the_pixel():
    X, D = sr.case("planted")
    t = np.full(X.shape[1], 0.5)
    t[3], t[7], t[11], t[13] = -1.0, np.nan, np.inf, 1.0 + 1e-12
    fit = sr.ml_unmix(X, D, None, None, 0, t)
    bad = np.zeros(t.size, dtype=bool)
    bad[[3, 7, 11, 13]] = True
    assert fit["nonfinite"] == 4 and not fit["converged"][bad].any() and fit["converged"][~bad].all() and not fit["n_pass"][bad].any()


def test_presence_is_zero_where_the_abundance_is():
    """The step never puts an abundance AT zero (it keeps 0.01 h): exact zeros are those of a vertex - in ``zero_row`` the empty pixel
    and the pixel whose counts nothing reaches.  There the fit without j finds the same vertex and the same deviance, bit for bit."""
    pres = sr.presence_solved("zero_row")
    assert pres["converged"].all()
    gone = pres["H_ml"] == 0
    assert gone[:, 5].sum() == 3 and gone[:, -1].sum() == 3 and (pres["lr"][gone] == 0).all()
    assert sr.presence_solved("planted")["converged"].all()


@pytest.mark.parametrize("name", FITTED)
def test_two_summation_orders_agree_on_the_counts(name):
    """The margin the GPU tests leave for accept / reject ties: under a second order of every sum the pass counts differ in few pixels
    and the total by far less than the quarter the GPU tests allow."""
    X, D = sr.case(name)
    a, b = sr.solved(name), sr.flipped(X, D)
    diff = a["n_pass"] != b["n_pass"]
    print(f"{name}: {diff.sum()} of {diff.size} pixels differ in n_pass; totals {a['n_pass'].sum()} and {b['n_pass'].sum()}")
    assert b["converged"].all() and b["n_pass"].sum() <= 1.1 * a["n_pass"].sum() and a["n_pass"].sum() <= 1.1 * b["n_pass"].sum()


# ---- the binding and the refusals before any launch ---------------------------------------------------------------------------------------
def _s(*v):
    return (C.c_double * 8)(*v)


def test_entry_point_is_bound_and_the_wide_builds_refuse(lib):
    res, args = lib.SYMBOLS["espm_pixel_ml_simplex"]
    assert res is C.c_int and args == lib.SYMBOLS["espm_pixel_ml_pinned"][1]
    from espm_amd import presence
    assert presence.ALL_METHODS == presence.METHODS + ("simplex",)
    one = C.c_void_p(8)
    for k in (12, 20):   # the 9..16 and the 17..32 component builds export a stub
        v = lib.variant(k)
        rc = v.lib.espm_pixel_ml_simplex(one, 0, 0, 8, 8, 8, one, _s(1, 1, 1), 3, 3, 2, one, 1e-14, 1e-3, 1, one, one, one, one, one, one, one, one, 1 << 20, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)


def test_host_side_argument_errors_need_no_device(lib):
    """Status codes of the narrow build's entry point for arguments it refuses before any launch."""
    f = lib.lib.espm_pixel_ml_simplex
    one = C.c_void_p(8)   # (never dereferenced: every call below is refused on the host)
    s = _s(1, 1, 1)
    need = (3 + lib.PMLN_STATE_EXTRA) * 8 * 8   # k = 3, p = 8

    def call(x=one, layout=0, ld=8, n=8, p=8, s=s, k=3, mask=3, pin=2, t=one, log_shift=1e-14, tol=1e-3, n_pass=1, h=one, slope=one, state=one,
             nbytes=need):
        return f(x, 0, layout, ld, n, p, one, s, k, mask, pin, t, log_shift, tol, n_pass, h, one, one, slope, one, one, one, state, nbytes, None)

    assert call(k=9, mask=1, pin=1) == lib.EUNSUPPORTED
    assert call(k=0, mask=0, pin=0) == lib.EUNSUPPORTED
    # the pinned entry's refusals
    assert call(x=None) == lib.EINVAL
    assert call(h=None) == lib.EINVAL
    assert call(s=None) == lib.EINVAL
    assert call(layout=2) == lib.EINVAL
    assert call(ld=7) == lib.EINVAL
    assert b"ld=7" in lib.lib.espm_mu_last_error()
    assert call(n=0) == lib.EINVAL
    assert call(log_shift=0.0) == lib.EINVAL
    assert call(tol=0.0) == lib.EINVAL and call(tol=-1.0) == lib.EINVAL
    assert call(n_pass=0) == lib.EINVAL
    assert call(mask=8) == lib.EINVAL                   # a bit beyond the k components
    assert call(pin=3) == lib.EINVAL
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
    # its own: no pinned component is pin = -1, and then the set may not be empty; below -1 is no component; t and slope with a pin
    assert call(pin=-2) == lib.EINVAL
    assert b"pin=-2" in lib.lib.espm_mu_last_error()
    assert call(pin=-1, mask=0) == lib.EINVAL
    assert b"empty mask" in lib.lib.espm_mu_last_error()
    assert call(t=None) == lib.EINVAL and call(slope=None) == lib.EINVAL
    assert b"slope" in lib.lib.espm_mu_last_error()
    # ... and what it does NOT refuse on these grounds: pin = -1 with t and slope null gets as far as the state
    assert call(pin=-1, mask=7, t=None, slope=None, state=None) == lib.EINVAL
    assert b"state" in lib.lib.espm_mu_last_error()
    assert call(pin=2, mask=0, state=None) == lib.EINVAL   # an empty set with a pin, too
    assert b"state" in lib.lib.espm_mu_last_error()
    with pytest.raises(ValueError):
        lib.check(call(nbytes=0))


def test_argument_errors_come_before_the_upload(lib, monkeypatch):
    from espm_amd import _image, presence
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X, D = np.zeros((6, 10), np.float32), np.ones((6, 2))
    with pytest.raises(ValueError, match="method"):
        presence.ml_unmix(X, D, method="Simplex")
    with pytest.raises(ValueError, match="one component under the simplex"):
        presence.presence(X, np.ones((6, 1)), method="simplex")
    for t in (1.0 + 1e-9, 2.0, np.array([0.5] * 9 + [1.5])):
        with pytest.raises(ValueError, match="must not exceed 1"):
            presence.ml_unmix_pinned(X, D, 0, t, simplex=True)
    for t in (-1.0, np.nan, np.inf, np.ones(9)):
        with pytest.raises(ValueError, match="t must"):
            presence.ml_unmix_pinned(X, D, 0, t, simplex=True)
    with pytest.raises(ValueError, match="pinned component 0 is in"):
        presence.ml_unmix_pinned(X, D, 0, 0.5, components=[0, 1], simplex=True)
    with pytest.raises(ValueError, match="components"):
        presence.ml_unmix(X, D, components=[], method="simplex")
    with pytest.raises(ValueError, match="level"):
        presence.intervals(X, D, level=1.0, simplex=True)
    with pytest.raises(ValueError, match="H0"):
        presence.intervals(X, D, H0=np.ones((2, 9)), simplex=True)
    with pytest.raises(NotImplementedError, match="9 components"):
        presence.intervals(X, np.ones((6, 9)), simplex=True)


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import presence
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X, D = sr.case("planted")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        presence.ml_unmix(X, D, method="simplex")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        presence.ml_unmix_pinned(X, D, 0, 0.5, simplex=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        presence.intervals(X, D, simplex=True)


def test_estimator_refuses_a_fit_without_the_simplex_first(lib):
    """``method="simplex"`` / ``simplex=True`` on an estimator without ``simplex_H``: a ValueError before every other refusal - before
    "not fitted", before a method that does not exist matters, before the image."""
    import types

    from espm_amd import hyperspy_adapter as ha
    from espm_amd.estimators import SmoothNMF
    free = SmoothNMF(n_components=2, simplex_H=False)
    with pytest.raises(ValueError, match="simplex_H"):
        free.presence_maps(method="simplex")          # (not fitted either: the simplex refusal comes first)
    with pytest.raises(ValueError, match="simplex_H"):
        free.abundance_intervals(level=2.0, simplex=True)   # (a bad level too)
    with pytest.raises(ValueError, match="simplex_H"):
        ha.presence_maps(free, method="simplex")
    est = SmoothNMF(n_components=2, simplex_H=True, simplex_W=False)
    with pytest.raises(Exception, match="not fitted"):
        est.presence_maps(method="simplex")
    with pytest.raises(Exception, match="not fitted"):
        est.abundance_intervals(simplex=True)
    est.W_, est.H_ = np.ones((6, 2)), np.full((2, 10), 0.5)
    est._image_argument = types.MethodType(lambda self, *a: pytest.fail("the image was reached"), est)
    with pytest.raises(ValueError, match="level"):
        est.abundance_intervals(0.0, np.zeros((6, 10)), simplex=True)
    with pytest.raises(ValueError, match="components"):
        est.abundance_intervals(X=np.zeros((6, 10)), components=[5], simplex=True)
    assert not hasattr(est, "H_interval_simplex_") and not hasattr(est, "ml_method_")


def test_the_committed_resource_table_meets_the_register_target():
    """profiles/pixel_ml_simplex_resources.txt (the compiler's own remarks for mu_pixel_ml_simplex.hip) against the pinned kernel's
    table: 64 instances, no scratch, no vector spills, and in every instance at least the pinned kernel's waves per SIMD."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def table(name):
        rows = {}
        for line in open(os.path.join(root, "profiles", name)):
            m = re.match(r"pixel_ml_\w+_kernel<(.*?)> \| (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) (\d+)", line)
            if m:
                rows[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
        return rows

    new, old = table("pixel_ml_simplex_resources.txt"), table("pixel_ml_pinned_resources.txt")
    assert len(new) == 64 and set(new) == set(old)
    for key, (vgprs, _, scratch, waves, _, spills, _) in new.items():
        assert scratch == 0 and spills == 0 and vgprs <= 256 and waves >= old[key][3], key
