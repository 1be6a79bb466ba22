"""Concentration intervals on the device: the batched pass (csrc/mu_spectra_ml.hip, espm_spectra_ml_pass_batch) against the single
pass bit for bit, ``spectra_ml.ml_spectra_pinned`` and ``intervals`` against the numpy definition of
tests/spectra_ml_pinned_reference.py, and ``est.concentration_intervals``.  tests/test_spectra_ml_intervals_cpu.py holds what this rests
on: the reference alone converges at every end within half of the caps.

The interval checks are SOLVER-AGNOSTIC: every returned end is held against long runs of the numpy rule (tol = 1e-8), with the bound
|g*(t) - dev* - q_level| <= lr_tol + tol + 1e-9 dev* that follows from the two certificates and the stop; the path is compared with
the reference only in its length."""
import functools

import numpy as np
import pytest

import spectra_ml_pinned_reference as P
import spectra_ml_reference as R
from test_gpu_pixel_diagnostics import quiet
from test_gpu_spectra_ml import _raw as _single

pytestmark = pytest.mark.gpu

TOL, LR_TOL = 1e-3, 1e-2
SENTINEL = -7.0


@pytest.fixture(scope="module")
def sml():
    from espm_amd import spectra_ml
    return spectra_ml


# ---- the batched pass, through the entry point itself -------------------------------------------------------------------------------------
def _batch(X, Ds, H, layout="cm", active=None, k=None, n_models=None, scratch_short=0, null=None):
    """espm_spectra_ml_pass_batch on the host array X (n, p) at the models Ds (B, n, k): dict of host arrays with a leading B; the
    outputs start at SENTINEL and the counters at 99."""
    import torch

    from espm_amd import _image, _lib
    from espm_amd._image_args import layout_code
    from espm_amd.engine import _ptr, _stream
    Xd = torch.from_numpy(np.ascontiguousarray(X if layout == "cm" else X.T)).cuda()
    n, p = X.shape
    Ds = np.ascontiguousarray(Ds, dtype=np.float64)
    B, _, kk = Ds.shape
    nt = kk * (kk + 1) // 2
    Dd, Hd = torch.from_numpy(Ds).cuda(), torch.from_numpy(np.array(H)).cuda()   # (the cases are read-only: a copy)
    f = dict(dtype=torch.float64, device="cuda")
    dev, ys, q, tri = (torch.full(s, SENTINEL, **f) for s in ((B, n), (B, n), (B, n, kk), (B, n, nt)))
    un = torch.full((B,), 99, dtype=torch.int64, device="cuda")
    act = None if active is None else torch.tensor(active, dtype=torch.uint8, device="cuda")
    nbytes = int(_lib.lib.espm_spectra_ml_pass_batch_scratch(n, p, kk, B))
    assert nbytes == B * int(_lib.lib.espm_spectra_ml_pass_scratch(n, p, kk))
    scratch = torch.empty(nbytes // 8, **f)
    ptrs = dict(x=_ptr(Xd), d=_ptr(Dd), h=_ptr(Hd), dev=_ptr(dev), ysum=_ptr(ys), q=_ptr(q), a_tri=_ptr(tri), unmodelled=_ptr(un), scratch=_ptr(scratch))
    if null is not None:
        ptrs[null] = None
    _lib.check(_lib.lib.espm_spectra_ml_pass_batch(ptrs["x"], _image.dtype_code(Xd.dtype), layout_code(layout), int(Xd.stride(0)), n, p, ptrs["d"],
                                                   ptrs["h"], kk if k is None else k, B if n_models is None else n_models,
                                                   None if act is None else _ptr(act), float(R.LOG_SHIFT), ptrs["dev"], ptrs["ysum"], ptrs["q"],
                                                   ptrs["a_tri"], ptrs["unmodelled"], ptrs["scratch"], nbytes - scratch_short, _stream()))
    torch.cuda.synchronize()
    return dict(dev=dev.cpu().numpy(), ysum=ys.cpu().numpy(), Q=q.cpu().numpy(), tri=tri.cpu().numpy(), unmodelled=un.cpu().numpy())


def _models(name):
    """(X, (3, n, k) models, H): G W, 0.5 G W and a perturbed W."""
    X, G, W, H = R.case(name)
    rng = np.random.default_rng(5)
    return X, np.stack([G @ W, 0.5 * (G @ W), G @ (W * rng.uniform(0.5, 1.5, W.shape))]), H


@functools.lru_cache(maxsize=None)
def _single_pass(name, b):
    """The single pass of model b of ``_models`` on the u8, channel-major image (the single pass gives the same bits for every layout
    and dtype: test_gpu_spectra_ml.py), with the triangle as the entry point wrote it."""
    X, Ds, H = _models(name)
    out = _single(X, Ds[b], H)
    il, jl = R.tri_index(H.shape[0])
    return dict(dev=out["dev"], ysum=out["ysum"], Q=out["Q"], tri=out["A"][:, il, jl], unmodelled=out["unmodelled"])


def _equal(got, b, want):
    return all(np.array_equal(got[key][b], want[key]) for key in ("dev", "ysum", "Q", "tri")) and got["unmodelled"][b] == want["unmodelled"]


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("name", ["k8", "seams", "k5"])
def test_batch_pass_equals_the_single_pass_bit_for_bit(sml, name, layout, dtype):
    X, Ds, H = _models(name)
    X = X.astype(dtype)
    got = _batch(X, Ds, H, layout)
    for b in range(3):
        assert _equal(got, b, _single_pass(name, b)), f"model {b} of 3"
    rev = _batch(X, Ds[::-1], H, layout)
    for b in range(3):
        assert _equal(rev, 2 - b, _single_pass(name, b)), f"model {b}, reversed order"
    for b in range(3):
        assert _equal(_batch(X, Ds[b:b + 1], H, layout), 0, _single_pass(name, b)), f"model {b} alone"
    again = _batch(X, Ds, H, layout)
    assert all(np.array_equal(again[key], got[key]) for key in got), "a second call"


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("name", ["k8", "seams", "k5"])
def test_a_retired_model_is_never_touched(sml, name, layout):
    X, Ds, H = _models(name)
    got = _batch(X, Ds, H, layout, active=[1, 0, 1])
    assert all((got[key][1] == SENTINEL).all() for key in ("dev", "ysum", "Q", "tri")) and got["unmodelled"][1] == 99
    assert _equal(got, 0, _single_pass(name, 0)) and _equal(got, 2, _single_pass(name, 2))
    none = _batch(X, Ds, H, layout, active=[0, 0, 0])
    assert all((none[key] == SENTINEL).all() for key in ("dev", "ysum", "Q", "tri")) and (none["unmodelled"] == 99).all()
    every = _batch(X, Ds, H, layout, active=[1, 3, 255])   # (any value but 0 is active)
    assert all(_equal(every, b, _single_pass(name, b)) for b in range(3))


def test_batch_entry_point_refusals(sml):
    from espm_amd import _lib
    X, Ds, H = _models("k1")
    for k in (0, 9):
        with pytest.raises(NotImplementedError, match=f"k={k}"):
            _batch(X, Ds, H, k=k)
    for bad in (0, _lib._D["ESPM_SML_MAX_MODELS"] + 1):
        with pytest.raises(ValueError, match=f"n_models={bad}"):
            _batch(X, Ds, H, n_models=bad)
    for null in ("x", "d", "h", "dev", "ysum", "q", "a_tri", "unmodelled", "scratch"):
        with pytest.raises(ValueError, match="bad arguments"):
            _batch(X, Ds, H, null=null)
    n, p = X.shape
    need = int(_lib.lib.espm_spectra_ml_pass_batch_scratch(n, p, 1, 3))
    with pytest.raises(ValueError, match=f"scratch of {need - 1} bytes, {need} needed"):
        _batch(X, Ds, H, scratch_short=1)
    q = _lib.lib.espm_spectra_ml_pass_batch_scratch
    assert q(n, p, 1, 0) == 0 and q(n, p, 1, _lib._D["ESPM_SML_MAX_MODELS"] + 1) == 0 and q(n, p, 9, 3) == 0 and q(0, p, 1, 3) == 0
    assert 1 <= _lib._D["ESPM_SML_MAX_MODELS"] <= 65535
    # active = null means all models
    got = _batch(X, Ds, H, active=None)
    assert all(_equal(got, b, _single_pass("k1", b)) for b in range(3))


# ---- one point of the profile -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full(name):
    from espm_amd import spectra_ml
    X, G, _, H = R.case(name)
    return spectra_ml.ml_spectra(X, G, H, tol=TOL)


@pytest.mark.parametrize("where", ["zero", "ml", "twice"])
@pytest.mark.parametrize("name", ["k3", "k1", "planted"])
def test_pinned_fit_recomputed_in_numpy(sml, name, where):
    """deviance, gap and slope recomputed from the returned W by the reference's evaluation, to the pass's derived rounding bounds.
    The device's D = G W is a product of non-negative terms rounded in another order: every entry, and so every y, within (m + 1) eps
    relative of numpy's.  Deviance: C1 p eps sum |t| (the pass), n eps dev (the sum over the channels, terms >= 0) and, from D,
    2 (m + 1) eps sum |y - x| (dt / dy = 1 - x / y).  Every entry of q = G^T Q: C4 (p + k + 2) eps (the pass), n eps (the product with
    G) and (m + 1) eps (from D), relative, Q >= 0 - together e.  So gap = 2 sum_M (a - q) W + 2 N max(max_M q / a - 1, 0) moves by at
    most 2 e (sum_M q W + N max_M q / a), plus the rounding of its own sum, 2 |M| eps sum_M (a + q) W; slope = 2 (a_pin - q_pin) by
    2 e q_pin."""
    X, G, _, H = R.case(name)
    n, p = X.shape
    k = H.shape[0]
    F, _ = R.free_set(G, H)
    pin = tuple(int(v) for v in np.argwhere(F)[-1])
    W_ml = _full(name)["W"]
    t = dict(zero=0.0, ml=W_ml[pin], twice=2 * W_ml[pin] + 1)[where]
    got = sml.ml_spectra_pinned(X, G, H, pin, t, W0=W_ml, tol=TOL)
    ev = P.evaluate(X, G, H, got["W"], pin)
    M = F.copy()
    M[pin] = False
    m = G.shape[1]
    e = (R.C4 * (p + k + 2) + n + m + 1) * R.EPS
    terms = R.sums(X, G @ got["W"], H)["abs_terms"].sum()
    away = np.abs(np.maximum(G @ got["W"] @ H, R.LOG_SHIFT) - X).sum()
    b_dev = R.C1 * p * R.EPS * terms + n * R.EPS * abs(ev["deviance"]) + 2 * (m + 1) * R.EPS * away
    b_gap = 2 * e * (float(ev["q"][M] @ got["W"][M]) + ev["N"] * (ev["q"][M] / ev["a"][M]).max()) \
        + 2 * M.sum() * R.EPS * float((ev["a"][M] + ev["q"][M]) @ got["W"][M])
    b_slope = 2 * e * ev["q"][pin]
    print(f"{name} {where}: t = {t:.4g}, passes {got['n_pass']}, |d deviance| {abs(got['deviance'] - ev['deviance']):.3g} of {b_dev:.3g}, "
          f"|d gap| {abs(got['gap'] - ev['gap']):.3g} of {b_gap:.3g}, |d slope| {abs(got['slope'] - ev['slope']):.3g} of {b_slope:.3g}")
    assert got["converged"] and got["gap"] <= TOL and got["n_pass"] <= P.MAX_PASS // 2
    assert got["W"][pin] == t and (got["W"] >= 0).all() and not got["W"][~F].any()
    assert abs(got["deviance"] - ev["deviance"]) <= b_dev and abs(got["gap"] - ev["gap"]) <= b_gap and abs(got["slope"] - ev["slope"]) <= b_slope
    assert got["unmodelled"] == ev["unmodelled"] and got["channel_deviance"].shape == (n,)
    assert abs(got["channel_deviance"].sum() - got["deviance"]) <= n * R.EPS * abs(got["deviance"])
    want = P.ml_spectra_pinned(X, G, H, pin, t, W_ml, None, TOL)
    assert got["n_pass"] <= 1.25 * want["n_pass"] and abs(got["deviance"] - want["deviance"]) <= TOL


def test_a_free_set_of_the_pin_alone_is_one_pass(sml):
    X, G, _, H = R.case("k3")
    one = np.zeros((6, 3), dtype=bool)
    one[2, 1] = True
    got = sml.ml_spectra_pinned(X, G, H, (2, 1), 1.5, free=one)
    ev = P.evaluate(X, G, H, got["W"], (2, 1), one)
    assert got["converged"] and got["n_pass"] == 1 and got["gap"] == 0 and got["W"].sum() == 1.5
    assert abs(got["deviance"] - ev["deviance"]) <= 1e-12 * ev["deviance"] and abs(got["slope"] - ev["slope"]) <= 1e-9 * abs(ev["slope"])


# ---- the intervals ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _intervals(name, layout="cm", batch=None):
    from espm_amd import spectra_ml
    X, G, _, H = R.case(name)
    return spectra_ml.intervals(X if layout == "cm" else np.ascontiguousarray(X.T), G, H, tol=TOL, lr_tol=LR_TOL, layout=layout, batch=batch)


def _check(name, out):
    """Test 5's conditions on an ``intervals`` dict of a whole case."""
    ref = P.solved(name)
    worst, worst0, passes = P.check_ends(name, out, LR_TOL, TOL)   # (asserts the long-run bound at every end)
    print(f"{name}: batch {out['batch']}, {out['n_lockstep']} lockstep passes for {out['n_pass'].sum()} passes of {out['converged'].size} ends "
          f"(reference {ref['n_pass'].sum()}); |phi| <= {worst:.3g}, phi at the zero ends <= {worst0:.3g}; long runs within {passes} passes")
    E = len(ref["entries"])
    assert np.array_equal(out["entries"], ref["entries"]) and out["converged"].shape == out["n_eval"].shape == out["n_pass"].shape == (E, 2)
    assert out["converged"].all() and out["n_eval"].max() <= P.MAX_EVAL // 2
    assert out["n_pass"].sum() <= 1.25 * ref["n_pass"].sum()
    lo, hi, W = out["lower"], out["upper"], out["W_ml"]
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo >= 0).all() and (lo <= W).all() and (W <= hi).all()
    assert out["threshold"] == P.threshold(0.95) and out["level"] == 0.95


@pytest.mark.parametrize("name,layout", [("k1", "cm"), ("k3", "cm"), ("k3", "pm"), ("k8", "cm")])
def test_interval_ends_against_the_long_runs(sml, name, layout):
    out = _intervals(name, layout)
    _check(name, out)
    full = _full(name)
    assert out["n_full_pass"] == full["n_pass"] and out["unmodelled"] == full["unmodelled"] == 1 and not out["inert"].any()
    if layout == "cm":
        assert np.array_equal(out["W_ml"], full["W"]) and out["deviance_ml"] == full["deviance"]


def test_batch_of_one_and_the_default_batch(sml):
    X, G, _, H = R.case("k3")
    auto, one = _intervals("k3"), _intervals("k3", batch=1)
    assert auto["batch"] == 36 and one["batch"] == 1 and one["n_lockstep"] == one["n_pass"].sum() and auto["n_lockstep"] < one["n_lockstep"] / 8
    _check("k3", one)
    _check("k3", auto)
    five = sml.intervals(X, G, H, tol=TOL, lr_tol=LR_TOL, batch=5)   # (a batch that does not divide the 36 ends)
    _check("k3", five)
    again = sml.intervals(X, G, H, tol=TOL, lr_tol=LR_TOL)
    for key in ("W_ml", "lower", "upper", "converged", "n_eval", "n_pass"):
        assert np.array_equal(again[key], auto[key]), f"{key}: a repeated call"
    assert again["deviance_ml"] == auto["deviance_ml"]


@pytest.mark.parametrize("name", ["planted", "k8"])
def test_lower_is_exactly_zero_where_the_presence_test_does_not_reject(sml, name):
    X, G, _, H = R.case(name)
    out = _intervals(name)
    pres = sml.presence(X, G, H, tol=TOL, max_pass=P.MAX_PASS)
    away = np.abs(pres["lr"] - out["threshold"]) > 2 * TOL
    excluded = int((~away).sum())
    print(f"{name}: {excluded} entries within 2 tol of the decision; lower == 0 at {(out['lower'] == 0).sum()} of {away.size}")
    assert excluded == 0
    assert np.array_equal((out["lower"] == 0)[away], (pres["lr"] <= out["threshold"])[away])
    assert out["converged"].all()
    if name == "planted":
        zero = np.zeros(out["lower"].shape, dtype=bool)
        for e, j in R.PLANTED_AT:
            zero[e, j] = True
        assert np.array_equal(out["lower"] == 0, zero) and (out["upper"][zero] > 0).all()


def test_a_subset_holes_an_inert_entry_no_counts_and_a_cap_too_small(sml):
    X, G, _, H = R.case("k3")
    full = _intervals("k3")
    ent = np.array([[4, 2], [0, 0], [3, 1]])
    sub = sml.intervals(X, G, H, entries=ent, tol=TOL, lr_tol=LR_TOL)
    tested = np.zeros((6, 3), dtype=bool)
    tested[ent[:, 0], ent[:, 1]] = True
    assert np.array_equal(sub["entries"], ent) and np.isnan(sub["lower"][~tested]).all() and np.isnan(sub["upper"][~tested]).all()
    assert sub["converged"].shape == sub["n_eval"].shape == sub["n_pass"].shape == (3, 2) and sub["converged"].all() and sub["batch"] == 6
    P.check_ends("k3", sub, LR_TOL, TOL)   # (each end is the same problem as in the whole case, in a batch of another size: the same bound)
    assert (sub["lower"][tested] > 0).all() and (sub["lower"][tested] < sub["W_ml"][tested]).all() and (sub["W_ml"][tested] < sub["upper"][tested]).all()
    # a free set with holes, one of them asked for; and a column of G that is all zero: its entries are inert
    free = np.ones((6, 3), dtype=bool)
    free[2, 1] = free[5, 0] = False
    Gz = np.array(G)
    Gz[:, 4] = 0.0
    got = sml.intervals(X, Gz, H, free=free, entries=np.array([[2, 1], [1, 1], [4, 0]]), tol=TOL, lr_tol=LR_TOL)
    assert got["inert"][4].all() and got["inert"].sum() == 3 and not got["W_ml"][4].any() and got["W_ml"][2, 1] == 0
    assert got["converged"].all() and np.array_equal(got["n_eval"][[0, 2]], np.zeros((2, 2))) and (got["n_eval"][1] > 0).all()
    assert np.isnan(got["lower"][2, 1]) and np.isnan(got["upper"][4, 0]) and 0 < got["lower"][1, 1] < got["W_ml"][1, 1] < got["upper"][1, 1]
    opt = R.ml_spectra(X, Gz, H, got["W_ml"], free, 1e-8, 20000)   # the long runs of this model: the bound of ``P.check_ends``
    for t in (got["lower"][1, 1], got["upper"][1, 1]):
        long = P.ml_spectra_pinned(X, Gz, H, (1, 1), t, got["W_ml"], free, 1e-8, 20000)
        assert opt["converged"] and long["converged"]
        assert abs(long["deviance"] - opt["deviance"] - got["threshold"]) <= LR_TOL + TOL + 1e-9 * opt["deviance"]
    # an image without counts: W_ml = 0, every lower end exactly 0 without a fit, every upper end the root of 2 a t = q_level
    X1, G1, _, H1 = R.case("k1")
    none = sml.intervals(np.zeros_like(X1), G1, H1, tol=TOL, lr_tol=LR_TOL)
    a = R.column_sums(G1, H1)
    assert not none["W_ml"].any() and not none["lower"].any() and none["converged"].all() and not none["n_eval"][:, 0].any()
    np.testing.assert_allclose(none["upper"], none["threshold"] / (2 * a), rtol=1e-9)
    # a cap too small: not converged, NaN, no exception
    short = sml.intervals(X, G, H, entries=ent, tol=TOL, lr_tol=LR_TOL, max_eval=1)
    assert not short["converged"].any() and (short["n_eval"] == 1).all() and np.isnan(short["lower"]).all() and np.isnan(short["upper"]).all()
    assert np.array_equal(short["W_ml"], full["W_ml"])


# ---- the estimator and the adapter --------------------------------------------------------------------------------------------------------
ATTRS = ("W_lower_", "W_upper_", "W_interval_level_", "W_interval_entries_", "W_interval_converged_", "W_interval_n_eval_", "W_ml_", "W_deviance_ml_")


def _fit(fixed_W=None, G=True, hspy_comp=False, max_iter=30):
    from espm_amd.estimators import SmoothNMF
    X, Gd, _, _ = R.case("k3")
    est = SmoothNMF(n_components=3, G=np.array(Gd) if G else None, shape_2d=(15, 20), max_iter=max_iter, tol=0.0, verbose=0, random_state=0,
                    simplex_W=False, simplex_H=True, fixed_W=fixed_W, hspy_comp=hspy_comp)
    X = np.ascontiguousarray(X.T) if hspy_comp else X   # (hspy_comp: the rows of X are pixels)
    quiet(est.fit, X.astype(np.float32))
    return est, X


@pytest.mark.parametrize("hspy_comp", [False, True])
def test_estimator_and_adapter(sml, hspy_comp):
    from espm_amd import hyperspy_adapter as ha
    fixed = -np.ones((6, 3))
    fixed[1, 2] = fixed[4, 0] = 0.0
    est, X = _fit(fixed_W=fixed, hspy_comp=hspy_comp)
    with pytest.raises(AttributeError, match="concentration_intervals"):
        ha.concentration_intervals(est)
    kept = {a: np.array(getattr(est, a), copy=True) for a in ("W_", "H_", "G_")}
    out = est.concentration_intervals(X=X)
    held = fixed == 0
    assert all(hasattr(est, a) for a in ATTRS) and est.W_lower_.shape == est.W_upper_.shape == est.W_ml_.shape == est.W_.shape == (6, 3)
    assert est.W_interval_entries_.shape == (16, 2) and est.W_interval_converged_.shape == est.W_interval_n_eval_.shape == (16, 2)
    assert est.W_interval_level_ == 0.95 and est.W_interval_converged_.all() and out["lower"] is est.W_lower_
    assert np.isnan(est.W_lower_[held]).all() and np.isnan(est.W_upper_[held]).all() and not est.W_ml_[held].any()
    assert not any(held[e, j] for e, j in est.W_interval_entries_)
    assert (est.W_lower_[~held] <= est.W_ml_[~held]).all() and (est.W_ml_[~held] <= est.W_upper_[~held]).all() and (est.W_lower_[~held] >= 0).all()
    G, W, H = est._model_factors()
    want = sml.intervals(X, G, H, W0=W, free=~held, log_shift=est.log_shift, layout="pm" if hspy_comp else "cm")
    assert np.array_equal(want["lower"], est.W_lower_, equal_nan=True) and np.array_equal(want["upper"], est.W_upper_, equal_nan=True)
    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), f"{a} changed"
    tab = ha.concentration_intervals(est)
    assert tab["lower"] is est.W_lower_ and tab["upper"] is est.W_upper_ and set(tab) >= {"W_ml", "level", "entries", "converged", "n_eval"}
    est.concentration_intervals(X=X, level=0.68, entries=np.array([[0, 0]]))
    assert est.W_interval_level_ == 0.68 and np.isnan(est.W_upper_).sum() == 17 and est.W_upper_[0, 0] < want["upper"][0, 0]


def test_estimator_refusals(sml):
    fixed = -np.ones((6, 3))
    fixed[2, 1] = 0.4
    pos, X = _fit(fixed_W=fixed, max_iter=3)
    with pytest.raises(NotImplementedError, match="positive"):
        pos.concentration_intervals(X=X)
    none, X = _fit(G=False, max_iter=3)
    with pytest.raises(NotImplementedError, match="dictionary or physics model G"):
        none.concentration_intervals(X=X)
    ok, X = _fit(max_iter=3)
    with pytest.raises(ValueError, match="level"):
        ok.concentration_intervals(X=X, level=1.0)
    assert not any(hasattr(est, "W_upper_") for est in (pos, none, ok))
