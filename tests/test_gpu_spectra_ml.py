"""The spectra ML on the device: the pass (csrc/mu_spectra_ml.hip, espm_spectra_ml_pass) against its definitions, the solver and the
nested tests of espm_amd/spectra_ml.py, and ``est.element_presence``.  tests/spectra_ml_reference.py holds the rule, the cases and
the derivation of the bounds; tests/test_spectra_ml_cpu.py holds what all of this rests on (the reference alone converges on every
case within half of MAX_PASS).

As in test_gpu_pixel_ml_newton.py the solver checks are SOLVER-AGNOSTIC: the certificate and the deviance are recomputed in numpy
from the returned W, and the optimum they are held against is the recorded end of a long EM run, itself certified from the
definitions.  The path is compared with the numpy restatement only in its length.  Every case carries one counted entry under the
floor (a zero row of G): ``unmodelled`` is 1 and the certificate has the slack the reference's docstring derives."""
import functools

import numpy as np
import pytest

import spectra_ml_reference as R
from spectral_reference import _ratio
from test_gpu_pixel_diagnostics import quiet

pytestmark = pytest.mark.gpu

TOL = 1e-3


@pytest.fixture(scope="module")
def sml():
    from espm_amd import spectra_ml
    return spectra_ml


# ---- the pass, through the entry point itself ---------------------------------------------------------------------------------------------
def _raw(X, D, H, layout="cm", k=None, scratch_short=0, null=None, log_shift=R.LOG_SHIFT):
    """espm_spectra_ml_pass on X (a host array (n, p), or a device tensor in ``layout`` with any row stride): dict of host arrays."""
    import torch

    from espm_amd import _image, _lib
    from espm_amd._image_args import layout_code
    from espm_amd.engine import _ptr, _stream
    if isinstance(X, torch.Tensor):
        Xd = X
    else:
        Xd = torch.from_numpy(np.ascontiguousarray(X if layout == "cm" else X.T)).cuda()
    n, p = (Xd.shape if layout == "cm" else Xd.shape[::-1])
    kk = D.shape[1]
    nt = kk * (kk + 1) // 2
    Dd, Hd = torch.from_numpy(np.ascontiguousarray(D)).cuda(), torch.from_numpy(np.ascontiguousarray(H)).cuda()
    dev, xs, ys = (torch.full((n,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3))
    q = torch.full((n, kk), -7.0, dtype=torch.float64, device="cuda")
    tri = torch.full((n, nt), -7.0, dtype=torch.float64, device="cuda")
    un = torch.full((1,), 99, dtype=torch.int64, device="cuda")   # (zeroed by the call)
    k = kk if k is None else k
    nbytes = int(_lib.lib.espm_spectra_ml_pass_scratch(n, p, kk))
    assert nbytes == -(-p // _lib.CDIAG_PCHUNK) * (3 + kk + nt) * n * 8
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    ptrs = dict(x=_ptr(Xd), d=_ptr(Dd), h=_ptr(Hd), dev=_ptr(dev), xsum=_ptr(xs), ysum=_ptr(ys), q=_ptr(q), a_tri=_ptr(tri), unmodelled=_ptr(un),
                scratch=_ptr(scratch))
    if null is not None:
        ptrs[null] = None
    _lib.check(_lib.lib.espm_spectra_ml_pass(ptrs["x"], _image.dtype_code(Xd.dtype), layout_code(layout), int(Xd.stride(0)), n, p, ptrs["d"],
                                             ptrs["h"], k, float(log_shift), ptrs["dev"], ptrs["xsum"], ptrs["ysum"], ptrs["q"], ptrs["a_tri"],
                                             ptrs["unmodelled"], ptrs["scratch"], nbytes - scratch_short, _stream()))
    torch.cuda.synchronize()
    A = np.empty((n, kk, kk))
    il, jl = R.tri_index(kk)
    A[:, il, jl] = A[:, jl, il] = tri.cpu().numpy()
    return dict(dev=dev.cpu().numpy(), xsum=xs.cpu().numpy(), ysum=ys.cpu().numpy(), Q=q.cpu().numpy(), A=A, unmodelled=int(un.item()))


KEYS = ("dev", "xsum", "ysum", "Q", "A")


def _same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in KEYS) and a["unmodelled"] == b["unmodelled"]


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("name", R.CASES)
def test_pass_sums_against_the_definitions(sml, name, layout):
    """The derived bounds (spectra_ml_reference: C1 p eps sum |t| for the deviance, sums of counts exact, C2 (p + k) eps relative for
    the model spectrum, C4 (p + k + 2) eps relative for every entry of Q and A); the worst ratios are printed before they are asserted."""
    X, G, W, H = R.case(name)
    n, p = X.shape
    k = H.shape[0]
    D = G @ W
    ref, out = R.sums(X, D, H), _raw(X, D, H, layout)
    r_dev = _ratio(np.abs(out["dev"] - ref["dev"]), R.C1 * p * R.EPS * ref["abs_terms"])
    r_y = _ratio(np.abs(out["ysum"] - ref["ysum"]), R.C2 * (p + k) * R.EPS * ref["ysum"])
    lim = R.C4 * (p + k + 2) * R.EPS
    r_q = _ratio(np.abs(out["Q"] - ref["Q"]), lim * np.abs(ref["Q"]))
    r_a = _ratio(np.abs(out["A"] - ref["A"]), lim * np.abs(ref["A"]))
    print(f"{name} {layout}: deviance {r_dev:.3g}, ysum {r_y:.3g}, Q {r_q:.3g}, A {r_a:.3g} of their bounds; unmodelled {out['unmodelled']}")
    assert all(np.isfinite(out[key]).all() for key in KEYS)
    assert r_dev <= 1 and r_y <= 1 and r_q <= 1 and r_a <= 1
    assert np.array_equal(out["xsum"], ref["xsum"]), "sums of counts are exact"
    assert out["unmodelled"] == ref["unmodelled"] == 1
    assert np.array_equal(out["A"], out["A"].transpose(0, 2, 1))


@pytest.mark.parametrize("name", ["k5", "k8", "seams"])
def test_layouts_dtypes_padded_rows_and_a_second_call_give_the_same_bits(sml, name):
    import torch
    X, G, W, H = R.case(name)
    D = G @ W
    want = _raw(X, D, H)
    assert _same(_raw(X, D, H), want), "a second call"
    for dtype in (np.uint8, np.uint16, np.float32, np.float64):
        for layout in ("cm", "pm"):
            assert _same(_raw(X.astype(dtype), D, H, layout), want), (dtype, layout)
    for layout, Xl in (("cm", X), ("pm", np.ascontiguousarray(X.T))):   # rows 13 elements longer than they say, filled with counts
        wide = torch.full((Xl.shape[0], Xl.shape[1] + 13), 255, dtype=torch.uint8, device="cuda")
        wide[:, :Xl.shape[1]] = torch.from_numpy(Xl).cuda()
        view = wide[:, :Xl.shape[1]]
        assert view.stride(0) == Xl.shape[1] + 13
        assert _same(_raw(view, D, H, layout), want), layout


def test_entry_point_refusals(sml):
    X, G, W, H = R.case("k1")
    D = G @ W
    for k in (0, 9):
        with pytest.raises(NotImplementedError, match=f"k={k}"):
            _raw(X, D, H, k=k)
    with pytest.raises(ValueError, match="scratch of .* bytes, .* needed"):
        _raw(X, D, H, scratch_short=8)
    for null in ("x", "d", "h", "dev", "q", "a_tri", "unmodelled", "scratch"):
        with pytest.raises(ValueError, match="bad arguments"):
            _raw(X, D, H, null=null)
    for shift in (0.0, -1e-14):
        with pytest.raises(ValueError, match="log_shift must be positive"):
            _raw(X, D, H, log_shift=shift)
    from espm_amd import _lib
    assert _lib.lib.espm_spectra_ml_pass_scratch(40, 70, 9) == 0 and _lib.lib.espm_spectra_ml_pass_scratch(0, 70, 1) == 0


# ---- the solver: solver-agnostic ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solved(name, layout="cm"):
    """The device's fit of a named case from W = 1 (shared: read-only)."""
    from espm_amd import spectra_ml
    X, G, _, H = R.case(name)
    return spectra_ml.ml_spectra(X if layout == "cm" else np.ascontiguousarray(X.T), G, H, tol=TOL, layout=layout)


def _certified(X, G, H, got, free=None):
    """What every returned point passes, whatever the path: the certificate and the deviance recomputed in numpy from W."""
    ev = R.evaluate(X, G, H, got["W"], free)
    F, _ = R.free_set(G, H, free)
    # r = (G^T Q) / a: Q within C4 (p + k + 2) eps (the pass's bound), n more additions in G^T Q - times 2 N in the gap
    n, p = X.shape
    assert got["converged"] and got["gap"] <= TOL and ev["gap"] <= TOL + 2 * ev["N"] * R.C4 * (p + n + H.shape[0] + 2) * R.EPS
    assert abs(got["deviance"] - ev["deviance"]) <= 1e-9 * abs(ev["deviance"])
    assert np.abs(got["channel_deviance"] - ev["channel_deviance"]).max() <= 1e-9 * abs(ev["deviance"])
    assert (got["W"] >= 0).all() and not got["W"][~F].any()
    np.testing.assert_allclose(ev["a"][F] @ got["W"][F], ev["N"], rtol=1e-14)   # W as scaled in step 1
    assert got["unmodelled"] == ev["unmodelled"]
    return ev


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("name", R.CASES)
def test_certificate_recomputed_in_numpy(sml, name, layout):
    X, G, _, H = R.case(name)
    got, ref, opt = _solved(name, layout), R.solved(name), R.optimum(name)
    print(f"{name} {layout}: passes {got['n_pass']} (reference {ref['n_pass']}), rejected {got['n_rejected']}, fallbacks {got['n_fallback']}; "
          f"dev - dev_opt = {got['deviance'] - opt['deviance']:.3g}, gap {got['gap']:.3g}")
    assert got["W"].shape == ref["W"].shape and got["channel_deviance"].shape == (X.shape[0],) and got["inert"].shape == ref["W"].shape
    _certified(X, G, H, got)
    assert got["deviance"] <= opt["deviance"] + TOL
    assert not got["inert"].any() and got["unmodelled"] == 1
    # the path's length: the margin covers accept / reject ties under another order of the sums
    assert got["n_pass"] <= 1.25 * ref["n_pass"] and got["n_pass"] <= R.MAX_PASS // 2


def test_a_free_set_a_start_with_holes_and_an_inert_entry(sml):
    X, G, _, H = R.case("k3")
    free = np.ones((6, 3), dtype=bool)
    free[2, 1] = free[5, 0] = False
    W0 = np.full((6, 3), 2.0)
    W0[0, 0], W0[3, 2] = 0.0, -1.0   # (not > 0: the fill)
    got, ref = sml.ml_spectra(X, G, H, W0=W0, free=free, tol=TOL), R.ml_spectra(X, G, H, W0, free, TOL)
    _certified(X, G, H, got, free)
    assert got["W"][2, 1] == 0 and got["W"][5, 0] == 0
    assert got["deviance"] <= ref["deviance"] + TOL and got["deviance"] >= _solved("k3")["deviance"] - TOL   # (a smaller feasible set)
    assert got["n_pass"] <= 1.25 * ref["n_pass"] and got["n_pass"] <= R.MAX_PASS // 2
    # a column of G that is all zero: its entries are inert - reported, held at 0, and the rest is fitted as without them
    Gz = np.array(G)
    Gz[:, 4] = 0.0
    got = sml.ml_spectra(X, Gz, H, tol=TOL)
    assert got["inert"][4].all() and got["inert"].sum() == 3 and not got["W"][4].any()
    _certified(X, Gz, H, got)


def test_an_image_without_counts_and_a_cap_too_small(sml):
    X, G, _, H = R.case("k1")
    got = sml.ml_spectra(np.zeros_like(X), G, H)
    assert not got["W"].any() and got["deviance"] == 0 and got["gap"] == 0 and got["n_pass"] == 0 and got["converged"]
    X, G, _, H = R.case("k8")
    short = sml.ml_spectra(X, G, H, tol=TOL, max_pass=2)
    assert not short["converged"] and short["n_pass"] == 2 and short["gap"] > TOL and np.isfinite(short["W"]).all()
    ev = R.evaluate(X, G, H, short["W"])   # the last accepted point: W, deviance and gap belong together
    assert abs(short["deviance"] - ev["deviance"]) <= 1e-9 * abs(ev["deviance"]) and abs(short["gap"] - ev["gap"]) <= 1e-6 * abs(ev["gap"])
    _certified(X, G, H, sml.ml_spectra(X, G, H, W0=short["W"], tol=TOL))


# ---- presence -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k3", "k1", "planted"])
def test_presence_against_the_reference(sml, name):
    """Each of the four deviances is within tol above its optimum and max(., 0) is 1-Lipschitz: |lr - lr_ref| <= 2 tol."""
    X, G, _, H = R.case(name)
    out, ref = sml.presence(X, G, H, tol=TOL), R.tested(name)
    m, k = G.shape[1], H.shape[0]
    E = len(ref["entries"])
    print(f"{name}: |lr - lr_ref| <= {np.nanmax(np.abs(out['lr'] - ref['lr'])):.3g}; passes {out['n_pass']} (reference {ref['n_pass']})")
    assert out["lr"].shape == out["pvalue"].shape == out["W_ml"].shape == (m, k) and np.array_equal(out["entries"], ref["entries"])
    assert out["converged"].shape == out["gap"].shape == out["n_pass"].shape == (1 + E,) and out["converged"].all()
    assert (out["gap"] <= TOL).all() and out["n_pass"].max() <= R.MAX_PASS // 2
    assert np.array_equal(np.isnan(out["lr"]), np.isnan(ref["lr"])) and np.array_equal(np.isnan(out["pvalue"]), np.isnan(out["lr"]))
    ok = ~np.isnan(ref["lr"])
    assert (np.abs(out["lr"] - ref["lr"])[ok] <= 2 * TOL).all()
    from espm_amd.presence import pvalue
    assert np.array_equal(out["pvalue"][ok], pvalue(out["lr"][ok]))
    full = _solved(name)
    assert np.array_equal(out["W_ml"], full["W"]) and out["deviance_ml"] == full["deviance"] and out["n_pass"][0] == full["n_pass"]
    if name == "k1":   # k = 1, m = 3: every entry can be removed; with one free entry its removal leaves none - NaN, and no fit
        one = np.zeros((3, 1), dtype=bool)
        one[1, 0] = True
        alone = sml.presence(X, G, H, free=one, tol=TOL)
        assert np.isnan(alone["lr"]).all() and alone["n_pass"][1] == 0 and np.array_equal(alone["entries"], [[1, 0]])
    if name == "planted":
        assert all(out["lr"][e, j] < 2.71 for e, j in R.PLANTED_AT)


def test_presence_of_a_subset_of_the_entries(sml):
    X, G, _, H = R.case("k3")
    full = sml.presence(X, G, H, tol=TOL)
    ent = np.array([[4, 2], [0, 0], [3, 1]])
    sub = sml.presence(X, G, H, entries=ent, tol=TOL)
    tested = np.zeros((6, 3), dtype=bool)
    tested[ent[:, 0], ent[:, 1]] = True
    assert np.array_equal(sub["entries"], ent) and np.isnan(sub["lr"][~tested]).all() and np.isnan(sub["pvalue"][~tested]).all()
    assert np.array_equal(sub["lr"][tested], full["lr"][tested]) and np.array_equal(sub["W_ml"], full["W_ml"])
    where = [int(np.flatnonzero((full["entries"] == e).all(axis=1))[0]) for e in ent]
    assert np.array_equal(sub["n_pass"][1:], full["n_pass"][1:][where]) and sub["n_pass"].shape == (4,)


# ---- the estimator and the adapter --------------------------------------------------------------------------------------------------------
ATTRS = ("W_ml_", "W_deviance_ml_", "W_presence_lr_", "W_presence_pvalue_", "W_ml_converged_", "W_ml_gap_", "W_ml_n_pass_", "W_presence_entries_")


def _fit(fixed_W=None, fp64=False, max_iter=30):
    from espm_amd.estimators import SmoothNMF
    X, G, _, _ = R.case("k3")
    est = SmoothNMF(n_components=3, G=np.array(G), shape_2d=(15, 20), max_iter=max_iter, tol=0.0, verbose=0, random_state=0, simplex_W=False,
                    simplex_H=True, fixed_W=fixed_W)   # (simplex_H: the image has a pixel without counts)
    if fp64:
        est.set_precision("fp64")
    quiet(est.fit, X.astype(np.float64 if fp64 else np.float32))
    return est, X


def test_estimator_and_adapter(sml):
    from espm_amd import hyperspy_adapter as ha
    est, X = _fit()
    with pytest.raises(AttributeError, match="element_presence"):
        ha.element_presence(est)
    kept = {a: np.array(getattr(est, a), copy=True) for a in ("W_", "H_", "G_")}
    out = est.element_presence(X=X)
    m, k = est.W_.shape
    E = len(est.W_presence_entries_)
    assert all(hasattr(est, a) for a in ATTRS) and (m, k) == (6, 3) and E == 18
    assert est.W_ml_.shape == est.W_presence_lr_.shape == est.W_presence_pvalue_.shape == est.W_.shape
    assert est.W_ml_converged_.shape == est.W_ml_gap_.shape == est.W_ml_n_pass_.shape == (1 + E,) and est.W_presence_entries_.shape == (E, 2)
    assert est.W_ml_converged_.all() and est.W_ml_n_pass_.max() <= R.MAX_PASS // 2 and out["lr"] is est.W_presence_lr_
    G, W, H = est._model_factors()
    want = sml.presence(X, G, H, W0=W, log_shift=est.log_shift)
    assert np.array_equal(want["lr"], est.W_presence_lr_) and np.array_equal(want["W_ml"], est.W_ml_)
    fit_dev = R.evaluate(X, G, H, W, log_shift=est.log_shift)["deviance"]
    print(f"deviance of the fit - W_deviance_ml_ = {fit_dev - est.W_deviance_ml_:.6g}; passes {est.W_ml_n_pass_}")
    assert est.W_deviance_ml_ <= fit_dev + TOL   # the ML over W >= 0 with H_ held: no regulariser, certified to tol
    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), f"{a} changed"
    tab = ha.element_presence(est)
    assert tab["lr"] is est.W_presence_lr_ and tab["W_ml"] is est.W_ml_ and set(tab) >= {"pvalue", "entries", "converged", "gap", "n_pass"}
    # the fp64-mode estimator, given the same W_ and H_: the analysis is fp64 whatever the precision
    est64, _ = _fit(fp64=True, max_iter=3)
    est64.W_, est64.H_ = est.W_, est.H_
    est64.element_presence(X=X)
    assert (np.abs(est64.W_presence_lr_ - est.W_presence_lr_) <= 2 * TOL).all()


def test_estimator_fixed_W(sml):
    fixed = -np.ones((6, 3))
    fixed[1, 2] = fixed[4, 0] = 0.0
    est, X = _fit(fixed_W=fixed)
    assert est.W_[1, 2] == 0 and est.W_[4, 0] == 0
    est.element_presence(X=X)
    held = fixed == 0
    assert not est.W_ml_[held].any() and np.isnan(est.W_presence_lr_[held]).all() and not np.isnan(est.W_presence_lr_[~held]).any()
    assert len(est.W_presence_entries_) == 16 and est.W_ml_converged_.all()
    fixed[2, 1] = 0.4
    pos, X = _fit(fixed_W=fixed, max_iter=3)
    with pytest.raises(NotImplementedError, match="positive"):
        pos.element_presence(X=X)
    assert not hasattr(pos, "W_ml_")
