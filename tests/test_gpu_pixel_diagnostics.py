"""pixel_diagnostics on the GPU (csrc/mu_diag.hip) against the numpy fp64 reference of tests/diag_reference.py, whose docstring
derives the two bounds used here:  |dev - ref| <= 8 n eps sum_c |t_c|  and  |H_std - ref| <= 64 k eps cond(F_j) ref.

The parity shapes are the smallest that cross every boundary of the kernel: three workgroups with a tail of 155 pixels, one and
eight components, both layouts, the four dtypes, more channels than one LDS chunk of D (ESPM_DIAG_CHUNK + 52), a row stride above
the row length.  Every image holds a pixel without counts, an all-zero channel and an entry of D H below log_shift."""
import contextlib
import io

import numpy as np
import pytest

import diag_reference as dr

pytestmark = pytest.mark.gpu


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.fixture(scope="module")
def measures():
    from espm_amd import measures
    return measures


def _chunk():
    from espm_amd import _lib
    return _lib.DIAG_CHUNK


# (n or None for "one LDS chunk + 52", p, k, layout, dtype, padded row stride)
PARITY = [
    (70, 23 * 29, 3, "cm", "float32", False),
    (70, 23 * 29, 1, "cm", "float32", False),
    (70, 23 * 29, 8, "pm", "uint8", False),
    (None, 300, 5, "pm", "uint16", True),
    (70, 64, 2, "cm", "float64", False),
]


@pytest.mark.parametrize("simplex", [False, True], ids=["free", "simplex"])
@pytest.mark.parametrize("n,p,k,layout,dtype,padded", PARITY, ids=[f"k{c[2]}_{c[3]}_{c[4]}" for c in PARITY])
def test_parity_with_numpy(measures, n, p, k, layout, dtype, padded, simplex):
    import torch
    n = _chunk() + 52 if n is None else n
    X, D, H, facts = dr.image(n, p, k, dtype, simplex)
    ref = dr.reference(X, D, H, simplex=simplex)
    assert ref["cond"].max() < 1e8, "the parity images must stay away from the NaN rule"
    Xin = X if layout == "cm" else np.ascontiguousarray(X.T)
    if padded:   # a device tensor whose rows are 12 elements apart from their length; the padding holds counts that must not be read
        wide = np.full((Xin.shape[0], Xin.shape[1] + 12), 999, dtype=Xin.dtype)
        wide[:, :Xin.shape[1]] = Xin
        Xin = torch.from_numpy(wide).to("cuda")[:, :Xin.shape[1]]
        assert Xin.stride(0) == wide.shape[1]
    out = measures.pixel_diagnostics(Xin, D, H, simplex_H=simplex, layout=layout)
    assert out["deviance"].dtype == np.float64 and out["deviance"].shape == (p,)
    assert out["H_std"].dtype == np.float64 and out["H_std"].shape == (k, p) and out["n_singular"] == 0
    dr.check(out, ref, n, k, f"n={n} p={p} k={k} {layout} {dtype} simplex={simplex}")
    if k == 1 and simplex:
        assert not out["H_std"].any(), "one component on the simplex has no freedom: exactly 0"
    # the floor is active where D H = 0 and X holds a count: that pixel's deviance carries x ln(x / log_shift)
    assert out["deviance"][facts["floor_pixel"]] > 2 * (3 * np.log(3 / dr.LOG_SHIFT) - 3) - 1e-6


def test_other_dtypes_and_a_device_tensor(measures):
    """int32 and float16 images are converted to a dtype that holds them exactly; a device tensor gives what the host array gives."""
    import torch
    X, D, H, _ = dr.image(70, 64, 2, "float64", False)
    Xi = np.floor(X)
    want = measures.pixel_diagnostics(Xi, D, H)
    for other in (Xi.astype(np.int32), Xi.astype(np.float16), Xi.astype(np.int16), torch.from_numpy(Xi).to("cuda"),
                  torch.from_numpy(Xi.astype(np.int64)).to("cuda")):
        got = measures.pixel_diagnostics(other, D, H)
        assert np.array_equal(got["deviance"], want["deviance"]) and np.array_equal(got["H_std"], want["H_std"])
    again = measures.pixel_diagnostics(Xi, D, H)
    assert np.array_equal(again["H_std"], want["H_std"]) and np.array_equal(again["deviance"], want["deviance"])   # no atomics on doubles


# ---- singular pixels ------------------------------------------------------------------------------------------------------------
def test_identical_spectra_make_every_pixel_singular(measures):
    n, p = 70, 300
    X, _, H, _ = dr.image(n, p, 2, "float32", False)
    D = np.repeat(dr.spectra(n, 1, 500.0), 2, axis=1)
    for simplex in (False, True):
        out = measures.pixel_diagnostics(X, D, H, simplex_H=simplex)
        assert np.isnan(out["H_std"]).all() and out["n_singular"] == p
        ref = dr.reference(X, D, H)
        assert np.isfinite(out["deviance"]).all()
        assert (np.abs(out["deviance"] - ref["deviance"]) <= 8 * n * dr.EPS * ref["abs_terms"]).all()


def test_one_singular_pixel_leaves_the_others_alone(measures):
    """F_j = D^T diag(1 / y_j) D of a full-rank D is singular for no finite y, so one pixel is made singular by the pivot rule: the
    spectra have disjoint supports (F_j is diagonal), and an abundance of 1e40 takes component 0's entry of F_j forty decades below
    the others', under k eps max diag(F_j)."""
    n, p, k, j = 70, 300, 3, 123
    rng = np.random.default_rng(11)
    c = np.arange(n, dtype=np.float64)[:, None]
    centres = (np.arange(k)[None, :] + 0.5) * n / k
    D = np.where(np.abs(c - centres) <= 8, 60.0 * np.exp(-0.5 * ((c - centres) / 3.0) ** 2), 0.0)
    H = rng.random((k, p)) + 0.1
    X = rng.poisson(D @ H).astype(np.float32)
    ref = dr.reference(X, D, H)
    assert ref["cond"].max() < 1e8
    H[0, j] = 1e40
    out = measures.pixel_diagnostics(X, D, H)
    assert out["n_singular"] == 1 and np.isnan(out["H_std"][:, j]).all()
    others = np.arange(p) != j
    assert np.isfinite(out["H_std"][:, others]).all()
    assert (np.abs(out["H_std"] - ref["H_std"])[:, others] <= (64 * k * dr.EPS * ref["cond"] * ref["H_std"])[:, others]).all()
    assert np.isfinite(out["deviance"]).all()
    assert (np.abs(out["deviance"] - ref["deviance"])[others] <= (8 * n * dr.EPS * ref["abs_terms"])[others]).all()


# ---- the estimator --------------------------------------------------------------------------------------------------------------
N, GRID, K = 60, (16, 20), 3


def _fit_image(with_G, seed=5):
    rng = np.random.default_rng(seed)
    p = GRID[0] * GRID[1]
    D = dr.spectra(N, K, 600.0)
    G = None
    if with_G:   # a dictionary of six peaks on a floor; the spectra are mixtures of them
        c = np.arange(N, dtype=np.float64)[:, None]
        G = np.exp(-0.5 * ((c - (np.arange(6)[None, :] + 0.5) * N / 6) / 2.5) ** 2) + 0.05
        D = G @ (rng.random((6, K)) ** 2 + 0.05)
        D *= 600.0 / D.sum(axis=0, keepdims=True)
    H = rng.random((K, p)) + 0.1
    H /= H.sum(axis=0, keepdims=True)
    X = rng.poisson(D @ H).astype(np.float64)
    assert X.sum(axis=0).min() > 0 and X.sum(axis=1).min() > 0   # no empty lines: X_ holds no log_shift fill
    return X, G


ESTIMATORS = {
    "plain": dict(hspy_comp=False, normalize=False, with_G=False, simplex_H=False),
    "hspy_normalize": dict(hspy_comp=True, normalize=True, with_G=False, simplex_H=True),
    "normalize_G": dict(hspy_comp=False, normalize=True, with_G=True, simplex_H=True),
    "hspy_G": dict(hspy_comp=True, normalize=False, with_G=True, simplex_H=False),
    "fp64": dict(hspy_comp=False, normalize=True, with_G=False, simplex_H=True, fp64=True),
}


@pytest.mark.parametrize("name", list(ESTIMATORS))
def test_estimator_method(measures, name):
    from espm_amd.estimators import SmoothNMF
    cfg = dict(ESTIMATORS[name])
    X, G = _fit_image(cfg.pop("with_G"))
    fp64 = cfg.pop("fp64", False)
    p = X.shape[1]
    est = SmoothNMF(n_components=K, G=G, shape_2d=GRID, max_iter=30, tol=0.0, verbose=0, random_state=0, simplex_W=not cfg["simplex_H"], **cfg)
    if fp64:
        est.set_precision("fp64")
    Xin = np.ascontiguousarray(X.T) if cfg["hspy_comp"] else X
    quiet(est.fit, Xin)
    kept = {a: np.array(getattr(est, a), copy=True) for a in ("W_", "H_", "G_", "components_")}
    kept["X_"], losses = np.array(np.asarray(est.X_), copy=True), list(est.losses_)

    out = est.pixel_diagnostics(Xin)
    D = np.asarray(est.G_ @ est.W_, dtype=np.float64)
    want = measures.pixel_diagnostics(X, D, np.asarray(est.H_, dtype=np.float64), simplex_H=cfg["simplex_H"], log_shift=est.log_shift)
    assert np.array_equal(est.deviance_, want["deviance"]) and np.array_equal(est.H_std_, want["H_std"])
    assert est.deviance_.shape == (p,) and est.H_std_.shape == est.H_.shape == (K, p)
    assert np.array_equal(out["deviance"], est.deviance_) and out["n_singular"] == want["n_singular"] == 0
    assert np.array_equal(out["H_std"], est.H_std_.T if cfg["hspy_comp"] else est.H_std_)
    ref = dr.reference(X, D, est.H_, log_shift=est.log_shift, simplex=cfg["simplex_H"])
    assert ref["cond"].max() < 1e8
    dr.check(want, ref, N, K, f"{name}: X passed")

    none = est.pixel_diagnostics()   # the fit's X_ un-scaled: the same image to rounding (it has no empty lines)
    dr.check(dict(deviance=est.deviance_, H_std=est.H_std_), ref, N, K, f"{name}: X=None")
    assert none["H_std"].shape == ((p, K) if cfg["hspy_comp"] else (K, p))

    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), f"{a} changed"
    assert list(est.losses_) == losses

    from espm_amd import hyperspy_adapter as ha
    dev_map, std_map = ha.diagnostic_maps(est)
    assert dev_map.shape == GRID and std_map.shape == (K,) + GRID and dev_map[3, 7] == est.deviance_[3 * GRID[1] + 7]

    with pytest.raises(ValueError, match="channels"):
        est.pixel_diagnostics(Xin[:-1] if not cfg["hspy_comp"] else Xin[:, :-1])
    with pytest.raises(ValueError, match="pixels"):
        est.pixel_diagnostics(Xin[:, :-1] if not cfg["hspy_comp"] else Xin[:-1])


def test_estimator_refusals(measures, monkeypatch):
    from sklearn.exceptions import NotFittedError

    from espm_amd.estimators import SmoothNMF
    X, _ = _fit_image(False)
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=K).pixel_diagnostics(X)
    est = SmoothNMF(n_components=9, max_iter=3, tol=0.0, verbose=0, random_state=0)
    quiet(est.fit, X)
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    with pytest.raises(NotImplementedError, match="9 components"):
        est.pixel_diagnostics(X)
    with pytest.raises(NotImplementedError, match="9 components"):
        est.pixel_diagnostics()
    assert not hasattr(est, "deviance_")


# ---- what the number means ------------------------------------------------------------------------------------------------------
def test_h_std_is_the_spread_of_the_estimates(measures):
    """4000 Poisson pixels of one spectrum D h (k = 3, n = 70, ~500 counts), each unmixed by 300 H-only multiplicative iterations
    from the true h (no regulariser, no simplex): the empirical standard deviation of the estimates lies within 10 % of the mean
    H_std of those pixels.  The sampling error of a standard deviation over 4000 draws is 1.1 %, the bound is asymptotic at this
    dose; 10 % catches a wrong formula (a factor of 2, a missing square root), it is not a measurement.  The estimator is fitted
    for two iterations on a corner of the image only to exist; its spectra are then set to D (``simplex_W`` stays on, so that
    ``unmix`` returns H in D's units: utils.rescaled_DH applies only without any simplex)."""
    from espm_amd.estimators import SmoothNMF
    n, k, p = 70, 3, 4000
    rng = np.random.default_rng(42)
    D = dr.spectra(n, k, 500.0)
    h = np.array([0.5, 0.3, 0.2])
    X = rng.poisson(np.tile((D @ h)[:, None], (1, p))).astype(np.float64)
    est = SmoothNMF(n_components=k, max_iter=2, tol=0.0, no_stop_criterion=True, verbose=0, random_state=0)
    quiet(est.fit, X[:, :256])
    est.set_params(max_iter=300)
    est.W_ = D.copy()
    H_est = np.asarray(quiet(est.unmix, X, H=np.tile(h[:, None], (1, p))), dtype=np.float64)
    spread = H_est.std(axis=1, ddof=1)
    out = measures.pixel_diagnostics(X, D, H_est)
    bar = out["H_std"].mean(axis=1)
    print(f"mean estimate {H_est.mean(axis=1)}, empirical std {spread}, mean H_std {bar}, ratio {spread / bar}")
    assert out["n_singular"] == 0
    assert (np.abs(spread / bar - 1) < 0.10).all()
