"""transform(): the H of new data against fitted spectra (an H-only fit), on the GPU against the numpy oracle.

The yardstick is ``oracle.mu_oracle.fit(Xs, k, G=G_, W=Wf, fixed_W=Wf, H=H0, ...)`` (tests/test_transform_cpu.py: what that call is),
at the project's standing tolerances: loss history 1e-5 relative, H 5e-5 absolute, and the same number of
iterations under the stop rules - on cases whose stop in the oracle is not marginal (asserted on the oracle's own numbers: at the
stopping iteration and the one before it, every quantity a rule compares with ``tol`` is a factor of 2 away from it)."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import mu_oracle as oc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_RTOL, H_ATOL = 1e-5, 5e-5


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _truth(n, p, k, seed, m=None):
    rng = np.random.default_rng(seed)
    ell = np.linspace(0.0, 1.0, n)[:, None]
    centres = rng.uniform(0.1, 0.9, size=(1, 24))
    atoms = np.exp(-0.5 * ((ell - centres) / 0.03) ** 2) + 0.02     # (n, 24) peaks on a floor
    if m is None:
        G, D = None, atoms[:, :k] + 0.3 * atoms[:, k:2 * k].mean(axis=1, keepdims=True)
        if k > 12:
            D = D + 0.2 * rng.random((n, k))
    else:
        G = atoms[:, :m]
        D = G @ (rng.random((m, k)) ** 3 + 0.01)
    D = D / D.sum(axis=0, keepdims=True)
    H = rng.random((k, p)) ** 2 + 0.02
    H /= H.sum(axis=0, keepdims=True)
    return G, D, H, rng


def _draw(kind, D, H, rng):
    """Counts of the image D H on the store ``kind`` (what the engine's choice of a store goes by: integer counts and their density,
    counts above 255, values a bf16 holds exactly, anything else)."""
    n = D.shape[0]
    if kind in ("ell", "ell_heavy"):
        X = rng.poisson(0.25 * n * (D @ H)).astype(np.float64)        # ~ a quarter of the entries non-zero
        if kind == "ell_heavy":
            idx = rng.choice(X.size, size=12, replace=False)
            X.flat[idx] = rng.integers(300, 4000, size=12)
        return X
    X = rng.poisson(1.2 * n * (D @ H)).astype(np.float64)            # (a low dose: H off the simplex stays O(10), where fp32 resolves 5e-5)
    if kind == "u8":
        return np.minimum(X, 255.0)
    if kind == "bf16":
        return np.minimum(X, 120.0) * 0.5                            # half-integers below 2^7: exact in bf16, not integers
    return X + rng.random(X.shape)                                    # f32


CASES = {
    # name: (store, k, columns of G or None, regularisation, estimator arguments, what is special, chained?)
    "ell_k3_simplex_lap": ("ell", 3, None, "simplex_lap", {}, None, 1),
    "ell_heavy_k5_simplex_lap": ("ell_heavy", 5, None, "simplex_lap", {}, None, 0),   # (on the simplex: a heavy pixel's H off it is ~1e3, beyond fp32 at 5e-5)
    "u8_k5_G_simplex_lap": ("u8", 5, 9, "simplex_lap", {}, None, 1),
    "bf16_k8_plain": ("bf16", 8, None, "plain", {}, None, 1),
    "f32_k3_G_mu": ("f32", 3, 7, "mu", {}, None, 1),
    "ell_k12_simplex_lap": ("ell", 12, None, "simplex_lap", {}, None, 1),
    "u8_k12_plain": ("u8", 12, None, "plain", {}, None, 1),
    "f32_k20_simplex_lap": ("f32", 20, None, "simplex_lap", {}, None, 0),   # (on the simplex: the 17..32 build contracts on the matrix cores with operands split into two bf16 halves, ~2^-16 relative - 5e-5 absolute needs |H| <= 1)
    "bmd_k3": ("f32", 3, None, "plain", dict(algo="bmd"), None, 0),
    "l2_surrogate_k3": ("f32", 3, None, "simplex_lap", dict(algo="l2_surrogate"), None, 0),
    "normalize_ell_k3": ("ell", 3, None, "simplex_lap", dict(normalize=True), None, 1),
    "hspy_u8_k5": ("u8", 5, None, "mu", dict(hspy_comp=True), None, 1),
    "other_grid_ell_k5": ("ell", 5, None, "simplex_lap", {}, "other_grid", 1),
    "empty_lines_ell_k3": ("ell", 3, None, "simplex_lap", {}, "empty_lines", 1),
    "empty_lines_u8_k5": ("u8", 5, None, "mu", {}, "empty_lines", 1),
}
# (tol, max_iter) of every case: values at which the oracle's stop is not marginal (module docstring; found on the CPU, asserted below).
# The H-only rule converges linearly, so a loss rule that fires after a long run always fires marginally (successive decreases differ by
# far less than a factor of 4): the long runs end by the iteration limit with every rule a factor of 2 from firing at the iteration
# before, the runs that end by the loss rule do so at their second iteration, at a large tol.
MAX_ITER = 40
PARAMS = {
    "ell_k3_simplex_lap": (1e-4, 8), "ell_heavy_k5_simplex_lap": (1e-2, MAX_ITER), "u8_k5_G_simplex_lap": (1e-4, 16), "bf16_k8_plain": (5e-2, MAX_ITER),
    "f32_k3_G_mu": (1e-4, 16), "ell_k12_simplex_lap": (1e-4, 12), "u8_k12_plain": (1e-4, 16), "f32_k20_simplex_lap": (1e-4, 12),
    "bmd_k3": (1e-4, 12), "l2_surrogate_k3": (1e-4, 12), "normalize_ell_k3": (1e-4, 12), "hspy_u8_k5": (5e-2, MAX_ITER),
    "other_grid_ell_k5": (1e-4, 8), "empty_lines_ell_k3": (1e-4, 8), "empty_lines_u8_k5": (1e-4, 16),
}


def build_case(name):
    """(estimator arguments, X of the fit, its grid, X_new, its grid, the oracle's regularisation arguments)."""
    store, k, m, reg, extra, special, _ = CASES[name]
    n, fit_grid = 48, (12, 10)
    new_grid = (9, 14) if special == "other_grid" else fit_grid
    seed = sorted(CASES).index(name)
    G, D, H, rng = _truth(n, fit_grid[0] * fit_grid[1], k, seed, m)
    X_fit = _draw(store, D, H, rng)
    Hn = rng.random((k, new_grid[0] * new_grid[1])) ** 2 + 0.02
    Hn /= Hn.sum(axis=0, keepdims=True)
    X_new = _draw(store, D, Hn, rng)
    if special == "empty_lines":
        X_fit[5, :] = 0.0          # (the channel is empty in both images: a detector bin below its threshold)
        X_new[5, :] = 0.0
        X_new[:, 17] = 0.0
    regs = {"simplex_lap": dict(simplex_H=True, simplex_W=False, lambda_L=1.0),
            "mu": dict(mu=np.linspace(0.05, 0.3, k), simplex_H=False, simplex_W=True),
            "plain": dict(simplex_H=False, simplex_W=True)}[reg]
    if extra.get("algo") == "bmd":
        regs = dict(regs, simplex_W=False, simplex_H=True)   # (the Bregman W update has no simplex, updates.py:40-48)
    est_kw = dict(n_components=k, G=G, verbose=0, max_iter=PARAMS[name][1], tol=PARAMS[name][0], **regs, **extra)
    return est_kw, X_fit, fit_grid, X_new, new_grid, regs


def oracle_transform(est, X_new, new_grid, H0, regs, tol, algo, max_iter=MAX_ITER, **kw):
    scale = float(est.norm_factor_) if est.normalize else 1.0
    Wf = np.maximum(np.asarray(est.W_, dtype=np.float64) * scale, oc.LOG_SHIFT)   # (W_ may be float32: its entries on the floor read back a rounding below it)
    lam = regs.get("lambda_L", 0.0)
    return oc.fit(np.asarray(X_new, dtype=np.float64) * scale, est.n_components, G=None if est.G is None else np.asarray(est.G_, dtype=np.float64),
                  W=Wf.copy(), fixed_W=Wf.copy(), H=None if H0 is None else H0.copy(), lambda_L=lam, mu=regs.get("mu", 0),
                  simplex_H=regs["simplex_H"], simplex_W=regs["simplex_W"], shape_2d=new_grid if lam else None, tol=tol, max_iter=max_iter,
                  algo=algo, **kw)


def assert_stop_not_marginal(ref, tol):
    """Every comparison with ``tol`` that the stop rules (base.py:354-378) made at the last two iterations is a factor of 2 clear."""
    n, losses, rel_h, init = ref["n_iter"], ref["losses"], ref["rel"][:, 1], ref["eval_init"]
    assert np.all(ref["rel"][:, 0] == 0.0)

    def signed(i):   # (eval_before - eval_after) / eval_init at iteration i (1-based)
        return np.inf if i < 2 else (losses[i - 2] - losses[i - 1]) / init

    def goes_on(i):
        assert rel_h[i - 1] > 2 * tol and signed(i) > 2 * tol, (i, rel_h[i - 1], signed(i), tol)
    if n >= 2:
        goes_on(n - 1)
    if ref["exit"] == "rel":
        assert rel_h[n - 1] < tol / 2, (rel_h[n - 1], tol)
    elif ref["exit"] == "loss":
        assert rel_h[n - 1] > 2 * tol and abs(signed(n)) < tol / 2, (rel_h[n - 1], signed(n), tol)
    else:
        assert ref["exit"] == "max_iter", ref["exit"]   # (decided by the count alone)


@pytest.fixture(scope="module")
def SmoothNMF():
    from espm_amd.estimators import SmoothNMF as cls
    return cls


def _fitted(SmoothNMF, est_kw, X_fit, fit_grid):
    est = SmoothNMF(shape_2d=fit_grid, **est_kw)
    est.set_params(max_iter=6, no_stop_criterion=True)
    quiet(est.fit, X_fit.T if est.hspy_comp else X_fit)
    est.set_params(max_iter=est_kw["max_iter"], no_stop_criterion=est_kw.get("no_stop_criterion", False))
    return est


FITTED = ("W_", "H_", "G_", "X_", "losses_", "rel_", "n_iter_", "components_", "const_KL_")


@pytest.mark.parametrize("name", sorted(CASES))
def test_transform_matches_the_oracle(SmoothNMF, name, monkeypatch):
    """1, 2 and 4 of the issue: parity, the fitted attributes untouched, the path that ran.  With ESPM_H_CHAIN=1 - the library is handed
    the second record buffer - so that the chained launch runs wherever it is built and espm_mu_h_chain_applies is held to exactly those
    configurations; the default (the general path everywhere: the chained launch measured no faster) is
    test_default_is_the_general_path's."""
    monkeypatch.setenv("ESPM_H_CHAIN", "1")
    store, k, m, reg, extra, special, chained = CASES[name]
    est_kw, X_fit, fit_grid, X_new, new_grid, regs = build_case(name)
    est = _fitted(SmoothNMF, est_kw, X_fit, fit_grid)
    before = {a: np.array(getattr(est, a), copy=True) for a in FITTED}
    engine_before = est._engine
    supplied = name in ("u8_k5_G_simplex_lap", "f32_k20_simplex_lap", "other_grid_ell_k5")   # (H handed over; the others: H = None, updates.py:213-221)
    H0 = None
    if supplied:
        rng = np.random.default_rng(99)
        H0 = rng.random((k, X_new.shape[1])) + 0.2
        H0 /= H0.sum(axis=0, keepdims=True)
    tol, max_iter = PARAMS[name]
    ref = oracle_transform(est, X_new, new_grid, H0, regs, tol, extra.get("algo", "log_surrogate"), max_iter)
    assert_stop_not_marginal(ref, tol)

    arg_X = X_new.T if est.hspy_comp else X_new
    arg_H = None if H0 is None else (H0.T if est.hspy_comp else H0)
    # (transform where the estimator's rows are pixels - hspy_comp - and unmix, the same computation, for X (channels, pixels))
    assert hasattr(est, "transform") == bool(est.hspy_comp)
    Hn = quiet(est.transform if est.hspy_comp else est.unmix, arg_X, H=arg_H, shape_2d=new_grid if special == "other_grid" else None)
    if est.hspy_comp:
        assert Hn.shape == (X_new.shape[1], k)
        Hn = Hn.T
    print(f"{name}: n_iter {est.transform_n_iter_} (oracle {ref['n_iter']}, {ref['exit']}), path {est.transform_path_}, "
          f"max|dH| {np.abs(Hn - ref['H']).max():.2e}, max rel loss {np.abs(np.array(est.transform_losses_) / ref['losses'][:len(est.transform_losses_)] - 1).max():.2e}")
    assert est.transform_n_iter_ == ref["n_iter"]
    np.testing.assert_allclose(est.transform_losses_, ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(Hn, ref["H"], rtol=0, atol=H_ATOL)
    np.testing.assert_allclose(est.transform_rel_, ref["rel"][:, 1], rtol=2e-2, atol=2e-5)
    # the path: the store the case was drawn for, and the one-launch iteration exactly where it is built
    want_store = {"ell_heavy": "ell"}.get(store, store)
    if special == "empty_lines" and store != "ell":
        want_store = "f32"   # (a dense store keeps the reference's log_shift fill, which is neither an integer nor a bf16 value)
    assert est.transform_path_["x_store"] == want_store and (est.transform_path_["n_heavy"] > 0) == (store == "ell_heavy")
    assert est.transform_path_["h_chain"] == chained
    # nothing of the fit has moved
    for a in FITTED:
        assert np.array(getattr(est, a)).tobytes() == before[a].tobytes(), a
    assert est._engine is engine_before


def test_default_is_the_general_path(SmoothNMF, monkeypatch):
    monkeypatch.delenv("ESPM_H_CHAIN", raising=False)
    est_kw, X_fit, fit_grid, X_new, new_grid, regs = build_case("ell_k3_simplex_lap")
    est = _fitted(SmoothNMF, est_kw, X_fit, fit_grid)
    Hn = quiet(est.unmix, X_new)
    ref = oracle_transform(est, X_new, new_grid, None, regs, *PARAMS["ell_k3_simplex_lap"][:1], "log_surrogate", PARAMS["ell_k3_simplex_lap"][1])
    assert est.transform_path_["h_chain"] == 0 and est.transform_n_iter_ == ref["n_iter"]
    np.testing.assert_allclose(est.transform_losses_, ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(Hn, ref["H"], rtol=0, atol=H_ATOL)


def test_transform_no_stop_criterion_is_one_batch(SmoothNMF, monkeypatch):
    monkeypatch.setenv("ESPM_H_CHAIN", "1")
    est_kw, X_fit, fit_grid, X_new, new_grid, regs = build_case("ell_k3_simplex_lap")
    est_kw = dict(est_kw, no_stop_criterion=True)
    est = _fitted(SmoothNMF, est_kw, X_fit, fit_grid)
    est.set_params(max_iter=15)
    Hn = quiet(est.unmix, X_new)
    Wf = np.asarray(est.W_, dtype=np.float64)
    ref = oc.fit(X_new, 3, W=Wf.copy(), fixed_W=Wf.copy(), lambda_L=1.0, simplex_H=True, simplex_W=False, shape_2d=new_grid, max_iter=15,
                 no_stop_criterion=True, tol=est.tol)
    assert est.transform_n_iter_ == 15 and est.transform_path_["h_chain"] == 1
    np.testing.assert_allclose(est.transform_losses_, ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(Hn, ref["H"], rtol=0, atol=H_ATOL)


def test_transform_argument_errors(SmoothNMF):
    from sklearn.exceptions import NotFittedError
    est_kw, X_fit, fit_grid, X_new, new_grid, regs = build_case("ell_k3_simplex_lap")
    with pytest.raises(NotFittedError):
        SmoothNMF(shape_2d=fit_grid, **est_kw).unmix(X_new)
    est = _fitted(SmoothNMF, est_kw, X_fit, fit_grid)
    with pytest.raises(ValueError):
        est.unmix(X_new[:-1])                   # another channel count
    with pytest.raises(ValueError):
        est.unmix(-X_new)                       # negative values
    with pytest.raises(ValueError):
        est.unmix(X_new[:, :100])               # lambda_L != 0 and no grid for 100 pixels
    with pytest.raises(ValueError):
        est.unmix(X_new, shape_2d=(7, 9))


def test_transform_is_the_pixel_rows_method(SmoothNMF):
    """``transform`` exists where scikit-learn's meaning of it is the H-only fit (rows = pixels, hspy_comp) and gives what ``unmix`` gives
    there; with rows = channels it is not an attribute (scikit-learn's transformer checks then see the estimator they saw before)."""
    est_kw, X_fit, fit_grid, X_new, new_grid, regs = build_case("hspy_u8_k5")
    est = _fitted(SmoothNMF, est_kw, X_fit, fit_grid)
    a, b = quiet(est.transform, X_new.T), quiet(est.unmix, X_new.T)
    assert a.shape == (X_new.shape[1], 5) and a.tobytes() == b.tobytes()
    est_kw, X_fit, fit_grid, X_new, new_grid, regs = build_case("ell_k3_simplex_lap")
    est = _fitted(SmoothNMF, est_kw, X_fit, fit_grid)
    assert not hasattr(est, "transform") and hasattr(est, "unmix") and hasattr(est, "fit_transform")
    with pytest.raises(AttributeError):
        est.transform(X_new)


# ---- an X above the device-preparation threshold: ONE upload, the sign check and the empty lines from its scans ---------------------
BIG = (600, 90, 80, 3)      # 4.32 M entries, just above estimators/ingest.py's 4 M (the size test_gpu_estimator.py's large fit uses)
BIG_REGS = dict(simplex_H=True, simplex_W=False, lambda_L=1.0)
_big_cache = {}


def _big_draws(holes):
    """(X of the fit, X_new), both (n, p) fp32 counts; ``holes``: the same empty channels and pixels in both."""
    if ("draws", holes) not in _big_cache:
        from espm_amd import synth
        n, nx, ny, k = BIG
        prob = synth.make_problem(n, nx, ny, k, N=40.0, seed=5)
        draws = []
        for seed in (5, 6):
            X = synth.sample_numpy(prob, seed=seed).astype(np.float32)
            X[0, X.sum(axis=0) == 0] = 1.0                     # (no accidental holes: the parameter decides)
            X[X.sum(axis=1) == 0, 0] = 1.0
            if holes:
                X[:5] = 0
                X[300:303] = 0
                X[:, 1000:1040] = 0
                X[:, -7:] = 0
            draws.append(X)
        _big_cache["draws", holes] = draws
    return _big_cache["draws", holes]


def _big_fitted(SmoothNMF, layout, holes):
    """The estimator fitted 6 iterations on the first draw (once per layout and holes), set up for a 6-iteration unmix."""
    if ("est", layout, holes) not in _big_cache:
        from espm_amd import synth
        n, nx, ny, k = BIG
        X_fit = _big_draws(holes)[0]
        W0, H0 = synth.random_init(n, k, nx * ny, seed=5, scale=0.07)
        est = SmoothNMF(n_components=k, shape_2d=(nx, ny), max_iter=6, tol=0, no_stop_criterion=True, verbose=0, hspy_comp=(layout == "pm"), **BIG_REGS)
        quiet(est.fit, np.ascontiguousarray(X_fit.T) if layout == "pm" else X_fit, W=W0.copy(), H=H0.copy())
        _big_cache["est", layout, holes] = est
    return _big_cache["est", layout, holes]


@pytest.mark.parametrize("layout,holes,supplied", [("cm", False, True), ("cm", True, True), ("pm", False, True), ("pm", True, True), ("cm", False, False)],
                         ids=["cm", "cm-holes", "pm", "pm-holes", "cm-H_none"])
def test_unmix_of_a_large_x_on_the_device_and_on_the_host_matches_the_oracle(SmoothNMF, monkeypatch, layout, holes, supplied):
    """unmix of an X above the device-preparation threshold - uploaded once, as it lies (a (pixels, channels) array with hspy_comp: pixel-major),
    sign check, empty lines and the store's facts from the upload's scans, H = None: the pseudo-inverse on the device copy - against the
    oracle, and the same call with the threshold above the array's size (the host passes): the same store, the same tolerances."""
    from espm_amd.estimators import ingest
    n, nx, ny, k = BIG
    assert n * nx * ny >= ingest._DEVICE_PREP_MIN_SIZE
    est = _big_fitted(SmoothNMF, layout, holes)
    X_new = _big_draws(holes)[1]
    H0 = None
    if supplied:
        H0 = np.random.default_rng(99).random((k, nx * ny)) + 0.2
        H0 /= H0.sum(axis=0, keepdims=True)
    ref = oracle_transform(est, X_new, (nx, ny), H0, BIG_REGS, 0, "log_surrogate", 6, no_stop_criterion=True)
    assert ref["n_iter"] == 6
    arg_X = np.ascontiguousarray(X_new.T) if layout == "pm" else X_new
    arg_H = None if H0 is None else (H0.T if layout == "pm" else H0)
    stores = {}
    for path in ("device", "host"):
        if path == "host":
            monkeypatch.setattr(ingest, "_DEVICE_PREP_MIN_SIZE", X_new.size + 1)
        uploads = []
        upload = ingest._upload_with_scans
        monkeypatch.setattr(ingest, "_upload_with_scans", lambda *a, **kw: uploads.append(1) or upload(*a, **kw))
        Hn = quiet(est.unmix, arg_X, H=arg_H)
        monkeypatch.setattr(ingest, "_upload_with_scans", upload)
        assert len(uploads) == (1 if path == "device" else 0)          # (the path that was meant)
        if layout == "pm":
            assert Hn.shape == (nx * ny, k)
            Hn = Hn.T
        stores[path] = est.transform_path_["x_store"]
        print(f"{layout} holes={holes} H supplied={supplied}, {path} path: n_iter {est.transform_n_iter_}, store {stores[path]}, max|dH| {np.abs(Hn - ref['H']).max():.2e}, "
              f"max rel loss {np.abs(np.array(est.transform_losses_) / ref['losses'] - 1).max():.2e}")
        assert est.transform_n_iter_ == 6
        np.testing.assert_allclose(est.transform_losses_, ref["losses"], rtol=LOSS_RTOL)
        np.testing.assert_allclose(Hn, ref["H"], rtol=0, atol=H_ATOL)
    assert stores["device"] == stores["host"]


def test_unmix_of_a_large_x_refuses_nan_and_negative_values(SmoothNMF):
    est = _big_fitted(SmoothNMF, "cm", False)
    bad = _big_draws(False)[1].copy()
    bad[3, 17] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        quiet(est.unmix, bad)
    bad[3, 17] = -1.0
    with pytest.raises(ValueError, match="Negative values in data"):
        quiet(est.unmix, bad)


# ---- 3: the three ways through the H-only iteration give the same bits ----------------------------------------------------------
_CHILD = r"""
import sys, json, hashlib
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from espm_amd.engine import MUEngine
store, k, lam, mode, n_it = sys.argv[2], int(sys.argv[3]), float(sys.argv[4]), sys.argv[5], int(sys.argv[6])
rng = np.random.default_rng(7)
n, nx, ny = 64, 40, 36
tile_px = None
if len(sys.argv) > 7:   # another geometry: tile_px, n, nx, ny (tests/test_gpu_dense_geometry.py)
    tile_px, n, nx, ny = (int(v) for v in sys.argv[7:11])
W = rng.random((n, k)) + 0.05
H = rng.random((k, nx * ny)) + 0.05
H /= H.sum(axis=0, keepdims=True)
X = rng.poisson((0.3 if store == "ell" else 6.0) * n * (W / W.sum(axis=0)) @ H).astype(np.float64)
if store == "u8":
    X = np.minimum(X, 255.0)
if store == "f32":
    X = X * (0.5 + rng.random(X.shape))
eng = MUEngine(X, k, shape_2d=(nx, ny), lambda_L=lam, mu=0.1, simplex_H=True, simplex_W=False, tol=1e-4, max_iter=n_it + 2, device="cuda:0",
               tile_px=tile_px)
assert eng.x_store == store, eng.x_store
H0 = np.full((k, nx * ny), 1.0 / k)
eng.load_state(W, H0)
torch.cuda.synchronize()
held = [t.clone() for t in (eng.w[0], eng.gw_s, eng.colsum_gw)]
chain = eng.h_chain_applies()
if mode == "granular":
    for _ in range(n_it):
        eng.advance_h_only()
    eng.eval_current(advance_h=False)
else:
    eng.iterate_h(n_it, final_loss=True)
torch.cuda.synchronize()
same = all(bool((a == b).all()) for a, b in zip(held, (eng.w[eng.st.cur], eng.gw_s, eng.colsum_gw)))
hist = eng.hist[:n_it + 1].cpu().numpy()
print(json.dumps(dict(chain=int(chain), held=same, it=int(eng.st.it), tile_px=int(eng.st.tile_px), store=eng.x_store, h=hashlib.sha256(eng.get_H().tobytes()).hexdigest(),
                      hist=hashlib.sha256(hist.tobytes()).hexdigest(), hstat=hashlib.sha256(eng.hstat[eng.st.cur].cpu().numpy().tobytes()).hexdigest(),
                      loss_last=float(eng.history()["loss"][-1]))))
"""


def _child(store, k, lam, mode, n_it=9, geometry=None):
    """geometry: (tile_px, n, nx, ny) instead of the image's own tile and 64 channels on 40 x 36 pixels."""
    env = dict(os.environ)
    env["ESPM_H_CHAIN"] = "0" if mode == "general" else "1"   # (granular: sequenced by the host, the buffer is not used)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, store, str(k), str(lam), mode, str(n_it)] + [str(v) for v in geometry or ()], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("lam", [0.0, 1.0], ids=["no_lap", "lap"])
@pytest.mark.parametrize("k", [5, 12])
@pytest.mark.parametrize("store", ["ell", "u8"])
def test_chained_general_and_granular_agree_bit_for_bit(store, k, lam):
    chained, general, granular = (_child(store, k, lam, mode) for mode in ("chained", "general", "granular"))
    assert chained["chain"] == 1 and general["chain"] == 0
    for r in (chained, general, granular):
        assert r["held"] and r["it"] == 9          # W, gw_s, colsum_gw bit-unchanged
    for key in ("h", "hist", "hstat"):
        assert chained[key] == general[key] == granular[key], key


# ---- 5: the refusals come before anything is uploaded ----------------------------------------------------------------------------
def test_transform_refusals(SmoothNMF, monkeypatch):
    est_kw, X_fit, fit_grid, X_new, new_grid, regs = build_case("ell_k3_simplex_lap")
    est = _fitted(SmoothNMF, est_kw, X_fit, fit_grid)
    from espm_amd import engine as engine_mod

    def no_engine(*a, **k):
        raise AssertionError("an engine was built")
    monkeypatch.setattr(engine_mod.MUEngine, "__init__", no_engine)

    def refused(match, **attrs):
        old = {a: getattr(est, a, None) for a in attrs}
        for a, v in attrs.items():
            setattr(est, a, v)
        try:
            with pytest.raises(NotImplementedError, match=match):
                est.unmix(X_new)
        finally:
            for a, v in old.items():
                setattr(est, a, v)
    refused("linesearch", linesearch=True)
    refused("projected_gradient", algo="projected_gradient")
    refused("l2=True", l2=True, algo="l2_surrogate")
    refused("shard", _shard_group=object())
    refused("fp64 mode", _precision="fp64")
