"""GPU: the fp64 mode (MUEngine(precision="fp64"), SmoothNMF.set_precision("fp64")) against the numpy oracle in fp64 with the
reference's bisection (not exact_root).

Tolerances: one H or W step 1e-11 relative per entry (the oracle's products go through BLAS in another order of summation:
the difference is a few ulp, amplified at most by the bisection's last steps); whole fits: n_iter_ equal, losses 1e-9 relative,
W_ and H_ 1e-8 relative to their scale.
"""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import mu_oracle as oc  # noqa: E402

STEP_RTOL = 1e-11


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def make_x(rng, n, p, store, rate=30.0):
    lam = rng.random((n, p)) * rate + 1.0
    if store == "u8":
        return rng.poisson(lam).astype(np.float64)
    if store == "bf16":   # quarters below 64: at most 8 significant bits
        return np.minimum(rng.poisson(lam), 63).astype(np.float64) * 0.25
    return rng.poisson(lam) + rng.random((n, p))   # (not exact in fp32)


def rel_err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


STEP_CASES = [
    # k, store, simplex ("H" / "W" / None), mu ("s" scalar / "v" per component), lambda_L, grid, G columns (None: identity), layout, n, (nx, ny)
    (1, "u8", None, "s", 0.0, True, None, "cm", 333, (7, 19)),
    (3, "u8", "H", "s", 1.3, True, None, "cm", 333, (7, 19)),
    (3, "bf16", "H", "v", 1.3, False, 60, "pm", 333, (7, 19)),
    (5, "f64", "W", "v", 0.0, True, 60, "cm", 333, (7, 19)),
    (5, "u8", "W", "s", 1.3, True, None, "pm", 2050, (9, 12)),
    (8, "f64", "H", "v", 1.3, True, 60, "cm", 2050, (9, 12)),
    (8, "bf16", None, "s", 1.3, False, None, "cm", 333, (7, 19)),
    (8, "u8", "W", "v", 1.3, True, 60, "cm", 333, (7, 19)),
]


@pytest.mark.parametrize("case", STEP_CASES, ids=[f"k{c[0]}-{c[1]}-{c[2]}-mu{c[3]}-lam{c[4]}-{'grid' if c[5] else 'id'}-G{c[6]}-{c[7]}-n{c[8]}"
                                                   for c in STEP_CASES])
def test_one_h_and_one_w_step(case):
    from espm_amd.engine import MUEngine
    k, store, simplex, mu_kind, lam, grid, m, layout, n, (nx, ny) = case
    rng = np.random.default_rng(k * 1000 + n)
    p = nx * ny
    X = make_x(rng, n, p, store)
    G = None if m is None else rng.random((n, m)) + 0.05
    W = rng.random((n if m is None else m, k)) + 0.1
    H = rng.dirichlet(np.ones(k), p).T if simplex == "H" else rng.random((k, p)) + 0.05
    if simplex == "W":
        W = W / W.sum(axis=0, keepdims=True)
    mu = 0.05 if mu_kind == "s" else np.linspace(0.01, 0.08, k)
    L = oc.laplacian_matrix(nx, ny) if grid else oc.identity_L(p)
    eng = MUEngine(X if layout == "cm" else np.ascontiguousarray(X.T), k, layout=layout, G=G, shape_2d=(nx, ny) if grid else None,
                   lambda_L=lam, mu=mu, epsilon_reg=0.5, simplex_H=simplex == "H", simplex_W=simplex == "W", tol=1e-8,
                   max_iter=4, precision="fp64")
    assert eng.x_store == store
    eng.load_state(W, H)
    Gd = np.eye(n) if G is None else G
    h_ref = oc.multiplicative_step_h(X, Gd, W, H, simplex_H=simplex == "H", mu=mu, epsilon_reg=0.5, lambda_L=lam, L=L)
    w_ref = oc.multiplicative_step_w(X, Gd, W, H, simplex_W=simplex == "W")
    h = eng.step_h_only()
    w = eng.step_w_only()
    eh, ew = rel_err(h, h_ref), rel_err(w, w_ref)
    print(f"fp64 step {case}: H {eh:.2e}, W {ew:.2e}")
    assert eh < STEP_RTOL and ew < STEP_RTOL


@pytest.mark.parametrize("dtol", [1e-15, -1.0])
def test_bisection_late_stop_and_maxit(dtol):
    """dicotomy_tol = 1e-15: the global stop comes late (52 sweeps here); -1: no sweep satisfies it and the bisection stops at
    maxit = 100, like the reference's."""
    from espm_amd.engine import MUEngine
    rng = np.random.default_rng(5)
    n, nx, ny, k = 120, 10, 13, 4
    X = make_x(rng, n, nx * ny, "u8")
    W = rng.random((n, k)) + 0.1
    H = rng.dirichlet(np.ones(k), nx * ny).T
    L = oc.laplacian_matrix(nx, ny)
    eng = MUEngine(X, k, shape_2d=(nx, ny), lambda_L=1.0, simplex_H=True, dicotomy_tol=dtol, precision="fp64")
    eng.load_state(W, H)
    h = eng.step_h_only()
    ref = oc.multiplicative_step_h(X, np.eye(n), W, H, simplex_H=True, lambda_L=1.0, L=L, dicotomy_tol=dtol)
    # the sweeps the oracle made (its update's numerators and denominators, updates.py:127-141)
    t = 8 * H.max(axis=1, keepdims=True)
    num = H * (W.T @ (X / (W @ H)) + t)
    den = W.sum(axis=0)[:, None] + t + H @ L
    sweeps = oc.dichotomy_simplex(num, den, tol=dtol, return_sweeps=True)[1]
    assert sweeps == (oc.MAXIT_DICHOTOMY if dtol < 0 else 52)
    err = rel_err(h, ref)
    print(f"fp64 bisection, dicotomy_tol {dtol}: {sweeps} sweeps, H {err:.2e}")
    assert err < STEP_RTOL


# ---- whole fits -----------------------------------------------------------------------------------------------------------------
def issue_problem():
    rng = np.random.default_rng(0)
    n, nx, ny, k = 200, 24, 24, 3
    p = nx * ny
    D = rng.random((n, k))
    H = rng.dirichlet(np.ones(k), p).T
    X = rng.poisson(40 * D @ H).astype(np.float64)
    W0 = rng.random((n, k)) + 0.1
    H0 = rng.dirichlet(np.ones(k), p).T
    return X, W0, H0, (nx, ny), k


def compare_fit(est, Y, ref, n_iter=None):
    assert est.n_iter_ == ref["n_iter"], (est.n_iter_, ref["n_iter"])
    if n_iter is not None:
        assert est.n_iter_ == n_iter
    losses = np.asarray(est.losses_)
    el = float(np.max(np.abs(losses - ref["losses"]) / np.abs(ref["losses"])))
    ew = float(np.max(np.abs(est.W_ - ref["W"])) / np.max(np.abs(ref["W"])))
    eh = float(np.max(np.abs(est.H_ - ref["H"])) / np.max(np.abs(ref["H"])))
    print(f"fp64 fit: {est.n_iter_} iterations, losses {el:.2e}, W {ew:.2e}, H {eh:.2e}")
    assert el < 1e-9 and ew < 1e-8 and eh < 1e-8
    assert est.W_.dtype == np.float64 and est.H_.dtype == np.float64 and Y.dtype == np.float64


def test_fit_follows_the_reference_at_tol_1e8():
    """The issue's problem: fp64 + the reference's bisection stops at 540 iterations, fp32 at 207."""
    from espm_amd.estimators import SmoothNMF
    X, W0, H0, shape, k = issue_problem()
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), lambda_L=1.0, mu=0.0, shape_2d=shape, simplex_H=True, simplex_W=False,
                 tol=1e-8, max_iter=20000)
    est = SmoothNMF(n_components=k, lambda_L=1.0, mu=0.0, shape_2d=shape, simplex_H=True, simplex_W=False, tol=1e-8,
                    max_iter=20000, verbose=0).set_precision("fp64")
    Y = quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
    compare_fit(est, Y, ref, n_iter=540)


def test_fit_paper_like_dictionary_simplex_w_normalize():
    from espm_amd.estimators import SmoothNMF
    rng = np.random.default_rng(7)
    n, nx, ny, k, m = 160, 12, 14, 4, 30
    p = nx * ny
    G = rng.random((n, m)) + 0.02
    Wt = rng.dirichlet(np.ones(m), k).T
    Ht = rng.dirichlet(np.ones(k), p).T
    X = rng.poisson(200 * G @ Wt @ Ht).astype(np.float64)
    W0 = rng.dirichlet(np.ones(m), k).T
    H0 = rng.random((k, p)) + 0.1
    kw = dict(lambda_L=1.0, mu=0.004, epsilon_reg=0.01, shape_2d=(nx, ny), simplex_H=False, simplex_W=True, tol=1e-8, max_iter=300,
              normalize=True)
    ref = oc.fit(X, k, G=G, W=W0.copy(), H=H0.copy(), **kw)
    est = SmoothNMF(n_components=k, G=G, verbose=0, **kw).set_precision("fp64")
    Y = quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
    compare_fit(est, Y, ref)


def test_fit_physics_model_refreshes_g():
    from espm_amd.estimators import SmoothNMF
    from physics_double import AbsorbingModel
    rng = np.random.default_rng(11)
    n, nx, ny, k, m = 140, 10, 12, 3, 24
    p = nx * ny
    G0 = rng.random((n, m)) + 0.05
    Abs = rng.random((n, 6)) * 0.3
    X = rng.poisson(150 * G0 @ rng.dirichlet(np.ones(m), k).T @ rng.dirichlet(np.ones(k), p).T).astype(np.float64)
    W0 = rng.dirichlet(np.ones(m), k).T
    H0 = rng.random((k, p)) + 0.1
    kw = dict(lambda_L=0.5, mu=0.01, shape_2d=(nx, ny), simplex_H=False, simplex_W=True, tol=1e-8, max_iter=60)
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), physics_model=AbsorbingModel(G0, Abs, 0.8, 6), **kw)
    est = SmoothNMF(n_components=k, G=AbsorbingModel(G0, Abs, 0.8, 6), verbose=0, **kw).set_precision("fp64")
    Y = quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
    compare_fit(est, Y, ref)


@pytest.mark.parametrize("which", ["fixed_W", "fixed_H"])
def test_fit_fixed_entries(which):
    from espm_amd.estimators import SmoothNMF
    X, W0, H0, shape, k = issue_problem()
    fixed = -np.ones_like(W0 if which == "fixed_W" else H0)
    if which == "fixed_W":
        fixed[:20, 0] = W0[:20, 0]
    else:
        fixed[1, ::7] = 0.25
    kw = dict(lambda_L=1.0, mu=0.02, shape_2d=shape, simplex_H=which == "fixed_W", simplex_W=False, tol=1e-8, max_iter=150,
              **{which: fixed})
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), safe=True, **kw)
    est = SmoothNMF(n_components=k, verbose=0, **kw).set_precision("fp64")
    Y = quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
    compare_fit(est, Y, ref)


def test_fit_empty_channel_and_pixel_hspy_comp():
    """An all-zero channel and pixel (the log_shift fill: the fp64 store) and hyperspy's (pixels, channels) layout.  simplex_W:
    with simplex_H the reference's own bisection divides by zero at the empty pixel (its root sits at nu = -den, dicotomy.py:51-53)."""
    from espm_amd.estimators import SmoothNMF
    X, W0, H0, shape, k = issue_problem()
    X = X.copy()
    X[17, :] = 0
    X[:, 40] = 0
    W0 = W0 / W0.sum(axis=0, keepdims=True)
    kw = dict(lambda_L=1.0, mu=0.01, shape_2d=shape, simplex_H=False, simplex_W=True, tol=1e-8, max_iter=200)
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), **kw)
    est = SmoothNMF(n_components=k, verbose=0, hspy_comp=True, **kw).set_precision("fp64")
    Ht = quiet(est.fit_transform, np.ascontiguousarray(X.T), W=W0.copy(), H=H0.copy())
    assert est._engine.x_store == "f64"
    compare_fit(est, Ht, ref)


def test_fits_are_bit_identical():
    from espm_amd.estimators import SmoothNMF
    X, W0, H0, shape, k = issue_problem()
    outs = []
    for _ in range(2):
        est = SmoothNMF(n_components=k, lambda_L=1.0, shape_2d=shape, simplex_H=True, simplex_W=False, tol=1e-8, max_iter=60,
                        verbose=0).set_precision("fp64")
        quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
        outs.append((est.W_.copy(), est.H_.copy(), np.asarray(est.losses_)))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_mid_size_three_iterations():
    """2048 channels x 128^2 pixels: full H-pass blocks, the channel staging in one 2048-channel chunk, many W-pass chunks."""
    from espm_amd.engine import MUEngine
    rng = np.random.default_rng(3)
    n, nx, ny, k = 2048, 128, 128, 5
    p = nx * ny
    X = rng.poisson(rng.random((n, k)) @ rng.dirichlet(np.ones(k), p).T * 6).astype(np.float64)
    X[:, 0] += 1.0   # (no empty channel)
    W0 = rng.random((n, k)) + 0.1
    H0 = rng.dirichlet(np.ones(k), p).T
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), lambda_L=1.0, shape_2d=(nx, ny), simplex_H=True, simplex_W=False, tol=0,
                 no_stop_criterion=True, max_iter=3)
    eng = MUEngine(X, k, shape_2d=(nx, ny), lambda_L=1.0, simplex_H=True, simplex_W=False, tol=0.0, max_iter=3, precision="fp64")
    eng.load_state(W0, H0)
    eng.iterate(3, final_loss=True)
    hist = eng.history()
    el = float(np.max(np.abs(hist["loss"][1:] - ref["losses"]) / np.abs(ref["losses"])))
    ew, eh = rel_err(eng.get_W(), ref["W"]), float(np.max(np.abs(eng.get_H() - ref["H"])) / np.max(ref["H"]))
    print(f"fp64 mid-size: losses {el:.2e}, W {ew:.2e}, H {eh:.2e}")
    assert el < 1e-11 and ew < 1e-9 and eh < 1e-9
