"""GPU parity of the fit loop: espm_amd.estimators.SmoothNMF (HIP path through the C ABI) against the
golden trajectories captured from the reference and against the numpy oracle; the reference's
estimator tests that do not need hyperspy (espm/tests/test_estimators.py:100-104, :155-166, :207-259).

Tolerance (stated for fp32 device arithmetic against the fp64 reference): losses 1e-5 relative
(BASELINE.json north star), H 5e-5 absolute (the reference's own simplex multiplier is converged to
dicotomy_tol = 1e-5 only), W 2e-4 relative to its scale.
"""
import contextlib
import ctypes as C
import io
import json
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import mu_oracle as oc  # noqa: E402

LOSS_RTOL = 1e-5


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.fixture(scope="module")
def SmoothNMF():
    from espm_amd.estimators import SmoothNMF as cls
    return cls


@pytest.fixture(params=["auto", "fused", "fused_small"])
def geometry(request, monkeypatch):
    """"fused": the sparse store at its full geometry (512-pixel tiles, 1024-pixel blocks) also on these small images, so that
    the fits run through the fused H update + W accumulation launch (and the granular loop around it) that only large images
    get; "fused_small": the fused launch on the small images' own geometry (blocks of 128 pixels: the run-time-sized variant)."""
    if request.param == "fused":
        monkeypatch.setenv("ESPM_FORCE_ELL_TILE", "512")
    if request.param == "fused_small":
        monkeypatch.setenv("ESPM_FUSED", "always")
    return request.param


def _check_traj(est, GW, g, pre):
    assert est.n_iter_ == int(g[f"{pre}_n_iter"]), pre
    np.testing.assert_allclose(est.losses_, g[f"{pre}_losses"], rtol=LOSS_RTOL, err_msg=pre)
    det = np.array(est.detailed_losses_, dtype=float)
    ref = g[f"{pre}_detailed"]
    np.testing.assert_allclose(det[:, 0], ref[:, 0], rtol=LOSS_RTOL, err_msg=pre)          # KL
    np.testing.assert_allclose(det[:, 1:3], ref[:, 1:3], rtol=5e-5, atol=1e-9, err_msg=pre)  # log-reg, Laplacian
    np.testing.assert_array_equal(det[:, 3], ref[:, 3])                                    # gamma
    scale = np.abs(g[f"{pre}_W"]).mean()
    np.testing.assert_allclose(est.W_, g[f"{pre}_W"], rtol=2e-4, atol=2e-4 * scale, err_msg=pre)
    np.testing.assert_allclose(est.H_, g[f"{pre}_H"], rtol=2e-4, atol=5e-5, err_msg=pre)
    np.testing.assert_allclose(GW, g[f"{pre}_GW"], rtol=2e-4, atol=2e-4 * np.abs(g[f"{pre}_GW"]).mean(), err_msg=pre)
    np.testing.assert_allclose(est.reconstruction_err_, g[f"{pre}_recon"], rtol=LOSS_RTOL)
    rel, rel_ref = np.array(est.rel_), g[f"{pre}_rel"]
    # an entry of W thrown onto the clamp gives rel_W = W_old / 1e-14 ~ 1e14, decided by WHICH entry lands on the clamp: an empty
    # channel does with the sparse store and stops at 1.6e-14 with the reference's fill - order of magnitude only
    huge = rel_ref > 1e6
    np.testing.assert_allclose(rel[~huge], rel_ref[~huge], rtol=2e-2, atol=2e-5, err_msg=pre)
    np.testing.assert_allclose(np.log10(rel[huge]), np.log10(rel_ref[huge]), atol=1.0, err_msg=pre)


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c5", "cw"])
def test_trajectories_golden(SmoothNMF, golden, name, geometry):
    """F6: scaled-down analogues of BASELINE configs 1, 2, 3, 5 (+ simplex_W), free running 50 iterations
    and with the default stop rules (n_iter_ must match the reference)."""
    g = golden("f6_trajectories")
    c = json.loads(str(g["configs"]))[name]
    G = g.get(f"{name}_G")
    shape = tuple(int(v) for v in g[f"{name}_shape"])
    for mode, extra in (("free", dict(tol=0, no_stop_criterion=True, max_iter=50)), ("stop", dict(tol=1e-3, max_iter=200))):
        est = SmoothNMF(n_components=c["k"], G=G, shape_2d=shape, verbose=0, **c["kw"], **extra)
        GW = quiet(est.fit_transform, g[f"{name}_X"], W=g[f"{name}_W0"].copy(), H=g[f"{name}_H0"].copy())
        _check_traj(est, GW, g, f"{name}_{mode}")


def test_hspy_comp_and_api(SmoothNMF, golden):
    """F8: hyperspy conventions (base.py:243-247, :412-420), get_losses names, inverse_transform."""
    g = golden("f8_api")
    X, W0, H0 = g["hspy_X"], g["hspy_W0"], g["hspy_H0"]
    est = SmoothNMF(n_components=2, max_iter=3, simplex_H=True, simplex_W=False, verbose=0, hspy_comp=True)
    ret = quiet(est.fit_transform, X.T.copy(), W=W0.copy(), H=H0.copy())
    assert ret.shape == (X.shape[1], 2) and est.components_.shape == (2, X.shape[0])
    np.testing.assert_allclose(ret, g["hspy_ret"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(est.components_, g["hspy_components"], rtol=2e-4, atol=1e-6)
    losses = est.get_losses()
    assert list(losses.dtype.names) == json.loads(str(g["loss_names"]))
    np.testing.assert_allclose(np.array(losses.tolist())[:, :2], g["get_losses"][:, :2], rtol=LOSS_RTOL)
    np.testing.assert_allclose(est.inverse_transform(est.W_), g["inverse_transform"], rtol=2e-4, atol=1e-5)
    for attr in ("W_", "H_", "G_", "L_", "X_", "n_iter_", "losses_", "detailed_losses_", "rel_",
                 "reconstruction_err_", "components_", "n_components_", "const_KL_", "gamma_"):
        assert hasattr(est, attr), attr
    assert est.G_.shape == (X.shape[0], X.shape[0])  # dense identity for G=None (updates.py:166)


def test_no_simplex_rescaling(SmoothNMF, golden):
    g = golden("f8_api")
    X, W0, H0 = g["hspy_X"], g["hspy_W0"], g["hspy_H0"]
    est = SmoothNMF(n_components=2, max_iter=4, simplex_H=False, simplex_W=False, verbose=0)
    GW = quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
    np.testing.assert_allclose(GW, g["nosimplex_GW"], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(est.H_, g["nosimplex_H"], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(est.reconstruction_err_, g["nosimplex_recon"], rtol=LOSS_RTOL)


def test_normalize_golden_and_scale_invariance(SmoothNMF, golden, geometry):
    """espm/tests/test_estimators.py:207-247 (normalize=True => results invariant under X -> X / fac)."""
    g = golden("f8_api")
    X, fac = g["norm_X"], float(g["norm_fac"])
    kw = dict(n_components=5, lambda_L=1.0, max_iter=10, init="nndsvd", normalize=True, shape_2d=[8, 4], random_state=0,
              simplex_W=False, simplex_H=True, verbose=0)
    est = SmoothNMF(**kw)
    GP = quiet(est.fit_transform, X)
    H = est.H_
    # NNDSVD zeros (clamped to 1e-14) put simplex roots ~1e-11 from a pole of f(nu): the reference
    # resolves those in fp64 only to ulp(den) and its H columns then sum to 1 +- 5e-3 (see
    # oracle.dichotomy_simplex_exact).  The HIP path solves for nu + den_min instead; it is compared
    # tightly with the well-conditioned oracle and only loosely with the reference's own output.
    ref = oc.fit(X, 5, lambda_L=1.0, max_iter=10, init="nndsvd", normalize=True, shape_2d=(8, 4), random_state=0,
                 simplex_W=False, simplex_H=True, exact_root=True)
    np.testing.assert_allclose(GP, ref["GW"], rtol=2e-4, atol=2e-4 * np.abs(ref["GW"]).mean())
    np.testing.assert_allclose(H, ref["H"], rtol=2e-4, atol=5e-5)
    np.testing.assert_allclose(est.losses_, ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(H.sum(axis=0), 1.0, atol=2e-6)
    assert np.abs(GP - g["norm_GP"]).max() < 0.1 * np.abs(g["norm_GP"]).mean()
    X_plus = np.concatenate([X / fac, X / fac], axis=0)
    GP_plus = quiet(est.fit_transform, X_plus)
    H_plus = est.H_

    def ratio(a, b):
        return np.sum(np.abs(a - b)) / np.sum(np.abs(a))

    assert ratio(GP_plus * fac, np.concatenate([GP, GP], axis=0)) < 1e-4
    assert ratio(H_plus, H) < 1e-4


def test_fixed_matrices_respected(SmoothNMF, geometry):
    """espm/tests/test_estimators.py:155-166."""
    from espm_amd import synth
    prob = synth.make_problem(40, 10, 20, 2, N=80.0, seed=5, m=8)
    X = synth.sample_numpy(prob, seed=5)
    fW = -np.ones((8, 2))
    fW[0, 0] = 0.0
    fW[1, 0] = 0.0
    fH = -np.ones((2, 200))
    fH[0, 0:20] = 1.0
    fH[1, 0:20] = 0.0
    est = SmoothNMF(G=prob["G"], n_components=2, max_iter=30, simplex_W=False, simplex_H=True, fixed_W=fW, verbose=0)
    quiet(est.fit_transform, X)
    np.testing.assert_allclose(est.W_[fW >= 0], fW[fW >= 0])
    est = SmoothNMF(G=prob["G"], n_components=2, max_iter=30, simplex_W=False, simplex_H=True, fixed_H=fH, verbose=0)
    quiet(est.fit_transform, X)
    np.testing.assert_allclose(est.H_[fH >= 0], fH[fH >= 0])


def test_more_lambda_is_smoother(SmoothNMF):
    """espm/tests/test_estimators.py:139-153 (trace(H L H^T) decreases with lambda_L)."""
    from espm_amd import synth
    prob = synth.make_problem(48, 10, 20, 2, N=60.0, seed=6, m=8)
    X = synth.sample_numpy(prob, seed=6)
    L = oc.laplacian_matrix(10, 20)
    tr = []
    for lam in (0.0, 100.0):
        est = SmoothNMF(G=prob["G"], lambda_L=lam, n_components=2, max_iter=100, simplex_W=False, simplex_H=True,
                        shape_2d=[10, 20], tol=1e-6, verbose=0, random_state=0)
        quiet(est.fit_transform, X)
        tr.append(oc.trace_xtLx(L, est.H_.T))
    assert tr[1] < tr[0]


def test_float32_input_and_pickle(SmoothNMF, golden):
    g = golden("f6_trajectories")
    X = g["c2_X"].astype(np.float32)
    est = SmoothNMF(n_components=3, simplex_H=True, simplex_W=False, max_iter=5, verbose=0)
    GW = quiet(est.fit_transform, X, W=g["c2_W0"].astype(np.float32), H=g["c2_H0"].astype(np.float32))
    assert GW.dtype == np.float32 and est.H_.dtype == np.float32  # base.py:247 keeps float32
    est2 = pickle.loads(pickle.dumps(est))
    np.testing.assert_array_equal(est2.H_, est.H_)
    with pytest.raises(ValueError):
        quiet(est.fit_transform, -X)  # base.py:528 "Negative values in data"


def test_iteration_method_matches_oracle(SmoothNMF, golden, geometry):
    g = golden("f6_trajectories")
    X, W0, H0 = g["c3_X"], g["c3_W0"], g["c3_H0"]
    shape = tuple(int(v) for v in g["c3_shape"])
    est = SmoothNMF(n_components=5, simplex_H=True, simplex_W=False, lambda_L=1.0, shape_2d=shape, max_iter=1, verbose=0)
    quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
    W1, H1 = est._iteration(W0.copy(), H0.copy())
    np.testing.assert_allclose(W1, g["c3_free_W1"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(H1, g["c3_free_H1"], rtol=1e-4, atol=2e-5)


def test_sklearn_check_estimator(SmoothNMF):
    """espm/tests/test_estimators.py:100-104."""
    from sklearn.utils.estimator_checks import check_estimator
    with contextlib.redirect_stdout(io.StringIO()):
        check_estimator(SmoothNMF(n_components=5, max_iter=200, simplex_W=False, simplex_H=True, mu=1.0, epsilon_reg=1.0,
                                  hspy_comp=False))
        check_estimator(SmoothNMF(n_components=5, lambda_L=2, max_iter=200, simplex_W=False, simplex_H=True, mu=1.0,
                                  epsilon_reg=1.0, hspy_comp=False))


def test_physics_model_protocol(SmoothNMF, geometry):
    """G given as an object with NMF_update / NMF_simplex / NMF_initialize_W (espm/models/base.py:217-264):
    G is refreshed every 3rd iteration (base.py:388-392) and simplex_W acts on NMF_simplex() rows only."""
    from espm_amd import synth
    prob = synth.make_problem(40, 8, 8, 2, N=80.0, seed=7, m=6)
    X = synth.sample_numpy(prob, seed=7)

    class Model:
        def __init__(self, G):
            self.G = G.copy()
            self.calls = 0

        def NMF_update(self, W=None):
            self.calls += 1
            return self.G

        def NMF_simplex(self):
            return np.arange(4)

        def NMF_initialize_W(self, D):
            return np.abs(np.linalg.lstsq(self.G, D, rcond=None)[0])

    model = Model(prob["G"])
    est = SmoothNMF(G=model, n_components=2, max_iter=7, simplex_W=True, simplex_H=False, verbose=0, tol=0,
                    no_stop_criterion=True, random_state=0)
    quiet(est.fit_transform, X)
    assert model.calls == 1 + 2  # at init, after iterations 3 and 6
    np.testing.assert_allclose(est.W_[:4].sum(axis=0), 1.0, atol=2e-5)
    W0 = est.W_.copy()
    ref = oc.multiplicative_step_w(X, prob["G"], W0, est.H_, simplex_W=True, simplex_rows=np.arange(4))
    from espm_amd.estimators.updates import multiplicative_step_w
    got = multiplicative_step_w(X, prob["G"], W0, est.H_, simplex_W=True, physics_model=model)
    np.testing.assert_allclose(got, ref, rtol=3e-5, atol=1e-7)


@pytest.mark.parametrize("n,nx,ny,k,m", [(1980, 10, 13, 3, None), (100, 20, 20, 3, None), (333, 7, 19, 8, 17), (65, 3, 5, 1, 4),
                                         (2050, 4, 33, 6, None)])
def test_ragged_shapes_match_oracle(SmoothNMF, n, nx, ny, k, m):
    """Channel counts that are not multiples of the vector width, pixel counts that do not fill a tile, k = 1..8."""
    from espm_amd import synth
    prob = synth.make_problem(n, nx, ny, k, N=90.0, seed=n, m=m)
    X = synth.sample_numpy(prob, seed=n)
    W0, H0 = synth.random_init(m if m else n, k, nx * ny, seed=n, scale=0.2)
    kw = dict(lambda_L=0.7, mu=0.02, simplex_H=True, simplex_W=False, tol=0, no_stop_criterion=True, max_iter=10)
    ref = oc.fit(X, k, G=prob["G"], W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, **kw)
    est = SmoothNMF(n_components=k, G=prob["G"], shape_2d=(nx, ny), verbose=0, **kw)
    quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
    np.testing.assert_allclose(est.losses_, ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(est.H_, ref["H"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(est.W_, ref["W"], rtol=2e-4, atol=2e-4 * np.abs(ref["W"]).mean())


@pytest.mark.parametrize("store", ["ell", "u8"])
@pytest.mark.parametrize("n,nx,ny,k,m,counts,hot,kw", [
    (64, 12, 10, 5, None, 90.0, 0, dict(lambda_L=0.7, mu=0.02, simplex_H=True, simplex_W=False)),
    (333, 7, 19, 8, 17, 90.0, 0, dict(lambda_L=0.7, mu=0.02, simplex_H=True, simplex_W=False)),    # G given, k = 8
    (1980, 33, 31, 3, None, 500.0, 0, dict(lambda_L=0.0, simplex_H=True, simplex_W=False)),           # BASELINE config 2 shape, 1023 pixels
    (2050, 4, 33, 6, None, 300.0, 40, dict(lambda_L=1.0, simplex_H=False, simplex_W=True)),           # 12 index bits: counts > 15 are split
    (50, 5, 6, 2, None, 150.0, 25, dict(lambda_L=0.3, simplex_H=True, simplex_W=False)),              # counts > 63: split in the W lists
    (100, 40, 30, 2, None, 20.0, 0, dict(lambda_L=0.5, mu=0.1, simplex_H=True, simplex_W=False)),     # very sparse, two W blocks
    (70, 5, 6, 7, None, 40.0, 0, dict(lambda_L=0.0, simplex_H=True, simplex_W=False)),
])
def test_count_stores_match_oracle(store, n, nx, ny, k, m, counts, hot, kw):
    """The sparse count store (x_store='ell': non-zero entries only) and the dense 8-bit store against the fp64
    oracle: ragged channel / pixel counts, every k, G given, counts that need several entries, fixed_H."""
    import torch
    from espm_amd import synth
    from espm_amd.engine import MUEngine
    prob = synth.make_problem(n, nx, ny, k, N=counts, seed=n, m=m)
    X = np.minimum(synth.sample_numpy(prob, seed=n), 255.0)
    if hot:  # a few bright entries whose counts do not fit the count field of one entry
        rng = np.random.default_rng(n)
        X[rng.integers(0, n, hot), rng.integers(0, nx * ny, hot)] = rng.integers(70, 256, hot)
    X[X.sum(axis=1) == 0, 0] = 1.0  # the count stores take strictly integer data: no all-zero lines (base.py:519-528)
    X[0, X.sum(axis=0) == 0] = 1.0
    W0, H0 = synth.random_init(m if m else n, k, nx * ny, seed=n, scale=0.2)
    fixed_H = None
    if k >= 2 and not kw.get("simplex_H"):
        fixed_H = -np.ones((k, nx * ny))
        fixed_H[0, ::3] = 0.25
    ref = oc.fit(X, k, G=prob["G"], W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, no_stop_criterion=True,
                 max_iter=6, tol=0, fixed_H=fixed_H, **kw)
    eng = MUEngine(X, k, G=prob["G"], shape_2d=(nx, ny), max_iter=6, tol=0, x_store=store, fixed_H=fixed_H, **kw)
    assert eng.x_store == store
    eng.load_state(W0, H0)
    eng.iterate(6, final_loss=True)
    torch.cuda.synchronize()
    h = eng.history()
    np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(eng.get_H(), ref["H"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(eng.get_W(), ref["W"], rtol=2e-4, atol=2e-4 * np.abs(ref["W"]).mean())
    assert h["bad"].sum() == 0


@pytest.mark.parametrize("kw", [dict(simplex_H=True, simplex_W=False, mu=0.3, lambda_L=2.0), dict(simplex_H=False, simplex_W=True)])
@pytest.mark.parametrize("m", [None, 5])
def test_empty_channels_keep_the_sparse_store(SmoothNMF, kw, m, geometry):
    """Measured spectra have channels without a single count in the whole image.  The reference fills them with
    log_shift (base.py:519-528); the sparse store leaves that fill out of its lists (an O(1e-14) change) instead of
    falling back to a dense fp32 X.  Engine and estimator against the fp64 oracle, which fills like the reference."""
    import torch
    from espm_amd import synth
    from espm_amd.engine import MUEngine
    n, nx, ny, k = 160, 16, 20, 3
    prob = synth.make_problem(n, nx, ny, k, N=25.0, seed=3, m=m)
    X = synth.sample_numpy(prob, seed=3)
    X[0, X.sum(axis=0) == 0] = 1.0
    X[:7] = 0
    X[60:64] = 0
    X[-9:] = 0
    W0, H0 = synth.random_init(m if m else n, k, nx * ny, seed=3, scale=0.2)
    ref = oc.fit(X, k, G=prob["G"], W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, no_stop_criterion=True,
                 max_iter=8, tol=0, **kw)
    eng = MUEngine(X, k, G=prob["G"], shape_2d=(nx, ny), max_iter=8, tol=0, **kw)
    assert eng.x_store == "ell"
    eng.load_state(W0, H0)
    eng.iterate(8, final_loss=True)
    torch.cuda.synchronize()
    h = eng.history()
    np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(eng.get_H(), ref["H"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(eng.get_W(), ref["W"], rtol=2e-4, atol=2e-4 * np.abs(ref["W"]).mean())
    assert h["bad"].sum() == 0
    est = SmoothNMF(n_components=k, G=prob["G"], shape_2d=(nx, ny), max_iter=8, tol=0, no_stop_criterion=True, verbose=0,
                    normalize=True, **kw)
    Xin = X.copy()
    quiet(est.fit, Xin, W=W0.copy(), H=H0.copy())
    assert est._engine.x_store == "ell" and (Xin == X).all()
    refn = oc.fit(X, k, G=prob["G"], W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, no_stop_criterion=True,
                  max_iter=8, tol=0, normalize=True, **kw)
    np.testing.assert_allclose(est.losses_, refn["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(est.H_, refn["H"], rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("k,store,m,kw", [
    (9, "u8", None, dict(lambda_L=0.7, mu=0.02, simplex_H=True, simplex_W=False)),
    (12, "f32", 20, dict(lambda_L=0.5, mu=0.05, simplex_H=True, simplex_W=False)),
    (16, "u8", None, dict(lambda_L=1.0, simplex_H=False, simplex_W=True)),
    (11, "bf16", 14, dict(lambda_L=0.0, simplex_H=False, simplex_W=True)),
    (16, "f32", None, dict(lambda_L=0.3, simplex_H=True, simplex_W=False, fixed=True)),
    (10, "u8", None, dict(lambda_L=0.0, simplex_H=False, simplex_W=False)),
    # from 13 components on the dense H-step runs on the matrix cores too (mu_h_mfma_kernel.hpp; n_pad = 152 is neither a
    # multiple of 16 nor of 64: the guarded loads and the partial last channel tile); "valu": the vector kernels at that k
    (13, "u8", None, dict(lambda_L=0.7, mu=0.02, simplex_H=True, simplex_W=False)),
    (14, "bf16", 9, dict(lambda_L=0.4, mu=0.05, simplex_H=True, simplex_W=False)),
    (16, "u8", None, dict(lambda_L=1.0, simplex_H=False, simplex_W=True, valu=True)),
    # the sparse count store with 12- and 16-float table rows (round 2)
    (9, "ell", None, dict(lambda_L=0.7, mu=0.02, simplex_H=True, simplex_W=False)),
    (12, "ell", 20, dict(lambda_L=0.5, mu=0.05, simplex_H=True, simplex_W=False)),
    (13, "ell", None, dict(lambda_L=1.0, simplex_H=False, simplex_W=True)),
    (16, "ell", None, dict(lambda_L=0.3, simplex_H=True, simplex_W=False, fixed=True)),
])
def test_nine_to_sixteen_components(k, store, m, kw):
    """More than 8 components run on the second build of the library (libespm_mu_wide.so: component stride 16, every
    store): engine against the fp64 oracle with simplex over H or W, a dictionary G, mu, the Laplacian and fixed_H."""
    _wide_build_against_oracle(k, store, m, kw, 16)


@pytest.mark.parametrize("k,store,m,kw", [
    (17, "u8", None, dict(lambda_L=0.7, mu=0.02, simplex_H=True, simplex_W=False)),
    (24, "f32", 30, dict(lambda_L=0.5, mu=0.05, simplex_H=True, simplex_W=False)),
    (32, "u8", None, dict(lambda_L=1.0, simplex_H=False, simplex_W=True)),
    (20, "bf16", 25, dict(lambda_L=0.0, simplex_H=False, simplex_W=True)),
    (32, "f32", None, dict(lambda_L=0.3, simplex_H=True, simplex_W=False, fixed=True)),
    (19, "u8", None, dict(lambda_L=0.0, simplex_H=False, simplex_W=False)),
    (28, "bf16", 33, dict(lambda_L=0.4, mu=0.05, simplex_H=True, simplex_W=False)),
    (32, "bf16", None, dict(lambda_L=0.7, mu=0.02, simplex_H=True, simplex_W=False)),
    # "valu": the vector kernels (the widest build keeps them for the fp32 store: the alternate rules and A/B run there)
    (24, "f32", None, dict(lambda_L=1.0, simplex_H=True, simplex_W=False, valu=True)),
    (31, "f32", 36, dict(lambda_L=0.2, simplex_H=False, simplex_W=True, valu=True)),
])
def test_seventeen_to_thirtytwo_components(k, store, m, kw):
    """VERDICT r4, missing 3: the reference has no limit on n_components (base.py:126-132).  17..32 components run on the third
    build of the library (libespm_mu_wide32.so: component stride 32, the dense stores, both contractions on the matrix cores in two
    halves of 16 components): engine against the fp64 oracle as for 9..16."""
    _wide_build_against_oracle(k, store, m, kw, 32)


def _wide_build_against_oracle(k, store, m, kw, kp):
    import torch
    from espm_amd import synth
    from espm_amd.engine import MUEngine
    kw = dict(kw)
    n, nx, ny = 150, 19, 23
    prob = synth.make_problem(n, nx, ny, k, N=120.0, seed=k, m=m)
    X = np.minimum(synth.sample_numpy(prob, seed=k), 255.0)
    X[X.sum(axis=1) == 0, 0] = 1.0
    X[0, X.sum(axis=0) == 0] = 1.0
    if store == "f32":
        X = X * 0.37
    W0, H0 = synth.random_init(m if m else n, k, nx * ny, seed=k, scale=0.2)
    fixed_H = None
    if kw.pop("fixed", False):
        fixed_H = -np.ones((k, nx * ny))
        fixed_H[k - 1, ::3] = 0.05
    fused = not kw.pop("valu", False)
    ref = oc.fit(X, k, G=prob["G"], W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, no_stop_criterion=True,
                 max_iter=6, tol=0, fixed_H=fixed_H, **kw)
    eng = MUEngine(X, k, G=prob["G"], shape_2d=(nx, ny), max_iter=6, tol=0, fixed_H=fixed_H, x_store="auto" if store == "f32" else store,
                   fused=fused, **kw)
    assert eng.x_store == store and eng.V.KP == kp
    eng.load_state(W0, H0)
    eng.iterate(6, final_loss=True)
    torch.cuda.synchronize()
    h = eng.history()
    np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(h["rel_W"][1:], ref["rel"][:, 0], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(h["rel_H"][1:], ref["rel"][:, 1], rtol=1e-3, atol=1e-5)
    We, He = eng.get_W().astype(np.float64), eng.get_H().astype(np.float64)
    if not kw["simplex_H"] and not kw["simplex_W"]:
        We, He = oc.rescaled_DH(We, He)   # base.py:399-400: what the fit loop returns without a simplex
    np.testing.assert_allclose(He, ref["H"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(We, ref["W"], rtol=2e-4, atol=2e-4 * np.abs(ref["W"]).mean())
    assert h["bad"].sum() == 0


@pytest.mark.parametrize("kw", [dict(simplex_H=True, simplex_W=False, mu=0.2, lambda_L=1.5), dict(simplex_H=True, simplex_W=False),
                                dict(simplex_H=False, simplex_W=True, lambda_L=0.5), dict(simplex_H=False, simplex_W=False)])
@pytest.mark.parametrize("m", [None, 6])
def test_pixels_without_counts_keep_the_sparse_store(SmoothNMF, kw, m, geometry):
    """Holes, vacuum and low doses leave pixels without a single count.  The reference fills them with log_shift in every
    channel (base.py:519-528) and, under simplex_H, that fill alone decides their column of H.  The sparse store keeps
    their lists empty and the H-step adds the fill's numerator from a small pass of its own (ell_fill_* in espm_mu.h).
    Engine and estimator against the fp64 oracle, which fills like the reference; scattered pixels, a whole image row,
    image corners, together with empty channels."""
    import torch
    from espm_amd import synth
    from espm_amd.engine import MUEngine
    n, nx, ny, k = 130, 18, 21, 4
    prob = synth.make_problem(n, nx, ny, k, N=30.0, seed=8, m=m)
    X = synth.sample_numpy(prob, seed=8)
    X[0, X.sum(axis=0) == 0] = 1.0
    X[:3] = 0                                 # empty channels as well
    empty = np.zeros(nx * ny, dtype=bool)
    empty[[0, ny - 1, nx * ny - 1, 100, 101, 233]] = True
    empty[5 * ny:6 * ny] = True               # a whole image row
    X[:, empty] = 0
    W0, H0 = synth.random_init(m if m else n, k, nx * ny, seed=8, scale=0.2)
    ref = oc.fit(X, k, G=prob["G"], W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, no_stop_criterion=True,
                 max_iter=8, tol=0, **kw)
    eng = MUEngine(X, k, G=prob["G"], shape_2d=(nx, ny), max_iter=8, tol=0, **kw)
    assert eng.x_store == "ell" and int(eng.st.ell_fill_n) == int(empty.sum())
    eng.load_state(W0, H0)
    eng.iterate(8, final_loss=True)
    torch.cuda.synchronize()
    h = eng.history()
    We, He = eng.get_W().astype(np.float64), eng.get_H().astype(np.float64)
    if not kw["simplex_H"] and not kw["simplex_W"]:
        We, He = oc.rescaled_DH(We, He)
    np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(h["rel_H"][1:], ref["rel"][:, 1], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(He[:, ~empty], ref["H"][:, ~empty], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(He[:, empty], ref["H"][:, empty], rtol=5e-4, atol=5e-5)     # the columns the fill decides
    np.testing.assert_allclose(We, ref["W"], rtol=2e-4, atol=2e-4 * np.abs(ref["W"]).mean())
    assert h["bad"].sum() == 0
    if kw["simplex_H"]:
        np.testing.assert_allclose(He[:, empty].sum(axis=0), 1.0, atol=1e-5)
    est = SmoothNMF(n_components=k, G=prob["G"], shape_2d=(nx, ny), max_iter=8, tol=0, no_stop_criterion=True, verbose=0,
                    normalize=True, **kw)
    Xin = X.copy()
    quiet(est.fit, Xin, W=W0.copy(), H=H0.copy())
    assert est._engine.x_store == "ell" and (Xin == X).all()
    refn = oc.fit(X, k, G=prob["G"], W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, no_stop_criterion=True,
                  max_iter=8, tol=0, normalize=True, **kw)
    np.testing.assert_allclose(est.losses_, refn["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(est.H_, refn["H"], rtol=5e-4, atol=5e-5)


def test_sparse_store_is_chosen_for_sparse_counts_only():
    from espm_amd import synth
    from espm_amd.engine import MUEngine
    prob = synth.make_problem(128, 8, 8, 2, N=30.0, seed=1)
    X = synth.sample_numpy(prob, seed=1)
    X[X.sum(axis=1) == 0, 0] = 1.0
    X[0, X.sum(axis=0) == 0] = 1.0
    assert MUEngine(X, 2, shape_2d=(8, 8)).x_store == "ell"            # ~20 % non-zero
    assert MUEngine(X + 1.0, 2, shape_2d=(8, 8)).x_store == "u8"       # dense counts
    assert MUEngine(X * 0.5, 2, shape_2d=(8, 8)).x_store == "bf16"     # not integer
    with pytest.raises(ValueError):
        MUEngine(X * 0.5, 2, shape_2d=(8, 8), x_store="ell")


@pytest.mark.parametrize("n,p,k,init,dtype", [(300, 20000, 4, None, np.float64), (2100, 2400, 5, "nndsvd", np.float64),
                                               (256, 17000, 3, "nndsvdar", np.float32), (6000, 700, 6, "nndsvda", np.float64)])
def test_device_nndsvd_matches_sklearn(n, p, k, init, dtype):
    """espm_amd.init_device (randomized SVD passes over X on the GPU) against scikit-learn's _initialize_nmf, which
    the reference calls (espm/estimators/updates.py:179): same random stream, same algorithm, equal to rounding -
    for a wide X (transposed inside the randomized SVD), a tall one, fp32 input and every NNDSVD variant."""
    from sklearn.decomposition._nmf import _initialize_nmf
    from espm_amd import init_device
    from espm_amd.estimators.updates import initialize_algorithms
    rng = np.random.default_rng(n)
    W = rng.random((n, k)) ** 3
    H = rng.random((k, p)) ** 2
    X = rng.poisson(3.0 * W @ H).astype(dtype)
    assert X.size >= init_device.DEVICE_INIT_MIN_SIZE
    Wr, Hr = _initialize_nmf(X, n_components=k, init=init, random_state=7)
    Wd, Hd = init_device.initialize_nmf_device(X, k, init=init, random_state=7)
    tol = 2e-4 if dtype == np.float32 else 1e-8
    assert Wd.dtype == Wr.dtype and Hd.dtype == Hr.dtype
    if init == "nndsvdar":
        # The random fill of the zeros draws ONE stream over the zeros of W, then of H: an entry that sits within rounding of the
        # 1e-6 cut (sklearn's own fp32 result there depends on the rounding of its LAPACK) moves every later fill by one draw.  So:
        # the SVD-decided entries against scikit-learn's to rounding, the zero pattern equal up to a handful of such entries, the
        # fills equal where the patterns agree from the start and otherwise of the right size.
        Wz, Hz = _initialize_nmf(X, n_components=k, init="nndsvd", random_state=7)
        Wd0, Hd0 = init_device.initialize_nmf_device(X, k, init="nndsvd", random_state=7)
        np.testing.assert_allclose(Wd0, Wz, rtol=tol, atol=tol * np.abs(Wz).max())
        np.testing.assert_allclose(Hd0, Hz, rtol=tol, atol=tol * np.abs(Hz).max())
        flips = int(((Wd0 == 0) != (Wz == 0)).sum() + ((Hd0 == 0) != (Hz == 0)).sum())
        assert flips <= 4, flips
        for got, ref, z0, zr in ((Wd, Wr, Wd0, Wz), (Hd, Hr, Hd0, Hz)):
            kept = (z0 != 0) & (zr != 0)
            np.testing.assert_allclose(got[kept], ref[kept], rtol=tol, atol=tol * np.abs(ref).max())
            filled = (z0 == 0) & (zr == 0)
            assert (got[filled] >= 0).all() and got[filled].max() <= 6 * X.mean() / 100 and abs(got[filled].mean() / ref[filled].mean() - 1) < 0.05
        if flips == 0:
            np.testing.assert_allclose(Wd, Wr, rtol=tol, atol=tol * np.abs(Wr).max())
            np.testing.assert_allclose(Hd, Hr, rtol=tol, atol=tol * np.abs(Hr).max())
        if flips:
            return      # (the entry point below draws the same shifted stream: covered by the other variants)
    else:
        np.testing.assert_allclose(Wd, Wr, rtol=tol, atol=tol * np.abs(Wr).max())
        np.testing.assert_allclose(Hd, Hr, rtol=tol, atol=tol * np.abs(Hr).max())
    # and through the module-level entry point the estimators use
    G, W0, H0 = initialize_algorithms(X, None, None, None, k, init, 7, True, False)
    scale = Hr.sum(axis=0, keepdims=True)
    np.testing.assert_allclose(H0, np.maximum(Hr / scale, 1e-14), rtol=10 * tol, atol=tol)
    np.testing.assert_allclose(W0, np.maximum(Wr * scale.mean(), 1e-14), rtol=10 * tol, atol=tol * np.abs(Wr).max())


def test_one_dimensional_spectrum_fit(SmoothNMF):
    """The reference's 1-D fitting use (espm/datasets/eds_spim.py:228-253): p = 1, k = 1, no shape_2d,
    fixed_H = 1, G an ndarray; and an empty-looking spectrum with all-zero channels (base.py:519-528)."""
    rng = np.random.default_rng(5)
    n, m = 300, 6
    G = rng.random((n, m)) + 0.01
    w = rng.random((m, 1)) * 5
    x = rng.poisson(G @ w).astype(float)
    x[50:60] = 0
    est = SmoothNMF(n_components=1, G=G, fixed_H=np.ones((1, 1)), simplex_H=False, simplex_W=False, max_iter=50, tol=1e-9,
                    verbose=0)
    quiet(est.fit, x)
    ref = oc.fit(x, 1, G=G, fixed_H=np.ones((1, 1)), simplex_H=False, simplex_W=False, max_iter=50, tol=1e-9)
    assert est.H_.shape == (1, 1) and est.W_.shape == (m, 1) and est.n_iter_ == ref["n_iter"]
    np.testing.assert_allclose(est.G_ @ est.W_ @ est.H_, ref["GW"] @ ref["H"], rtol=2e-4, atol=1e-4)
    np.testing.assert_allclose(est.losses_, ref["losses"], rtol=LOSS_RTOL)


def test_k_above_build_limit_is_refused(SmoothNMF):
    X = np.random.default_rng(0).random((40, 50))
    with pytest.raises(NotImplementedError):
        quiet(SmoothNMF(n_components=33, verbose=0, max_iter=2).fit, X)


@pytest.mark.parametrize("k,counts", [(20, True), (32, False)])
def test_whole_fit_with_more_than_sixteen_components(SmoothNMF, k, counts):
    """`fit_transform` end to end on the third build of the library (17..32 components): the NNDSVD initialisation, the fit loop
    with the default stop rule, the results - against the oracle from the same initial matrices."""
    from espm_amd import synth
    from espm_amd.estimators.updates import initialize_algorithms
    n, nx, ny = 120, 16, 20
    prob = synth.make_problem(n, nx, ny, k, N=200.0, seed=k)
    X = synth.sample_numpy(prob, seed=k)
    X[X.sum(axis=1) == 0, 0] = 1.0
    X[0, X.sum(axis=0) == 0] = 1.0
    if not counts:
        X = X * 0.43
    kw = dict(lambda_L=0.5, simplex_H=True, simplex_W=False)
    est = SmoothNMF(n_components=k, shape_2d=(nx, ny), max_iter=25, tol=1e-7, verbose=0, init="nndsvdar", random_state=3, **kw)
    quiet(est.fit, X)
    assert est._engine.V.KP == 32 and est._engine.x_store == ("u8" if counts else "f32")
    # (the same initial matrices for the oracle: the entry point the estimator called, updates.py:160-223)
    _, W0, H0 = initialize_algorithms(X, None, None, None, k, "nndsvdar", 3, True, False)
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, max_iter=25, tol=1e-7, **kw)
    assert est.n_iter_ == ref["n_iter"]
    np.testing.assert_allclose(est.losses_, ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(est.H_, ref["H"], rtol=5e-4, atol=5e-5)
    np.testing.assert_allclose(est.H_.sum(axis=0), 1.0, atol=1e-5)


@pytest.mark.parametrize("case", ["all_ones", "no_ones", "wide", "ones_and_bright"])
def test_sparse_store_unit_rows_edge_cases(case):
    """The two segments of the sparse store's lists at their extremes, against the fp64 oracle: an image of ones (unit
    rows only), an image without a single one (general rows only), more than 4096 channels (no unit rows in the H
    lists, unit rows in the W lists), and ones next to counts that need several general entries."""
    import torch
    from espm_amd.engine import MUEngine
    rng = np.random.default_rng(11)
    if case == "all_ones":
        n, nx, ny, k = 128, 24, 24, 3
        X = np.ones((n, nx * ny))
    elif case == "no_ones":
        n, nx, ny, k = 96, 20, 27, 4
        X = 2.0 * rng.poisson(0.3, size=(n, nx * ny))
    elif case == "wide":
        n, nx, ny, k = 4100, 30, 30, 2
        X = rng.poisson(0.4, size=(n, nx * ny)).astype(np.float64)
    else:
        n, nx, ny, k = 200, 33, 32, 5
        X = rng.poisson(0.5, size=(n, nx * ny)).astype(np.float64)
        X[rng.integers(0, n, 300), rng.integers(0, nx * ny, 300)] = rng.integers(100, 256, 300)
    X[X.sum(axis=1) == 0, 0] = 2.0
    X[0, X.sum(axis=0) == 0] = 2.0
    W0 = rng.uniform(0.05, 1.0, size=(n, k))
    H0 = rng.uniform(0.05, 1.0, size=(k, nx * ny))
    H0 /= H0.sum(axis=0, keepdims=True)
    kw = dict(lambda_L=0.4, simplex_H=True, simplex_W=False)
    ref = oc.fit(X, k, G=None, W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, no_stop_criterion=True,
                 max_iter=5, tol=0, **kw)
    eng = MUEngine(X, k, shape_2d=(nx, ny), max_iter=5, tol=0, x_store="ell", **kw)
    e = eng.ell
    if case == "all_ones":
        assert e["unit_rows_h"] * 128 == e["entries_h"] and e["unit_rows_w"] > 0
    if case == "no_ones":
        assert e["unit_rows_h"] == 0 and e["unit_rows_w"] == 0
    if case == "wide":
        assert e["unit_rows_h"] == 0 and e["unit_rows_w"] > 0
    if case == "ones_and_bright":
        assert 0 < e["unit_rows_h"] < e["rows_h"] and 0 < e["unit_rows_w"] < e["rows_w"]
    eng.load_state(W0, H0)
    eng.iterate(5, final_loss=True)
    torch.cuda.synchronize()
    h = eng.history()
    np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(eng.get_H(), ref["H"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(eng.get_W(), ref["W"], rtol=2e-4, atol=2e-4 * np.abs(ref["W"]).mean())
    assert h["bad"].sum() == 0


def test_linesearch_and_truth_tracking_golden(SmoothNMF, golden, geometry):
    """linesearch=True (gamma_ adapts every iteration) and true_D / true_H tracking against the reference's own
    trajectories (fixture F9)."""
    g = golden("f9_linesearch_truth")
    cfgs = json.loads(str(g["configs"]))
    for name in list(g["names_ls"]) + list(g["names_tm"]):
        c = cfgs[name]
        G = g.get(f"{name}_G")
        shape = tuple(int(v) for v in g[f"{name}_shape"])
        kw = dict(c["kw"], tol=0, no_stop_criterion=True, max_iter=c["iters"])
        if name in g["names_ls"]:
            kw["linesearch"] = True
        else:
            kw.update(true_D=g[f"{name}_true_D"], true_H=g[f"{name}_true_H"])
        est = SmoothNMF(n_components=c["k"], G=G, shape_2d=shape, verbose=0, **kw)
        GW = est.fit_transform(g[f"{name}_X"], W=g[f"{name}_W0"].copy(), H=g[f"{name}_H0"].copy())
        np.testing.assert_allclose(est.losses_, g[f"{name}_losses"], rtol=LOSS_RTOL, err_msg=name)
        det = np.array(est.detailed_losses_, dtype=float)
        np.testing.assert_allclose(det[:, 3], g[f"{name}_detailed"][:, 3], rtol=1e-9, err_msg=name + " gamma")   # same decisions
        np.testing.assert_allclose(det[:, :2], g[f"{name}_detailed"][:, :2], rtol=2e-5, atol=1e-12, err_msg=name)
        # (the Laplacian term is a sum of differences of neighbours: with an unconstrained H - lsw - it is ~1e-2 of the loss and
        # carries the fp32 rounding of H amplified by that ratio)
        np.testing.assert_allclose(det[:, 2], g[f"{name}_detailed"][:, 2], rtol=1e-4, atol=1e-12, err_msg=name)
        np.testing.assert_allclose(est.H_, g[f"{name}_H"], rtol=5e-4, atol=5e-5, err_msg=name)
        np.testing.assert_allclose(GW, g[f"{name}_GW"], rtol=5e-4, atol=5e-4 * np.abs(g[f"{name}_GW"]).mean(), err_msg=name)
        if name in g["names_tm"]:
            np.testing.assert_allclose(est.angles_, g[f"{name}_angles"], rtol=1e-3, atol=1e-3, err_msg=name)
            np.testing.assert_allclose(est.mse_, g[f"{name}_mse"], rtol=1e-3, atol=1e-9, err_msg=name)
            np.testing.assert_allclose(est.true_losses_, g[f"{name}_true_losses"], rtol=LOSS_RTOL, err_msg=name)
            gl = est.get_losses()
            assert list(gl.dtype.names) == json.loads(str(g[f"{name}_loss_names"]))
            got, want = np.array(gl.tolist()), g[f"{name}_get_losses"]
            huge = want > 1e6      # rel_W of an entry thrown onto the clamp (~1e14): order of magnitude only, see _check_traj
            np.testing.assert_allclose(got[~huge], want[~huge], rtol=2e-3, atol=1e-6)
            np.testing.assert_allclose(np.log10(got[huge]), np.log10(want[huge]), atol=1.0)


def test_bregman_variant_golden(SmoothNMF, golden, geometry):
    """use_bregman=True in both step functions and algo="bmd" fits (with mu, lambda, linesearch) against the reference's
    outputs (fixture F10)."""
    from espm_amd.estimators.updates import multiplicative_step_h, multiplicative_step_w
    from espm_amd.utils import create_laplacian_matrix
    g = golden("f10_bregman")
    cfgs = json.loads(str(g["configs"]))
    for name in g["names"]:
        c = cfgs[name]
        shape = tuple(int(v) for v in g[f"{name}_shape"])
        X, W0, H0 = g[f"{name}_X"], g[f"{name}_W0"], g[f"{name}_H0"]
        kw = dict(c["kw"])
        G = np.eye(c["n"])
        Hs = multiplicative_step_h(X, G, W0, H0.copy(), simplex_H=kw["simplex_H"], mu=kw["mu"], lambda_L=kw["lambda_L"],
                                   L=create_laplacian_matrix(*shape), sigmaL=8, use_bregman=True)
        np.testing.assert_allclose(Hs, g[f"{name}_step_H"], rtol=5e-5, atol=5e-6, err_msg=name)
        Ws = multiplicative_step_w(X, G, W0.copy(), H0, use_bregman=True)
        np.testing.assert_allclose(Ws, g[f"{name}_step_W"], rtol=3e-5, atol=1e-7, err_msg=name)
        est = SmoothNMF(n_components=c["k"], shape_2d=shape, verbose=0, algo="bmd", tol=0, no_stop_criterion=True,
                        max_iter=c["iters"], **kw)
        GW = est.fit_transform(X, W=W0.copy(), H=H0.copy())
        np.testing.assert_allclose(est.losses_, g[f"{name}_losses"], rtol=LOSS_RTOL, err_msg=name)
        det = np.array(est.detailed_losses_, dtype=float)
        np.testing.assert_allclose(det[:, 3], g[f"{name}_detailed"][:, 3], rtol=1e-9, err_msg=name + " gamma")
        np.testing.assert_allclose(est.H_, g[f"{name}_H"], rtol=5e-4, atol=5e-5, err_msg=name)
        np.testing.assert_allclose(GW, g[f"{name}_GW"], rtol=5e-4, atol=5e-4 * np.abs(g[f"{name}_GW"]).mean(), err_msg=name)


def test_quadratic_surrogate_golden(SmoothNMF, golden):
    """algo="l2_surrogate": multiplicative_step_hq (positive root of the quadratic surrogate, its own simplex multiplier)
    as a direct call and inside fits (G given, simplex_W, lambda = 0, linesearch) against the reference (fixture F11)."""
    from espm_amd.estimators.updates import multiplicative_step_hq
    from espm_amd.utils import create_laplacian_matrix
    g = golden("f11_quadratic_surrogate")
    cfgs = json.loads(str(g["configs"]))
    for name in g["names"]:
        c = cfgs[name]
        shape = tuple(int(v) for v in g[f"{name}_shape"])
        X, W0, H0 = g[f"{name}_X"], g[f"{name}_W0"], g[f"{name}_H0"]
        G = g.get(f"{name}_G")
        Gd = np.eye(c["n"]) if G is None else G
        kw = dict(c["kw"])
        Hs = multiplicative_step_hq(X, Gd, W0, H0.copy(), simplex_H=kw["simplex_H"], lambda_L=kw["lambda_L"],
                                    L=create_laplacian_matrix(*shape), sigmaL=8)
        # the reference's multiplier is converged to dicotomy_tol = 1e-5 only (global stop rule)
        np.testing.assert_allclose(Hs, g[f"{name}_step_H"], rtol=5e-5, atol=5e-6, err_msg=name)
        if kw["simplex_H"]:
            np.testing.assert_allclose(Hs.sum(axis=0), 1.0, atol=5e-6)
        est = SmoothNMF(n_components=c["k"], G=G, shape_2d=shape, verbose=0, algo="l2_surrogate", tol=0, no_stop_criterion=True,
                        max_iter=c["iters"], **kw)
        GW = est.fit_transform(X, W=W0.copy(), H=H0.copy())
        np.testing.assert_allclose(est.losses_, g[f"{name}_losses"], rtol=3 * LOSS_RTOL, err_msg=name)
        det = np.array(est.detailed_losses_, dtype=float)
        np.testing.assert_allclose(det[:, 3], g[f"{name}_detailed"][:, 3], rtol=1e-9, err_msg=name + " gamma")
        np.testing.assert_allclose(est.H_, g[f"{name}_H"], rtol=1e-3, atol=1e-4, err_msg=name)
        np.testing.assert_allclose(GW, g[f"{name}_GW"], rtol=1e-3, atol=1e-3 * np.abs(g[f"{name}_GW"]).mean(), err_msg=name)


def test_frobenius_fit_golden(SmoothNMF, golden):
    """l2=True inside a fit (the reference keeps it only with algo="l2_surrogate", smooth_nmf.py:223-237): quadratic-surrogate
    H step, Frobenius W step (updates.py:31-36) and loss (base.py:197-198); G given, simplex_W asked for (ignored by that W
    step), normalize, and a run that ends on the stop criterion - against the reference (fixture F14) and the oracle."""
    g = golden("f14_frobenius_fit")
    cfgs = json.loads(str(g["configs"]))
    for name in g["names"]:
        c = cfgs[name]
        shape = tuple(int(v) for v in g[f"{name}_shape"])
        X, W0, H0 = g[f"{name}_X"], g[f"{name}_W0"], g[f"{name}_H0"]
        G = g.get(f"{name}_G")
        kw = dict(c["kw"])
        if not c.get("stop"):
            kw.update(tol=0, no_stop_criterion=True)
        est = SmoothNMF(n_components=c["k"], G=G, shape_2d=shape, verbose=0, algo="l2_surrogate", l2=True, max_iter=c["iters"], **kw)
        GW = quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
        assert est.l2 is True and est._engine.frobenius and est.n_iter_ == int(g[f"{name}_n_iter"]), name
        np.testing.assert_allclose(est.losses_, g[f"{name}_losses"], rtol=3 * LOSS_RTOL, err_msg=name)
        det = np.array(est.detailed_losses_, dtype=float)
        np.testing.assert_allclose(det[:, :3], g[f"{name}_detailed"][:, :3], rtol=1e-3, atol=1e-7, err_msg=name)
        np.testing.assert_allclose(np.array(est.rel_), g[f"{name}_rel"], rtol=2e-2, atol=1e-4, err_msg=name)
        np.testing.assert_allclose(est.H_, g[f"{name}_H"], rtol=1e-3, atol=1e-4, err_msg=name)
        np.testing.assert_allclose(GW, g[f"{name}_GW"], rtol=1e-3, atol=1e-3 * np.abs(g[f"{name}_GW"]).mean(), err_msg=name)
        # loss() of the fitted estimator is the Frobenius one too (base.py:197-198)
        np.testing.assert_allclose(est.loss(est.W_ * (est.norm_factor_ if kw.get("normalize") else 1.0), est.H_), est.losses_[-1],
                                   rtol=1e-5, err_msg=name)


def test_physics_model_trajectories_golden(SmoothNMF, golden, geometry):
    """Fits with a physics model whose G changes with W (fixture F16, generated from the reference with
    tests/physics_double.py mixed into its abstract PhysicalModel): G refreshed after every third iteration and the loss
    re-evaluated with it before the next stop test (base.py:388-392), simplex over the NMF_simplex() rows, the same
    n_iter_ under the default stop rules, and the Frobenius W step with the CURRENT G^T G (l2=True, updates.py:31-36)."""
    from physics_double import AbsorbingModel
    g = golden("f16_physics_model")
    cfgs = json.loads(str(g["configs"]))
    for name in g["names"]:
        c = cfgs[name]
        shape = tuple(int(v) for v in g[f"{name}_shape"])
        model = AbsorbingModel(g[f"{name}_G0"], g[f"{name}_Abs"], float(g[f"{name}_strength"]), c["m0"])
        kw = dict(c["kw"])
        if not c.get("stop"):
            kw.update(tol=0, no_stop_criterion=True)
        est = SmoothNMF(n_components=c["k"], G=model, shape_2d=shape, verbose=0, max_iter=c["iters"], **kw)
        GW = quiet(est.fit_transform, g[f"{name}_X"], W=g[f"{name}_W0"].copy(), H=g[f"{name}_H0"].copy())
        assert est.physics_model_ is model and est.n_iter_ == int(g[f"{name}_n_iter"]) and model.updates == int(g[f"{name}_updates"]), name
        l2 = bool(kw.get("l2"))
        np.testing.assert_allclose(est.losses_, g[f"{name}_losses"], rtol=(3 if l2 else 1) * LOSS_RTOL, err_msg=name)
        det = np.array(est.detailed_losses_, dtype=float)
        np.testing.assert_allclose(det[:, :3], g[f"{name}_detailed"][:, :3], rtol=1e-3 if l2 else 2e-5, atol=1e-7 if l2 else 1e-12, err_msg=name)
        np.testing.assert_allclose(np.array(est.rel_), g[f"{name}_rel"], rtol=2e-2, atol=1e-4, err_msg=name)
        np.testing.assert_allclose(est.G_, g[f"{name}_G"], rtol=2e-5, err_msg=name)
        np.testing.assert_allclose(est.H_, g[f"{name}_H"], rtol=1e-3, atol=1e-4 if l2 else 5e-5, err_msg=name)
        np.testing.assert_allclose(est.W_, g[f"{name}_W"], rtol=1e-3, atol=2e-4 * np.abs(g[f"{name}_W"]).max(), err_msg=name)
        np.testing.assert_allclose(GW, g[f"{name}_GW"], rtol=1e-3, atol=1e-3 * np.abs(g[f"{name}_GW"]).mean(), err_msg=name)
        if kw.get("simplex_W"):
            np.testing.assert_allclose(est.W_[:c["m0"]].sum(axis=0), 1.0, atol=2e-5)


def test_projected_gradient_golden(SmoothNMF, golden):
    """algo="projected_gradient" with a given gamma = [gamma_H, gamma_W]: both steps as direct calls and whole fits (G
    given, mu, lambda, entries at the clamp) against the reference (fixture F12)."""
    from espm_amd.estimators.updates import proj_grad_step_h, proj_grad_step_w
    from espm_amd.utils import create_laplacian_matrix
    g = golden("f12_projected_gradient")
    cfgs = json.loads(str(g["configs"]))
    for name in g["names"]:
        c = cfgs[name]
        shape = tuple(int(v) for v in g[f"{name}_shape"])
        X, W0, H0 = g[f"{name}_X"], g[f"{name}_W0"], g[f"{name}_H0"]
        G = g.get(f"{name}_G")
        Gd = np.eye(c["n"]) if G is None else G
        kw = dict(c["kw"])
        gh, gw = kw["gamma"]
        Hs = proj_grad_step_h(X, Gd, W0, H0.copy(), gh, simplex_H=kw["simplex_H"], mu=kw["mu"], lambda_L=kw["lambda_L"],
                              L=create_laplacian_matrix(*shape))
        np.testing.assert_allclose(Hs, g[f"{name}_step_H"], rtol=5e-5, atol=5e-6, err_msg=name)
        Ws = proj_grad_step_w(X, Gd, W0.copy(), H0, gw, simplex_W=False)
        np.testing.assert_allclose(Ws, g[f"{name}_step_W"], rtol=5e-5, atol=1e-6 * np.abs(W0).mean(), err_msg=name)
        est = SmoothNMF(n_components=c["k"], G=G, shape_2d=shape, verbose=0, algo="projected_gradient", tol=0,
                        no_stop_criterion=True, max_iter=c["iters"], **kw)
        GW = est.fit_transform(X, W=W0.copy(), H=H0.copy())
        np.testing.assert_allclose(est.losses_, g[f"{name}_losses"], rtol=3 * LOSS_RTOL, err_msg=name)
        det = np.array(est.detailed_losses_, dtype=float)
        np.testing.assert_allclose(det[:, 3], g[f"{name}_detailed"][:, 3], rtol=1e-9, err_msg=name + " gamma")
        np.testing.assert_allclose(est.H_, g[f"{name}_H"], rtol=1e-3, atol=1e-4, err_msg=name)
        np.testing.assert_allclose(GW, g[f"{name}_GW"], rtol=1e-3, atol=1e-3 * np.abs(g[f"{name}_GW"]).mean(), err_msg=name)
    with pytest.raises(NotImplementedError):
        quiet(SmoothNMF(n_components=2, algo="projected_gradient", verbose=0).fit, g["p0_X"])   # simplex_W (the default) is refused
    # default gamma: the Lipschitz bounds at log_shift (~X / log_shift^3) - the iterates do not move, like the reference's
    est = SmoothNMF(n_components=3, algo="projected_gradient", simplex_W=False, simplex_H=False, max_iter=3, tol=0, verbose=0,
                    no_stop_criterion=True)
    quiet(est.fit, g["p0_X"], W=g["p0_W0"].copy(), H=g["p0_H0"].copy())
    assert est.gamma_[0] > 1e25 and est.gamma_[1] > 1e25
    assert np.allclose(est.losses_, est.losses_[0], rtol=1e-6)


def test_projected_gradient_linesearch_golden(SmoothNMF, golden):
    """The projected gradient WITH its linesearch (smooth_nmf.py:382-401, :438-447): the sequences of gamma_H / gamma_W the
    quadratic bound produces, and the losses, against the reference (fixture F13; in 'lx' an entry of GWH reaches the clamp
    at iteration 11, the loss jumps by ten orders of magnitude and gamma goes up)."""
    g = golden("f13_projected_gradient_linesearch")
    cfgs = json.loads(str(g["configs"]))
    for name in g["names"]:
        c = cfgs[name]
        shape = tuple(int(v) for v in g[f"{name}_shape"])
        gam = []

        class Rec(SmoothNMF):
            def _detailed(self, lkl, reg, lap):
                gam.append(list(self.gamma_))
                return super()._detailed(lkl, reg, lap)

        est = Rec(n_components=c["k"], G=g.get(f"{name}_G"), shape_2d=shape, verbose=0, algo="projected_gradient", linesearch=True,
                  tol=0, no_stop_criterion=True, max_iter=c["iters"], **c["kw"])
        quiet(est.fit_transform, g[f"{name}_X"], W=g[f"{name}_W0"].copy(), H=g[f"{name}_H0"].copy())
        ref_g, ref_l = g[f"{name}_gammas"], g[f"{name}_losses"]
        gam = np.array(gam)[:len(ref_g)]   # (one more _detailed call comes from the final loss() of a fit without any simplex)
        # up to the first blow-up of the loss every decision is the reference's; at and after it (an entry of GWH at the clamp:
        # the loss depends on the last bits of that entry) only the direction is required: gamma goes up
        n_ok = int(np.argmax(ref_l >= 10.0)) if (ref_l >= 10.0).any() else len(ref_l)
        np.testing.assert_allclose(gam[:n_ok], ref_g[:n_ok], rtol=1e-9, err_msg=name)
        np.testing.assert_allclose(np.array(est.losses_)[:n_ok], ref_l[:n_ok], rtol=3 * LOSS_RTOL, err_msg=name)
        if n_ok < len(ref_l):
            assert est.losses_[n_ok] > 1e3 and (np.diff(gam[n_ok - 1:, 0]) > 0).any() and np.isfinite(est.losses_).all()


def test_sparse_store_at_its_lds_limit():
    """The widest spectrum whose GW table, numerators, riding tail scratch and column-sum copy still fit the sparse H-step's LDS
    budget (k = 5: 7168 channels with the workgroup's whole 160 KB - table and numerators to the last byte, the column-sum copy then
    sits in the dead table, `cs_late`), and one channel row more (dense store): iterations in the C loop against the oracle."""
    import torch
    from espm_amd import _lib, ell, synth
    from espm_amd.engine import MUEngine
    k, nx, ny = 5, 16, 20
    n = max(v for v in range(8, 16384, 8) if ell.lds_bytes_h(v, k) <= _lib.ELL_LDS_MAX)
    assert n == 7168 and ell.lds_bytes_h(n, k) == _lib.ELL_LDS_MAX < ell.lds_bytes_h(n + 8, k)
    rng = np.random.default_rng(4)
    for nn, store in ((n, "ell"), (n + 8, "u8")):
        prob = synth.make_problem(nn, nx, ny, k, N=400.0, seed=4)
        X = np.minimum(synth.sample_numpy(prob, seed=4), 255.0)
        X[X.sum(axis=1) == 0, 0] = 1.0
        X[0, X.sum(axis=0) == 0] = 1.0
        W0, H0 = synth.random_init(nn, k, nx * ny, seed=4, scale=0.05)
        kw = dict(shape_2d=(nx, ny), lambda_L=0.8, simplex_H=True, simplex_W=False)
        eng = MUEngine(X, k, max_iter=5, tol=0, **kw)
        assert eng.x_store == store
        eng.load_state(W0, H0)
        eng.iterate(5, final_loss=True)
        torch.cuda.synchronize()
        h = eng.history()
        ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), exact_root=True, no_stop_criterion=True, max_iter=5, tol=0, **kw)
        np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL)
        np.testing.assert_allclose(h["rel_W"][1:], ref["rel"][:, 0], rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(eng.get_H(), ref["H"], rtol=2e-4, atol=2e-5)
        assert h["bad"].sum() == 0


@pytest.mark.parametrize("fused", ["always", False])
@pytest.mark.parametrize("nx,ny,tile", [(300, 300, 128), (400, 401, 256), (250, 180, 64)])
def test_sparse_store_mid_size_tiles(nx, ny, tile, fused):
    """Images between 256 x 256 and 512 x 512 pixels run the sparse store with 128- and 256-pixel H windows and W blocks of two
    windows, pixels past the last full window included - as one fused launch per block (8 waves) or as the two kernels (two
    or four waves share a list group): whole iterations against the oracle."""
    import torch
    from espm_amd import synth
    from espm_amd.engine import MUEngine
    n, k = 96, 4
    prob = synth.make_problem(n, nx, ny, k, N=25.0, seed=nx)
    X = synth.sample_numpy(prob, seed=nx)
    X[X.sum(axis=1) == 0, 0] = 1.0
    X[:, 1000:1003] = 0                       # a few pixels without counts
    W0, H0 = synth.random_init(n, k, nx * ny, seed=nx, scale=0.2)
    kw = dict(shape_2d=(nx, ny), lambda_L=0.7, mu=0.05, simplex_H=True, simplex_W=False)
    eng = MUEngine(X, k, max_iter=4, tol=0, fused=fused, **kw)
    assert eng.x_store == "ell" and eng.st.tile_px == tile and eng.st.ell_pb == 2 * tile and eng.st.nblk_w == -(-nx * ny // (2 * tile))
    assert bool(eng.lib.espm_mu_fused_applies(C.byref(eng.st))) == bool(fused)
    eng.load_state(W0, H0)
    eng.iterate(4, final_loss=True)
    torch.cuda.synchronize()
    h = eng.history()
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), exact_root=True, no_stop_criterion=True, max_iter=4, tol=0, **kw)
    np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(h["rel_W"][1:], ref["rel"][:, 0], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(h["rel_H"][1:], ref["rel"][:, 1], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(eng.get_H(), ref["H"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(eng.get_W(), ref["W"], rtol=2e-4, atol=2e-4 * np.abs(ref["W"]).mean())
    assert h["bad"].sum() == 0


def test_w_simplex_tolerance_is_the_module_constant(SmoothNMF, golden):
    """The reference's W step calls dichotomy_simplex with conf.dicotomy_tol whatever the estimator's dicotomy_tol is
    (updates.py:61-68: multiplicative_step_w has no such argument; only the H step takes it): a looser dicotomy_tol must not
    change a fit that has a simplex over W only."""
    g = golden("f6_trajectories")
    X, W0, H0 = g["cw_X"], g["cw_W0"], g["cw_H0"]
    shape = tuple(int(v) for v in g["cw_shape"])
    c = json.loads(str(g["configs"]))["cw"]
    fits = []
    for tol in (1e-5, 1e-2):
        est = SmoothNMF(n_components=c["k"], shape_2d=shape, verbose=0, tol=0, no_stop_criterion=True, max_iter=20, dicotomy_tol=tol, **c["kw"])
        quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
        fits.append((est.W_.copy(), est.H_.copy(), np.array(est.losses_)))
    assert c["kw"].get("simplex_W") and not c["kw"].get("simplex_H")
    np.testing.assert_array_equal(fits[0][0], fits[1][0])
    np.testing.assert_array_equal(fits[0][2], fits[1][2])


@pytest.mark.parametrize("n,nx,ny,k,kw", [
    (96, 14, 17, 3, dict(simplex_H=False, simplex_W=True)),
    (160, 9, 21, 5, dict(simplex_H=False, simplex_W=True, lambda_L=0.5, mu=0.1)),
    (2048, 8, 12, 8, dict(simplex_H=False, simplex_W=True, lambda_L=1.0)),   # (449 channels without a count at this dose)
    (64, 20, 20, 1, dict(simplex_H=False, simplex_W=True)),
])
def test_simplex_over_w_as_many_workgroups(n, nx, ny, k, kw):
    """With G = identity and every row in the simplex the multipliers of the W update follow from per-component sums over
    the channels: two many-workgroup launches (w_reduce_kernel's partials + w_simplex_update_kernel) instead of one
    workgroup that searches them.  Against the oracle (the reference's global-stop bisection) and against the one-workgroup
    finish of the same build (fused=False), including empty channels (numerators of zero) and a fixed entry of W."""
    import torch
    from espm_amd import synth
    from espm_amd.engine import MUEngine
    prob = synth.make_problem(n, nx, ny, k, N=60.0, seed=n + k)
    X = synth.sample_numpy(prob, seed=n + k)
    X[5] = 0                      # a channel without counts: its numerators are zero, it takes eps
    X[0, X.sum(axis=0) == 0] = 1.0
    W0, H0 = synth.random_init(n, k, nx * ny, seed=n + k, scale=0.2)
    W0 /= W0.sum(axis=0, keepdims=True)
    fixed_W = -np.ones((n, k))
    fixed_W[3, 0] = 0.01
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), no_stop_criterion=True, max_iter=8, tol=0, fixed_W=fixed_W, **kw)
    out = {}
    for name, fused in (("split", True), ("one_workgroup", False)):
        eng = MUEngine(X, k, shape_2d=(nx, ny), max_iter=8, tol=0, fixed_W=fixed_W, fused=fused, **kw)
        assert eng.st.n_pad % 32 == 0
        eng.load_state(W0, H0)
        eng.iterate(8, final_loss=True)
        torch.cuda.synchronize()
        h = eng.history()
        assert h["bad"].sum() == 0
        out[name] = (eng.get_W(), eng.get_H(), h["loss"], h["rel_W"])
    W, H, loss, rel_w = out["split"]
    np.testing.assert_allclose(loss[1:], ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(W, ref["W"], rtol=2e-4, atol=2e-4 * np.abs(ref["W"]).mean())
    np.testing.assert_allclose(H, ref["H"], rtol=2e-4, atol=5e-5)
    np.testing.assert_allclose(W.sum(axis=0) - W[3, 0] + 0.0, ref["W"].sum(axis=0) - ref["W"][3, 0], rtol=1e-4)
    # the same multipliers as the one-workgroup finish: the same sweep, the same midpoint (fused=False also takes the two-launch
    # H / W kernels, whose numerators are summed in another order than the fused launch's: 4e-6 after 8 iterations, not 2e-6)
    np.testing.assert_allclose(W, out["one_workgroup"][0], rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(loss, out["one_workgroup"][2], rtol=1e-6)
    np.testing.assert_allclose(rel_w[1:], out["one_workgroup"][3][1:], rtol=1e-4, atol=1e-6)   # (near the fixed point rel_W is rounding noise of the two summation orders)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(64, 12, 12), (512, 96, 96)])   # the host path of a small X, the device path of a large one
def test_fitted_estimator_is_freed_with_its_last_reference(SmoothNMF, shape):
    """A fitted estimator, its X_ (2 GB at the headline size) and its engine's device memory go when the last reference does - by
    reference counting, not whenever the cyclic collector gets to them (the reference's own caller check, base.py:249-259, leaves a
    frame <-> frame-list cycle behind: here it is broken)."""
    import gc
    import weakref
    n, nx, ny = shape
    rng = np.random.default_rng(1)
    X = rng.poisson(0.4, size=(n, nx * ny)).astype(np.float32)
    was = gc.isenabled()
    gc.disable()
    try:
        est = SmoothNMF(n_components=3, lambda_L=1.0, simplex_H=True, shape_2d=(nx, ny), max_iter=6, tol=0, verbose=0, random_state=0)
        quiet(est.fit_transform, X)
        _ = np.asarray(est.X_)
        refs = [weakref.ref(est)]
        eng = getattr(est, "_engine", None)
        if eng is not None:
            refs.append(weakref.ref(eng))
        del eng, _
        del est
        assert all(r() is None for r in refs), "a fitted estimator (or its engine) outlives its last reference: a reference cycle"
    finally:
        if was:
            gc.enable()


@pytest.mark.parametrize("layout", ["channels_first", "pixels_first"])
@pytest.mark.parametrize("normalize,dtype,holes", [(False, np.float32, False), (False, np.float32, True), (True, np.float64, True), (True, np.float32, False)])
def test_device_preparation_of_a_large_x_matches_the_oracle(SmoothNMF, layout, normalize, dtype, holes):
    """An X large enough for the device preparation (one upload in chunks, the reference's pre-loop passes over X - finiteness,
    sign, empty lines base.py:519-528, mean for `normalize` base.py:264-267, const_KL_ base.py:200-201 - riding behind the
    chunks; the engine's store chosen from the same scans) against the oracle fed the same array on the host: with and without
    empty channels / pixels (the filled branch takes its own passes), `normalize`, both precisions, and a (pixels, channels)
    array handed over with hspy_comp (uploaded as it lies)."""
    from espm_amd import synth
    from espm_amd.estimators import ingest
    n, nx, ny, k = 600, 90, 80, 3
    assert n * nx * ny >= ingest._DEVICE_PREP_MIN_SIZE
    prob = synth.make_problem(n, nx, ny, k, N=40.0, seed=5)
    X = synth.sample_numpy(prob, seed=5).astype(dtype)
    X[0, X.sum(axis=0) == 0] = 1.0                     # (no accidental holes: the parameter decides)
    X[X.sum(axis=1) == 0, 0] = 1.0
    if holes:
        X[:5] = 0
        X[300:303] = 0
        X[:, 1000:1040] = 0
        X[:, -7:] = 0
    W0, H0 = synth.random_init(n, k, nx * ny, seed=5, scale=0.07)
    kw = dict(lambda_L=1.0, simplex_H=True, simplex_W=False, shape_2d=(nx, ny), max_iter=6, tol=0, normalize=normalize)
    ref = oc.fit(X.astype(np.float64), k, W=W0.copy(), H=H0.copy(), exact_root=True, no_stop_criterion=True, **kw)
    est = SmoothNMF(n_components=k, no_stop_criterion=True, verbose=0, hspy_comp=(layout == "pixels_first"), **kw)
    if layout == "pixels_first":
        out = quiet(est.fit_transform, np.ascontiguousarray(X.T), W=W0.copy(), H=H0.copy())
        assert est._ingest_layout == "pm" and out.shape == (nx * ny, k)
        np.testing.assert_allclose(out, ref["H"].T, rtol=2e-4, atol=5e-5)
    else:
        GW = quiet(est.fit_transform, X, W=W0.copy(), H=H0.copy())
        np.testing.assert_allclose(GW, ref["GW"], rtol=2e-4, atol=2e-4 * np.abs(ref["GW"]).mean())
    np.testing.assert_allclose(est.losses_, ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(est.H_, ref["H"], rtol=2e-4, atol=5e-5)
    scale = np.abs(ref["W"]).mean()
    np.testing.assert_allclose(est.W_, ref["W"], rtol=2e-4, atol=2e-4 * scale)
    Xh = np.asarray(est.X_)
    assert Xh.shape == X.shape and Xh.dtype == X.dtype
    if not normalize:
        filled = X.copy()
        if holes:
            filled[:, X.sum(axis=0) == 0] = est.log_shift
            filled[X.sum(axis=1) == 0, :] = est.log_shift
        np.testing.assert_array_equal(Xh, filled)        # the estimator's own copy, lines filled like remove_zeros_lines
    # what must NOT pass the device preparation
    bad = X.copy()
    bad[3, 17] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        quiet(SmoothNMF(n_components=k, verbose=0, **kw).fit_transform, bad)
    bad[3, 17] = -1.0
    with pytest.raises(ValueError, match="Negative values in data"):
        quiet(SmoothNMF(n_components=k, verbose=0, **kw).fit_transform, bad)


def test_sparse_counts_whose_table_does_not_fit_take_the_dense_store_and_say_so():
    """VERDICT r4 (missing 3): 13-16 components at 2048 channels - the sparse store's table of 16-float rows does not fit the LDS -
    must not drop to the dense store silently: a RuntimeWarning and MUEngine.x_store_note; the fit itself still follows the oracle."""
    import torch
    from espm_amd.engine import MUEngine
    from oracle import mu_oracle as oc
    rng = np.random.default_rng(3)
    n, nx, ny, k = 2120, 12, 12, 14      # (14 components: up to 2112 channels)
    X = rng.poisson(0.2, size=(n, nx * ny)).astype(np.float64)
    X[:, 0] += 1.0
    X[0, :] += 1.0
    W0, H0 = rng.random((n, k)) + 0.1, rng.random((k, nx * ny)) + 0.1
    with pytest.warns(RuntimeWarning, match="dense 8-bit store"):
        eng = MUEngine(torch.from_numpy(X.astype(np.float32)).cuda(), k, layout="cm", shape_2d=(nx, ny), lambda_L=0.5, simplex_H=True, simplex_W=False,
                       tol=0.0, max_iter=6)
    assert eng.x_store == "u8" and "LDS" in eng.x_store_note
    eng.load_state(W0, H0)
    eng.iterate(3, final_loss=True)
    torch.cuda.synchronize()
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), lambda_L=0.5, simplex_H=True, simplex_W=False, shape_2d=(nx, ny), tol=0, no_stop_criterion=True, max_iter=3)
    np.testing.assert_allclose(eng.history()["loss"][1:4], ref["losses"], rtol=1e-5)
    # the same data with 5 components: the sparse store, no warning
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng5 = MUEngine(torch.from_numpy(X.astype(np.float32)).cuda(), 5, layout="cm", shape_2d=(nx, ny), lambda_L=0.5, simplex_H=True, simplex_W=False, tol=0.0, max_iter=6)
    assert eng5.x_store == "ell" and eng5.x_store_note is None


@pytest.mark.parametrize("k,n", [(13, 2048), (15, 2048), (16, 2048), (12, 2896), (9, 3024), (8, 4608), (4, 9216)])
def test_sparse_store_at_the_160_kb_limits(k, n):
    """sparse count data with 13-16 components at the headline's 2048 channels used to drop to the dense 8-bit store
    (the sparse H-step was given 144 KB of LDS; table rows of 16 floats: 128 KB + the numerators).  With the workgroup's whole 160 KB
    13-15 components fit, and 16 to the last byte - its column-sum copy then lives in the table once the walk has left it.  Whole
    iterations (the C loop, the W update's tail riding in the H-step launch) against the oracle."""
    import warnings
    import torch
    from espm_amd import _lib, ell, synth
    from espm_amd.engine import MUEngine
    nx, ny = 20, 30
    # (the other pairs: the widest spectrum the 160 KB hold at 12, 9, 8 and 4 components - 144 KB held 2552, 2680, 4088, 8184)
    assert ell.lds_bytes_h(n, k) <= _lib.ELL_LDS_MAX and (n == 2048 and k < 16 or ell.lds_bytes_h(n + 8, k) > _lib.ELL_LDS_MAX)
    assert k != 16 or ell.lds_bytes_h(n, k) == _lib.ELL_LDS_MAX
    prob = synth.make_problem(n, nx, ny, k, N=300.0, seed=k)
    X = np.minimum(synth.sample_numpy(prob, seed=k), 255.0)
    X[X.sum(axis=1) == 0, 0] = 1.0
    X[0, X.sum(axis=0) == 0] = 1.0
    W0, H0 = synth.random_init(n, k, nx * ny, seed=k, scale=0.1)
    kw = dict(shape_2d=(nx, ny), lambda_L=0.6, mu=0.02, simplex_H=True, simplex_W=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng = MUEngine(X, k, max_iter=6, tol=0, **kw)
    assert eng.x_store == "ell" and eng.V.KP == (16 if k > 8 else 8) and eng.x_store_note is None
    eng.load_state(W0, H0)
    eng.iterate(6, final_loss=True)
    torch.cuda.synchronize()
    h = eng.history()
    ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), exact_root=True, no_stop_criterion=True, max_iter=6, tol=0, **kw)
    np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL)
    np.testing.assert_allclose(h["rel_W"][1:], ref["rel"][:, 0], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(eng.get_H(), ref["H"], rtol=2e-4, atol=2e-5)
    assert h["bad"].sum() == 0


@pytest.mark.parametrize("algo", ["projected_gradient", "log_surrogate"])
def test_w_finishes_of_a_dictionary_over_5000_channels(SmoothNMF, algo):
    """A dictionary G over MORE than 4096 channels: both rules run the one-workgroup W finish that keeps nothing in registers
    (`w_finish_kernel`: the register-resident finishes hold up to four channels per thread).  projected_gradient: the branch it lacked
    until round 5.  log_surrogate: with m = 9 and k = 3 the workspace of 2 m k floats (216 bytes) does not hold the 20 row workgroups'
    partial column sums (1296), so the two-launch finish does not apply here either - its case at 5000 channels is the row
    n-dict-two-5000 of tests/test_gpu_w_update_forms.py.  Against the oracle."""
    rng = np.random.default_rng(11)
    n, nx, ny, k, m = 5000, 10, 12, 3, 9
    p = nx * ny
    G = rng.random((n, m)) * (rng.random((n, m)) < 0.5) + 0.01
    W = rng.random((m, k)) * 30.0 / n
    H = rng.random((k, p)) ** 2 + 0.03
    H /= H.sum(axis=0, keepdims=True)
    X = rng.poisson(G @ W @ H * 40).astype(np.float64) / 40
    X[X.sum(axis=1) == 0, 0] = 0.025
    X[0, X.sum(axis=0) == 0] = 0.025
    W0 = rng.random(W.shape) * W.mean() * 2 + 1e-3
    H0 = rng.random((k, p)) + 0.05
    H0 /= H0.sum(axis=0, keepdims=True)
    kw = dict(simplex_H=True, simplex_W=False, lambda_L=0.3, mu=0)
    L = oc.laplacian_matrix(nx, ny)
    gh = np.abs(oc.gradH(X, G, W0, H0, mu=0, lambda_L=0.3, L=L)).max()
    gw = np.abs(oc.gradW(X, G, W0, H0)).max()
    gamma = [float(gh / 0.05), float(gw / (0.2 * W0.mean()))]
    extra = dict(gamma=gamma) if algo == "projected_gradient" else {}
    ref = oc.fit(X, k, G=G, W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), algo=algo, tol=0, no_stop_criterion=True, max_iter=5,
                 exact_root=(algo == "log_surrogate"), **extra, **kw)
    assert np.isfinite(ref["losses"]).all() and (np.diff(ref["losses"]) <= 0).all()
    est = SmoothNMF(n_components=k, G=G, shape_2d=(nx, ny), algo=algo, tol=0, no_stop_criterion=True, max_iter=5, verbose=0, **extra, **kw)
    quiet(est.fit, X, W=W0.copy(), H=H0.copy())
    assert est._engine.w_update_form() == ("one_wg_general", {})
    np.testing.assert_allclose(est.losses_, ref["losses"], rtol=1e-4)
    np.testing.assert_allclose(est.H_, ref["H"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(est.W_, ref["W"], rtol=2e-3, atol=2e-3 * np.abs(ref["W"]).mean())

