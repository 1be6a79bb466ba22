"""Residual products and components on the device against their numpy restatement (tests/residuals_reference.py): both sides, the four
dtypes and both layouts within the derived bounds and bit-equal where that is promised, component and vector counts, two chunks with a
ragged second one, strided rows, the floor rule on a planted model, the adjoint, the subspace iteration and the scree against numpy's
SVD, the sampled null, the estimator's method on a fit with a missing phase, and the adapter.

The image is the splitting tests' 96 channels x 40 x 33 pixels: 1320 pixels are a ragged last wave and workgroup, 96 channels cross a
transposing tile of 64, 32 or 16 rows; the model has an all-zero row of D and all-zero columns of H.  16 and 300 channels x 2118 pixels
run two chunks of the channel side, the second of 70 pixels, with lanes that are no multiple of 64."""
import functools

import numpy as np
import pytest

import marginals_reference as mr
import residuals_reference as rr

pytestmark = pytest.mark.gpu

N, SHAPE = 96, (40, 33)
P = SHAPE[0] * SHAPE[1]
SIDES = ["pixels", "channels"]


@pytest.fixture(scope="module")
def residuals():
    from espm_amd import residuals
    return residuals


@functools.lru_cache(maxsize=None)
def _image(n, shape, dtype):
    return mr.image(n, shape, np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _model(n, p, k):
    return rr.planted_model(n, p, k, channel=min(20, n - 1), pixel=500)


def _dense(g, m, seed=1):
    return np.random.default_rng(seed + 10 * g).standard_normal((g, m))


def _lay(X, layout):
    return X if layout == "cm" else np.ascontiguousarray(X.T)


def _run(X, V, D, H, side, layout="cm", pad=0, **kw):
    """``residuals.products`` with chi2; ``pad``: X on the device with rows ``pad`` entries apart more than they are long."""
    from espm_amd import residuals
    Xl = _lay(X, layout)
    if pad:
        import torch
        wide = torch.zeros((Xl.shape[0], Xl.shape[1] + pad), dtype=getattr(torch, Xl.dtype.name), device="cuda")
        wide[:, :Xl.shape[1]] = torch.from_numpy(Xl).to("cuda")
        Xl = wide[:, :Xl.shape[1]]
        assert Xl.stride(0) == Xl.shape[1] + pad
    return residuals.products(Xl, V, D, H, side=side, layout=layout, chi2=True, **kw)


def _within(got, ref, what):
    for name in ("out", "chi2"):
        err = np.abs(got[name] - ref[name])
        b = ref[name + "_bound"]
        assert got[name].shape == ref[name].shape and np.isfinite(got[name]).all()
        room = float((err / np.where(b > 0, b, 1)).max())
        print(f"{what}: {name} worst error / bound {room:.3g}")
        assert (err <= b).all(), (what, name, room)
    assert got["unmodelled"] == ref["unmodelled"], what


def _same(a, b):
    return np.array_equal(a["out"], b["out"]) and np.array_equal(a["chi2"], b["chi2"]) and a["unmodelled"] == b["unmodelled"]


# ---- the products ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
def test_products_are_within_the_derived_bounds(dtype, side):
    X = _image(N, SHAPE, dtype)
    D, H = _model(N, P, 3)
    V = _dense(3, N if side == "pixels" else P)
    ref = rr.products(X, V, D, H, side)
    for layout in ("cm", "pm"):
        _within(_run(X, V, D, H, side, layout), ref, f"{dtype}, {side}, {layout}")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("g", [1, 4, 5, 8])
@pytest.mark.parametrize("k", [1, 4, 5, 8])
def test_component_and_vector_counts(k, g, side):
    X = _image(N, SHAPE, "uint8")
    D, H = _model(N, P, k)
    V = _dense(g, N if side == "pixels" else P)
    _within(_run(X, V, D, H, side), rr.products(X, V, D, H, side), f"k = {k}, g = {g}, {side}")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("n", [16, 300])
def test_two_chunks_with_a_ragged_second_one(n, dtype, side):
    shape = (6, 353)   # 2048 + 70 pixels
    p = shape[0] * shape[1]
    X = _image(n, shape, dtype)
    D, H = _model(n, p, 5)
    V = _dense(5, n if side == "pixels" else p)
    ref = rr.products(X, V, D, H, side)
    a, b = _run(X, V, D, H, side, "cm"), _run(X, V, D, H, side, "pm")
    _within(a, ref, f"n = {n}, {dtype}, {side}")
    assert _same(a, b)


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("side", SIDES)
def test_strided_rows(side, layout):
    X = _image(N, SHAPE, "uint8")
    D, H = _model(N, P, 3)
    V = _dense(3, N if side == "pixels" else P)
    assert _same(_run(X, V, D, H, side, layout, pad=13), _run(X, V, D, H, side, layout))


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
def test_both_layouts_and_two_calls_give_the_same_bits(dtype):
    X = _image(N, SHAPE, dtype)
    D, H = _model(N, P, 3)
    for side in SIDES:
        V = _dense(4, N if side == "pixels" else P)
        a = _run(X, V, D, H, side, "cm")
        assert _same(a, _run(X, V, D, H, side, "cm")) and _same(a, _run(X, V, D, H, side, "pm"))


def test_chi2_and_the_count_agree_from_both_sides():
    X = _image(N, SHAPE, "uint16")
    D, H = _model(N, P, 3)
    pix, chan = _run(X, _dense(1, N), D, H, "pixels"), _run(X, _dense(1, P), D, H, "channels")
    rp, rc = rr.products(X, _dense(1, N), D, H, "pixels"), rr.products(X, _dense(1, P), D, H, "channels")
    gap = abs(pix["chi2"].sum() - chan["chi2"].sum())
    bound = rp["chi2_bound"].sum() + rc["chi2_bound"].sum() + rr.gamma(N + P) * (rp["chi2"].sum() + rc["chi2"].sum())   # (and the sums here)
    print(f"chi2 summed from either side: gap {gap:.3g}, bound {bound:.3g}")
    assert gap <= bound and pix["unmodelled"] == chan["unmodelled"] == rp["unmodelled"] > 0


def test_the_floor_rule_on_a_planted_model():
    """An all-zero row of D and zero columns of H: those entries leave E and the ones with counts are counted.  Without the floor rule
    an entry there is (x - 0) / sqrt(0), or with the marginals' floor x / 1e-7."""
    X = _image(N, SHAPE, "uint16")
    D, H = _model(N, P, 3)
    e, _, floored, unmodelled = rr.pearson(X, D, H)
    assert floored[20].all() and floored[:, 500].all() and floored[:, 11].all() and unmodelled == int((X[floored] > 0).sum()) > 100
    for side in SIDES:
        V = np.ones((1, N if side == "pixels" else P))
        got = _run(X, V, D, H, side)
        assert got["unmodelled"] == unmodelled
        want = e.sum(axis=0 if side == "pixels" else 1)
        assert np.abs(got["out"][0] - want).max() <= rr.products(X, V, D, H, side)["out_bound"].max()
        if side == "pixels":
            assert not got["out"][0, [11, 500]].any() and not got["chi2"][[11, 500]].any()
        else:
            assert got["out"][0, 20] == 0 and got["chi2"][20] == 0


def test_the_adjoint():
    X = _image(N, SHAPE, "uint8")
    D, H = _model(N, P, 3)
    u, v = _dense(2, N, seed=5), _dense(2, P, seed=6)
    Ev, Etu = _run(X, v, D, H, "channels"), _run(X, u, D, H, "pixels")
    bv, bu = rr.products(X, v, D, H, "channels")["out_bound"], rr.products(X, u, D, H, "pixels")["out_bound"]
    for q in range(2):
        left, right = u[q] @ Ev["out"][q], Etu["out"][q] @ v[q]
        # each product's own bound carried through the closing dot product, and that product's roundings
        bound = np.abs(u[q]) @ bv[q] + bu[q] @ np.abs(v[q]) + rr.gamma(N) * (np.abs(u[q]) @ np.abs(Ev["out"][q])) + rr.gamma(P) * (np.abs(Etu["out"][q]) @ np.abs(v[q]))
        print(f"adjoint {q}: u . (E v) = {left:.12g}, (E^T u) . v = {right:.12g}, gap {abs(left - right):.3g}, bound {bound:.3g}")
        assert abs(left - right) <= bound


def test_more_vectors_than_a_launch_and_device_vectors(residuals):
    import torch
    X = _image(N, SHAPE, "uint8")
    D, H = _model(N, P, 3)
    for side in SIDES:
        V = _dense(11, N if side == "pixels" else P)
        whole, first, rest = _run(X, V, D, H, side), _run(X, V[:8], D, H, side), _run(X, V[8:], D, H, side)
        assert np.array_equal(whole["out"], np.concatenate([first["out"], rest["out"]])) and np.array_equal(whole["chi2"], first["chi2"])
        dev = residuals.products(X, torch.from_numpy(V).to("cuda"), D, H, side=side, chi2=True, device=True)
        assert dev["out"].is_cuda and np.array_equal(dev["out"].cpu().numpy(), whole["out"]) and np.array_equal(dev["chi2"].cpu().numpy(), whole["chi2"])
    with pytest.raises(ValueError, match="float64"):
        residuals.products(X, torch.ones((1, N), device="cuda"), D, H)


# ---- the decomposition ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _three():
    return rr.three_phase()


def _accept(out, sv, tol):
    """tests/test_residuals_cpu.py's acceptance: every value within rho_i + 1e-9 s_1 of a true one, the separated ones to 10 tol."""
    for i, (s, r) in enumerate(zip(out["singular_values"], out["ritz_residuals"])):
        gap = np.abs(sv - s).min()
        print(f"s_{i + 1} = {s:.6f}: rho {r:.3g}, nearest true value {gap:.3g} away, relative error to its own {abs(s - sv[i]) / sv[i]:.3g}")
        assert gap <= r + 1e-9 * sv[0], (i, gap, r)
    separated = [i for i in range(len(out["singular_values"])) if sv[i] >= 1.25 * sv[8]]
    for i in separated:
        assert abs(out["singular_values"][i] - sv[i]) <= 10 * tol * sv[i], i
    return separated


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_svd_against_numpys(residuals, layout):
    f = _three()
    X, D, H = f["X"], f["D"][:, :2], rr.two_phase_H(f["H"])
    e = rr.pearson(X, D, H)[0]
    sv = np.linalg.svd(e, compute_uv=False)
    out = residuals.svd(_lay(X, layout), D, H, n_vectors=4, layout=layout)
    print(f"{out['n_iter']} iterations, converged {out['converged']}")
    assert out["converged"] and 0 in _accept(out, sv, 1e-10)
    assert out["spectra"].shape == (N, 4) and out["maps"].shape == (4, P) and out["unmodelled"] == 0
    assert out["chi2_total"] == pytest.approx((e * e).sum(), rel=1e-12) and np.allclose(out["chi2_map"], (e * e).sum(axis=0), rtol=1e-12)
    assert abs(rr.corr(out["maps"][0], f["disc"])) >= 0.8 and abs(rr.corr(out["spectra"][:, 0], f["D"][:, 2])) >= 0.8
    assert out["spectra"][np.abs(out["spectra"][:, 0]).argmax(), 0] > 0 and out["spectra"][:, 0] @ e @ out["maps"][0] > 0


def test_scree_against_numpys(residuals):
    X = _three()["X"]
    D, H, T = rr.independence(X)
    Dm, Hm = residuals.independence_model(X)
    assert np.array_equal(Dm, D) and np.array_equal(Hm, H)   # integer sums: exact
    sv = np.linalg.svd(rr.pearson(X, D, H)[0], compute_uv=False)
    out = residuals.scree(X)
    assert _accept(out, sv, 1e-10) == [0, 1] and out["singular_values"].shape == (6,) and out["total_counts"] == T
    x = X.astype(np.float64)
    pca = np.linalg.svd(x / np.sqrt(np.outer(x.sum(axis=1), x.sum(axis=0))), compute_uv=False)
    assert np.allclose(out["normalised_pca"][:2], pca[1:3], rtol=1e-9, atol=0)


def test_adapter_scree_on_the_raw_cube(residuals):
    from espm_amd import hyperspy_adapter as ha
    X = _three()["X"]
    sig = ha.SpectrumImage(np.ascontiguousarray(X.T).reshape(SHAPE + (N,)))
    got, want = sig.scree(n_vectors=3), residuals.scree(np.ascontiguousarray(X.T), n_vectors=3, layout="pm")
    assert got["maps"].shape == (3,) + SHAPE and got["chi2_map"].shape == SHAPE
    assert np.array_equal(got["singular_values"], want["singular_values"]) and np.array_equal(got["maps"].reshape(3, P), want["maps"])
    assert np.array_equal(got["normalised_pca"], want["normalised_pca"]) and np.array_equal(got["spectra"], want["spectra"])


def test_null_singular_values(residuals):
    """The top value of replicates of the three-phase model against itself: near the edge, the same from call to call, replicate by
    replicate."""
    f = _three()
    null = residuals.null_singular_values(f["D"], f["H"], n_rep=3, seed=4)
    edge = np.sqrt(N) + np.sqrt(P)
    print(f"null of the three-phase model: {null}, edge {edge:.2f}")
    assert null.shape == (3,) and (null > 0.9 * edge).all() and (null < 1.1 * edge).all()
    assert np.array_equal(residuals.null_singular_values(f["D"], f["H"], n_rep=2, seed=4, replicate0=1), null[1:])
    with pytest.raises(ValueError, match="saturated"):
        residuals.null_singular_values(f["D"] * 1e5, f["H"], n_rep=1)


# ---- the estimator ----------------------------------------------------------------------------------------------------------------------------
def _fit(k, hspy_comp=False, normalize=False, group=None):
    """The estimator as it comes - no regularisation, its default initialisation - run until it stops by tol."""
    from espm_amd.estimators import SmoothNMF
    est = SmoothNMF(n_components=k, max_iter=5000, tol=1e-7, verbose=0, random_state=0, shape_2d=SHAPE, hspy_comp=hspy_comp, normalize=normalize)
    if group is not None:
        est.shard(group)
    X = _three()["X"]
    Xin = np.ascontiguousarray(X.T) if hspy_comp else X
    est.fit(Xin.astype(np.float32))
    return est, Xin


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("hspy_comp", [False, True], ids=["cm", "hspy"])
def test_estimator_finds_the_missing_phase(residuals, hspy_comp, normalize):
    """three_phase fitted with k = 2: the disc and the third spectrum are the leading residual component, far above the null.
    Measured with numpy MU (tests/residuals_reference.py): 3.1 times the largest null value, correlations 0.94 and 0.94; with this
    estimator (316 iterations): s_1 = 168.7 against a null of 45.7 .. 49.4, 3.4 times, correlations 0.97 and 0.95; under
    ``normalize`` (222 iterations): 143.9 against 45.7 .. 46.9, 3.1 times, 0.94 and 0.94.

    The factor rests on the null's LARGEST value, and at these doses that is a heavy-tailed number: the fit holds entries with a
    model far below one count (W entries at the floor), and a replicate that draws a single count at one of them carries e = 1 / sqrt(y)
    there.  Measured: the same fit started with init="nndsvdar" ends at s_1 = 143.8 and replicate 0 of its null draws one count at
    y = 7.8e-5 (e = 113): that replicate's top value is 119.6 where the other nine are 45.6 .. 46.4, and the factor is 1.20 -
    ``residual_pvalue_`` (1 / 11) and ``residual_n_significant_`` (1) are unmoved.  That is what the sampled null is for."""
    from espm_amd import hyperspy_adapter as ha
    f = _three()
    est, Xin = _fit(2, hspy_comp, normalize)
    kept = {a: np.array(getattr(est, a), copy=True) for a in ("W_", "H_", "G_", "components_", "X_")}
    out = est.residual_components(n_vectors=3, X=Xin, n_null=10)
    s, null = est.residual_singular_values_, est.residual_null_
    cm, cs = rr.corr(est.residual_maps_[0], f["disc"]), rr.corr(est.residual_spectra_[:, 0], f["D"][:, 2])
    print(f"k = 2 after {est.n_iter_} iterations: s = {s}, null {null.min():.2f} .. {null.max():.2f}, ratio {s[0] / null.max():.2f}, "
          f"corr map {cm:.3f}, spectrum {cs:.3f}, n_significant {est.residual_n_significant_}, p {est.residual_pvalue_:.3f}")
    assert est.n_iter_ < 5000   # (stopped by tol)
    assert s.shape == (3,) and est.residual_spectra_.shape == (N, 3) and est.residual_maps_.shape == (3, P) and null.shape == (10,)
    assert est.residual_chi2_map_.shape == (P,) and est.residual_explained_.shape == (3,) and est.residual_edge_ == np.sqrt(N) + np.sqrt(P)
    assert s[0] > 2.0 * null.max() and est.residual_n_significant_ >= 1 and est.residual_pvalue_ == 1 / 11
    assert abs(cm) >= 0.8 and abs(cs) >= 0.8
    assert out["singular_values"] is s and out["n_significant"] == est.residual_n_significant_ and np.array_equal(out["null"], null)
    D, H = est._model_counts()
    want = residuals.svd(Xin, D, H, n_vectors=3, log_shift=est.log_shift, layout="pm" if hspy_comp else "cm")
    assert np.array_equal(want["singular_values"], s) and np.array_equal(want["maps"], est.residual_maps_)
    assert np.array_equal(residuals.null_singular_values(D, H, n_rep=10, seed=0, log_shift=est.log_shift), null)
    # X=None: the fit's own X_, un-scaled
    mine = est.residual_components(n_vectors=3)
    assert np.allclose(mine["singular_values"], s, rtol=1e-5) and abs(rr.corr(mine["maps"][0], want["maps"][0])) > 0.999
    assert not hasattr(est, "residual_null_") or np.array_equal(est.residual_null_, null)
    maps, spectra = ha.residual_components(est)
    assert maps.shape == (3,) + SHAPE and spectra.shape == (3, N) and np.array_equal(maps.reshape(3, P), est.residual_maps_)
    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), a


def test_estimator_with_every_phase_finds_nothing():
    """The same data fitted with k = 3: nothing above the null.  Measured with numpy MU: s_1 = 45.30 against 45.2 .. 46.3."""
    est, Xin = _fit(3)
    est.residual_components(n_vectors=3, X=Xin, n_null=10)
    s, null = est.residual_singular_values_, est.residual_null_
    print(f"k = 3 after {est.n_iter_} iterations: s = {s}, null {null.min():.2f} .. {null.max():.2f}, p {est.residual_pvalue_:.3f}")
    assert est.n_iter_ < 5000 and est.residual_n_significant_ == 0


def test_sharded_estimator(monkeypatch):
    """Two ranks (threads, tests/thread_ranks.py): without a null every rank computes what the unsharded estimator computes from the
    same model; with a null it raises."""
    import torch.distributed as dist
    from thread_ranks import ThreadRank, run_ranks
    monkeypatch.setenv("ESPM_XCHG", "collective")
    # (the one call of est.shard()'s set-up the thread harness does not serve: a thread rank IS its global rank)
    real = dist.get_global_rank
    monkeypatch.setattr(dist, "get_global_rank", lambda group, r: r if isinstance(group, ThreadRank) else real(group, r))

    def body(group, rank):
        est, Xin = _fit(2, group=group)
        out = est.residual_components(n_vectors=2, X=Xin)
        with pytest.raises(NotImplementedError, match="shard"):
            est.residual_components(n_vectors=2, X=Xin, n_null=2)
        return out, est._model_counts()

    from espm_amd import residuals
    res = run_ranks(2, body)
    for out, (D, H) in res:
        want = residuals.svd(_three()["X"], D, H, n_vectors=2)
        assert np.array_equal(out["singular_values"], want["singular_values"]) and np.array_equal(out["maps"], want["maps"])
        assert np.array_equal(out["spectra"], want["spectra"])
    assert np.array_equal(res[0][0]["singular_values"], res[1][0]["singular_values"])


# ---- the wide libraries -----------------------------------------------------------------------------------------------------------------------
def test_the_wide_libraries_have_stubs():
    from espm_amd import _lib
    for k in (12, 20):
        v = _lib.variant(k)
        rc = v.lib.espm_residual_products(None, 0, 0, 8, 8, 8, 0, None, 1, None, None, 1, 1e-14, None, None, None, None, 0, None)
        assert rc == _lib.EUNSUPPORTED and v.lib.espm_residual_products_scratch(1, 96, 1320, 3) == 0
        with pytest.raises(NotImplementedError, match="component library only"):
            v.check(rc)
