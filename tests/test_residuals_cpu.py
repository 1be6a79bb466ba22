"""Residual components without a device: the numpy reference (tests/residuals_reference.py) in the kernel's order and in extended
precision against its own bounds, the subspace iteration of espm_amd.residuals on the reference's products against numpy's SVD, the
scree against hyperspy's Poisson-normalised PCA written out, ``calibrate``, the binding, the argument checks of the entry point that
come before any launch, the wide builds' stubs, and what the module, the estimator and the adapter refuse before anything is uploaded."""
import ctypes as C

import numpy as np
import pytest

from abi_header import CTYPE, _declared
import residuals_reference as rr

SHAPES = [(96, (40, 33), 20, 500), (300, (7, 10), 20, 33), (16, (50, 50), 5, 500)]   # (n, grid, the zero row of D, the zero column of H)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def residuals():
    from espm_amd import residuals
    return residuals


@pytest.fixture(scope="module")
def fixture():
    return rr.three_phase()


def _vectors(g, m, seed=3):
    """Dense signed vectors, the last one all zeros."""
    V = np.random.default_rng(seed).standard_normal((g, m))
    V[-1] = 0.0
    return V


# ---- the reference against its own bounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape,channel,pixel", SHAPES)
@pytest.mark.parametrize("side", ["pixels", "channels"])
def test_reference_in_the_kernels_order_keeps_its_bounds(side, n, shape, channel, pixel):
    """The fp64 reference against the rule evaluated in the kernel's order in extended precision (the exact value, for this purpose) and
    in fp64 (the device's arithmetic less its fused multiply-adds): both within the derived bounds, with the room printed."""
    import marginals_reference as mr
    p = shape[0] * shape[1]
    X = mr.image(n, shape, np.uint16)
    D, H = rr.planted_model(n, p, 3, channel, pixel)
    V = _vectors(3, n if side == "pixels" else p)
    ref = rr.products(X, V, D, H, side)
    e, mag, floored, unmodelled = rr.pearson(X, D, H)
    dead = floored.all(axis=0 if side == "pixels" else 1)   # (a pixel or channel without a model: every entry 0, exactly)
    assert ref["out"].shape == (3, p if side == "pixels" else n) and dead.any() and not ref["out_bound"][2].any()
    assert (ref["out_bound"][:2][:, ~dead] > 0).all() and not ref["out_bound"][:, dead].any() and not ref["out"][:, dead].any()
    assert floored[channel].all() and floored[:, pixel].all() and unmodelled == ref["unmodelled"] > 0 and np.isfinite(e).all()
    assert not e[floored].any() and (np.abs(e) <= mag).all()
    for ft in (np.longdouble, np.float64):
        out, chi2 = rr.in_kernel_order(X, V, D, H, side, ft=ft)
        for name, v in (("out", out), ("chi2", chi2)):
            err = np.abs(v.astype(np.longdouble) - ref[name])
            b = ref[name + "_bound"]
            room = float((err / np.where(b > 0, b, 1)).max())
            print(f"{n} x {p}, {side}, {np.dtype(ft).name}: {name} worst error / bound {room:.3g}")
            assert (err <= b).all(), (name, room)


# ---- the subspace iteration on the reference's products -------------------------------------------------------------------------------------------
def _accept(out, sv, tol):
    """The acceptance the device is held to as well: every returned value within rho_i + 1e-9 s_1 of a true singular value; the values
    numpy finds separated (s_i >= 1.25 s_9) to 10 tol relative."""
    got, rho = out["singular_values"], out["ritz_residuals"]
    for i, (s, r) in enumerate(zip(got, rho)):
        gap = np.abs(sv - s).min()
        print(f"s_{i + 1} = {s:.6f}: rho {r:.3g}, nearest true value {gap:.3g} away, relative error to its own {abs(s - sv[i]) / sv[i]:.3g}")
        assert gap <= r + 1e-9 * sv[0], (i, gap, r)
    separated = [i for i in range(len(got)) if sv[i] >= 1.25 * sv[8]]
    for i in separated:
        assert abs(got[i] - sv[i]) <= 10 * tol * sv[i], i
    return separated


def test_subspace_iteration_against_numpys_svd(residuals, fixture):
    """three_phase against the TRUE two-phase model: s_1 = 433.7 at 3e-16 relative, four separated values, the worst at 2e-11, after 19
    iterations; the leading triplet is the disc and the third spectrum (0.98, 0.997)."""
    X, D, H = fixture["X"], fixture["D"][:, :2], rr.two_phase_H(fixture["H"])
    n, p = X.shape
    e = rr.pearson(X, D, H)[0]
    u, sv, vt = np.linalg.svd(e, full_matrices=False)
    out = residuals._subspace_iteration(rr.make_products(X, D, H), n, p, n_vectors=4, tol=1e-10)
    print(f"{out['n_iter']} iterations, converged {out['converged']}")
    separated = _accept(out, sv, 1e-10)
    assert out["converged"] and out["n_iter"] < 60 and 0 in separated
    assert out["spectra"].shape == (n, 4) and out["maps"].shape == (4, p) and out["chi2_map"].shape == (p,)
    assert np.allclose(out["spectra"].T @ out["spectra"], np.eye(4), atol=1e-12) and np.allclose(out["maps"] @ out["maps"].T, np.eye(4), atol=1e-12)
    # the leading triplet is numpy's, with the sign the module fixes; it is the missing phase
    assert out["spectra"][np.abs(out["spectra"][:, 0]).argmax(), 0] > 0
    assert abs(abs(out["spectra"][:, 0] @ u[:, 0]) - 1) < 1e-9 and abs(abs(out["maps"][0] @ vt[0]) - 1) < 1e-9
    assert out["spectra"][:, 0] @ e @ out["maps"][0] > 0
    assert abs(rr.corr(out["maps"][0], fixture["disc"])) >= 0.8 and abs(rr.corr(out["spectra"][:, 0], fixture["D"][:, 2])) >= 0.8
    assert out["chi2_total"] == pytest.approx((e * e).sum(), rel=1e-12) and out["edge"] == np.sqrt(n) + np.sqrt(p)
    assert np.allclose(out["explained"], out["singular_values"] ** 2 / (e * e).sum(), rtol=1e-12) and out["unmodelled"] == 0
    # with the third phase in the model nothing stands out: the top value is at the edge
    full = residuals._subspace_iteration(rr.make_products(X, fixture["D"], fixture["H"]), n, p, n_vectors=1, tol=1e-8, max_iter=30)
    print(f"three-phase model: s_1 = {full['singular_values'][0]:.3f}, edge {full['edge']:.3f}")
    assert full["singular_values"][0] < 1.05 * full["edge"]


def test_scree_is_the_poisson_normalised_pca(residuals, fixture):
    """E against the independence model: its singular values over sqrt(T) are those of X / sqrt(r c^T) after the trivial 1
    (0.42362, 0.34978 for the two separated ones)."""
    X = fixture["X"]
    n, p = X.shape
    D, H, T = rr.independence(X)
    assert T == float(X.astype(np.int64).sum())
    out = residuals._subspace_iteration(rr.make_products(X, D, H), n, p, n_vectors=6, tol=1e-10)
    x = X.astype(np.float64)
    pca = np.linalg.svd(x / np.sqrt(np.outer(x.sum(axis=1), x.sum(axis=0))), compute_uv=False)
    assert abs(pca[0] - 1.0) <= 1e-12
    sv = np.linalg.svd(rr.pearson(X, D, H)[0], compute_uv=False)
    separated = _accept(out, sv, 1e-10)
    assert separated == [0, 1]   # three phases: two values above the bulk
    for i in separated:
        assert abs(out["singular_values"][i] / np.sqrt(T) - pca[1 + i]) <= 1e-9 * pca[1 + i]


def test_the_start_depends_on_the_seed_alone(residuals):
    a, b, c = residuals.start_block(96, 5), residuals.start_block(96, 5), residuals.start_block(96, 6)
    assert a.shape == (96, 8) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.allclose(a.T @ a, np.eye(8), atol=1e-14)
    assert np.array_equal(a, np.linalg.qr(np.random.default_rng(5).standard_normal((96, 8)))[0])
    assert residuals.start_block(5, 0).shape == (5, 5)


def test_calibrate(residuals):
    null = np.array([45.5, 46.0, 46.3, 45.9])
    out = residuals.calibrate([123.2, 47.0, 46.1, 46.5], null)
    assert out == dict(pvalue=1 / 5, n_significant=2)   # (46.5 is above the null too, but not among the LEADING values)
    assert residuals.calibrate([45.05, 44.0], null) == dict(pvalue=5 / 5, n_significant=0)
    assert residuals.calibrate([46.0], null) == dict(pvalue=3 / 5, n_significant=0)
    assert residuals.calibrate([50.0, 49.0], null) == dict(pvalue=1 / 5, n_significant=2)
    for bad in (([], null), ([1.0], []), ([[1.0]], null), ([np.nan], null), ([1.0], [np.inf])):
        with pytest.raises(ValueError):
            residuals.calibrate(*bad)


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["espm_residual_products", "espm_residual_products_scratch"])
def test_symbols_are_bound_with_the_headers_signatures(lib, name):
    res, args = lib.SYMBOLS[name]
    cres, cargs = _declared(name)
    assert res is CTYPE[cres]
    assert list(args) == [CTYPE[a] for a in cargs]
    for handle in (lib.lib, lib.variant(12).lib, lib.variant(20).lib):
        assert hasattr(handle, name)


def test_header_carries_the_sizes(lib, residuals):
    from espm_amd import _abi
    d = _abi.parse_defines(_abi.header_text())
    assert d["ESPM_RESID_MAX_G"] == lib.RESID_MAX_G == residuals.MAX_G == rr.MAX_G == residuals.BLOCK == 8
    assert d["ESPM_RESID_MAX_K"] == lib.RESID_MAX_K == residuals.MAX_K == rr.MAX_K == lib.DIAG_MAX_K
    assert d["ESPM_RESID_PCHUNK"] == lib.RESID_PCHUNK == rr.PCHUNK == lib.MARG_PCHUNK == 2048 and lib.RESID_BLOCK == 256
    assert (lib.RESID_PIXELS, lib.RESID_CHANNELS) == (0, 1)


U8, CM, PM, PIX, CHAN = 0, 0, 1, 0, 1


def _vp(v):
    return None if v is None else C.c_void_p(v)   # (never dereferenced: every call below is refused on the host)


def _call(f, x=8, dtype=U8, layout=CM, ld=80, n=8, p=80, side=PIX, vec=8, g=3, d=8, h=8, k=3, log_shift=1e-14, out=8, chi2=8, unmodelled=8,
          scratch=8, scratch_bytes=1 << 20):
    return f(_vp(x), dtype, layout, ld, n, p, side, _vp(vec), g, _vp(d), _vp(h), k, log_shift, _vp(out), _vp(chi2), _vp(unmodelled),
             _vp(scratch), scratch_bytes, None)


def test_argument_errors_need_no_device(lib):
    f, err = lib.lib.espm_residual_products, lib.lib.espm_mu_last_error
    for side in (PIX, CHAN):
        for name in ("x", "vec", "d", "h", "out"):
            assert _call(f, side=side, **{name: None}) == lib.EINVAL and b"bad arguments" in err(), name
    assert _call(f, side=CHAN, scratch=None) == lib.EINVAL and b"scratch" in err()
    assert _call(f, side=2) == lib.EINVAL and b"side 2" in err()
    assert _call(f, side=-1) == lib.EINVAL and b"side -1" in err()
    assert _call(f, layout=2) == lib.EINVAL and b"x_layout 2" in err()
    assert _call(f, dtype=4) == lib.EINVAL and b"x_dtype 4" in err()
    assert _call(f, dtype=-1) == lib.EINVAL
    assert _call(f, g=0) == lib.EINVAL and b"g=0" in err()
    assert _call(f, g=9) == lib.EINVAL and b"g=9" in err()
    assert _call(f, k=0) == lib.EINVAL and b"k=0" in err()   # a model is required
    assert _call(f, k=9) == lib.EINVAL and b"k=9" in err()
    assert _call(f, n=0) == lib.EINVAL and b"n=0" in err()
    assert _call(f, p=0) == lib.EINVAL and b"p=0" in err()
    assert _call(f, ld=79) == lib.EINVAL and b"ld=79" in err()
    assert _call(f, layout=PM, ld=7) == lib.EINVAL and b"ld=7" in err()      # pixel-major: rows of n
    assert _call(f, log_shift=0.0) == lib.EINVAL and b"log_shift=0" in err()
    assert _call(f, log_shift=-1.0) == lib.EINVAL and _call(f, log_shift=float("nan")) == lib.EINVAL
    # the scratch: chunks x (g + 1) x n doubles on the channel side, nothing on the pixel side
    q = lib.lib.espm_residual_products_scratch
    assert q(CHAN, 8, 80, 3) == 1 * 4 * 8 * 8 and q(CHAN, 16, 2500, 8) == 2 * 9 * 16 * 8 and q(CHAN, 2048, 512 * 512, 8) == 128 * 9 * 2048 * 8
    assert q(PIX, 8, 80, 3) == q(2, 8, 80, 3) == q(CHAN, 0, 80, 3) == q(CHAN, 8, 0, 3) == q(CHAN, 8, 80, 0) == q(CHAN, 8, 80, 9) == 0
    assert _call(f, side=CHAN, scratch_bytes=q(CHAN, 8, 80, 3) - 1) == lib.EINVAL and b"255 bytes, 256 needed" in err()
    assert _call(f, side=CHAN, n=65535 * 256 + 1, p=1, ld=1) == lib.EINVAL and b"n=16776961" in err()


def test_the_wide_builds_export_stubs(lib):
    for k in (12, 20):
        v = lib.variant(k)
        rc = v.lib.espm_residual_products(None, 0, 0, 8, 8, 8, 0, None, 1, None, None, 1, 1e-14, None, None, None, None, 0, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)
        assert v.lib.espm_residual_products_scratch(1, 96, 1320, 3) == 0 and lib.lib.espm_residual_products_scratch(1, 96, 1320, 3) > 0


# ---- the Python module, the estimator and the adapter, before the device ---------------------------------------------------------------------
def test_module_raises_before_upload(lib, residuals, monkeypatch):
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    monkeypatch.setattr(_image, "model_on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.zeros((6, 20), np.uint8)
    D, H = np.ones((6, 2)), np.ones((2, 20))
    Vn, Vp = np.ones((2, 6)), np.ones((2, 20))
    for side, V, other in (("pixels", Vn, Vp), ("channels", Vp, Vn)):
        def call(X=X, V=V, D=D, H=H, **kw):
            return residuals.products(X, V, D, H, side=side, **kw)
        with pytest.raises(ValueError, match="layout"):
            call(layout="rows")
        with pytest.raises(ValueError, match="2-D"):
            call(X=np.zeros(6, np.uint8))
        with pytest.raises(ValueError, match="vectors of shape"):
            call(V=other)
        with pytest.raises(ValueError, match="vectors of shape"):
            call(V=np.ones((2, 3, 4)))
        with pytest.raises(ValueError, match="not finite"):
            call(V=np.where(np.arange(V.size).reshape(V.shape) == 3, np.nan, V))
        with pytest.raises(ValueError, match="not finite"):
            call(X=np.where(np.arange(120).reshape(6, 20) == 7, np.inf, 0.0))
        with pytest.raises(ValueError, match="not finite"):
            call(D=np.where(np.arange(12).reshape(6, 2) == 7, np.nan, D))
        with pytest.raises(ValueError, match="from -1 to 0"):
            call(X=X.astype(np.int32) - (np.arange(120).reshape(6, 20) == 7))
        with pytest.raises(ValueError, match="model"):
            call(H=None)
        with pytest.raises(ValueError, match="channels"):
            call(D=np.ones((5, 2)))
        with pytest.raises(ValueError, match="pixels"):
            call(H=np.ones((2, 19)))
        with pytest.raises(ValueError, match="log_shift"):
            call(log_shift=0)
        with pytest.raises(NotImplementedError, match="9 components"):
            call(D=np.ones((6, 9)), H=np.ones((9, 20)))
    with pytest.raises(ValueError, match="side"):
        residuals.products(X, Vn, D, H, side="rows")
    for bad in (0, 7, 2.5, True):
        with pytest.raises(ValueError, match="n_vectors"):
            residuals.svd(X, D, H, n_vectors=bad)
        with pytest.raises(ValueError, match="n_vectors"):
            residuals.scree(X, n_vectors=bad)
    with pytest.raises(ValueError, match="tol"):
        residuals.svd(X, D, H, tol=0)
    with pytest.raises(ValueError, match="max_iter"):
        residuals.svd(X, D, H, max_iter=0)
    with pytest.raises(NotImplementedError, match="9 components"):
        residuals.svd(X, np.ones((6, 9)), np.ones((9, 20)))
    with pytest.raises(ValueError, match="layout"):
        residuals.scree(X, layout="rows")
    with pytest.raises(ValueError, match="layout"):
        residuals.independence_model(X, layout="rows")
    with pytest.raises(NotImplementedError, match="9 components"):
        residuals.null_singular_values(np.ones((6, 9)), np.ones((9, 20)))
    with pytest.raises(ValueError, match="negative"):
        residuals.null_singular_values(-D, H)
    with pytest.raises(ValueError, match="n_rep"):
        residuals.null_singular_values(D, H, n_rep=0)
    with pytest.raises(ValueError, match="seed"):
        residuals.null_singular_values(D, H, seed=-1)
    with pytest.raises(ValueError, match="log_shift"):
        residuals.null_singular_values(D, H, log_shift=0)


def test_no_cpu_fallback(lib, residuals, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X = np.zeros((6, 20), np.uint8)
    D, H = np.ones((6, 2)), np.ones((2, 20))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        residuals.products(X, np.ones((1, 6)), D, H)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        residuals.svd(X, D, H)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        residuals.scree(X)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        residuals.null_singular_values(D, H)


def _fitted(**kw):
    """An estimator with the attributes of a fit (the fit itself needs the device)."""
    from espm_amd.estimators import SmoothNMF
    args = dict(n_components=3, shape_2d=(4, 5), max_iter=5, verbose=0)
    args.update(kw)
    est = SmoothNMF(**args)
    k = args["n_components"]
    est.G_, est.W_, est.H_, est._identity_G = np.eye(6), np.ones((6, k)), np.ones((k, 20)) / k, True
    est.X_ = np.ones((6, 20))
    return est


def test_estimator_refuses_before_any_upload(lib, residuals, monkeypatch):
    from sklearn.exceptions import NotFittedError

    from espm_amd.estimators import SmoothNMF
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    monkeypatch.setattr(_image, "model_on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.ones((6, 20), np.uint8)
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=3, verbose=0).residual_components(X=X)
    with pytest.raises(ValueError, match="X has 5 channels"):
        _fitted().residual_components(X=X[:5])
    with pytest.raises(ValueError, match="X has 19 pixels"):
        _fitted().residual_components(X=X[:, :19])
    with pytest.raises(ValueError, match="X has 20 channels"):
        _fitted(hspy_comp=True).residual_components(X=X)
    binned = _fitted()
    binned.bin_ = (2, 2)
    with pytest.raises(ValueError, match="fit_binned"):
        binned.residual_components()
    with pytest.raises(ValueError, match="fit_binned"):
        binned.residual_components(X=X, n_null=3)
    with pytest.raises(ValueError, match="n_vectors"):
        _fitted().residual_components(n_vectors=7, X=X)
    with pytest.raises(ValueError, match="n_null"):
        _fitted().residual_components(X=X, n_null=-1)
    with pytest.raises(NotImplementedError, match="9 components"):
        _fitted(n_components=9).residual_components(X=X)
    sharded = _fitted()
    sharded._shard_group = object()
    with pytest.raises(NotImplementedError, match="shard"):
        sharded.residual_components(X=X, n_null=2)
    est = _fitted()
    for name in ("residual_singular_values_", "residual_maps_", "residual_null_"):
        assert not hasattr(est, name)


def test_adapter_needs_the_analysis_first(lib):
    from espm_amd import hyperspy_adapter as ha
    est = _fitted()
    with pytest.raises(AttributeError, match=r"call est.residual_components\(\) first"):
        ha.residual_components(est)
    est.residual_maps_, est.residual_spectra_ = np.arange(40.0).reshape(2, 20), np.arange(12.0).reshape(6, 2)
    maps, spectra = ha.residual_components(est)
    assert maps.shape == (2, 4, 5) and spectra.shape == (2, 6)
    assert np.array_equal(maps.reshape(2, 20), est.residual_maps_) and np.array_equal(spectra, est.residual_spectra_.T)
    assert ha.residual_components(est, shape_2d=(2, 10))[0].shape == (2, 2, 10)
