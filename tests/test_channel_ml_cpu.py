"""Channel ML without a device (espm_amd/channel_ml.py, NMFEstimator.spectrum_presence / spectrum_intervals): the refusals that come
before the upload, ``line_presence`` against its closed form, the signatures, the header block of espm_channel_ml_step as both readers
of include/espm_mu.h see it, and what tests/test_gpu_channel_ml.py rests on - the numpy definition (tests/channel_ml_reference.py)
converges on every channel of every case within half of the caps the GPU tests pass."""
import ctypes as C
import inspect

import numpy as np
import pytest

import abi_header
import channel_ml_reference as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def cml(lib):
    from espm_amd import channel_ml
    return channel_ml


@pytest.fixture
def no_upload(lib, monkeypatch):
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    monkeypatch.setattr(_image, "model_on_device", lambda *a, **k: pytest.fail("the upload was reached"))


# ---- refusals before the upload -----------------------------------------------------------------------------------------------------------
def test_refusals_before_the_upload(cml, no_upload):
    X, H = np.zeros((6, 10), np.uint8), np.ones((2, 10))
    calls = (cml.ml_channels, cml.presence, cml.intervals, lambda X, H, **kw: cml.ml_channels_pinned(X, H, 0, 1.0, **kw))
    for f in calls:
        with pytest.raises(ValueError, match="layout"):
            f(X, H, layout="rows")
        with pytest.raises(ValueError, match="pixels"):
            f(X, np.ones((2, 9)))
        with pytest.raises(ValueError, match="pixels"):
            f(X, H, layout="pm")                    # (6, 10) read as (pixels, channels)
        with pytest.raises(ValueError, match="2-D"):
            f(np.zeros(6), H)
        with pytest.raises(ValueError, match="not empty"):
            f(X, np.ones(10))
        with pytest.raises(NotImplementedError, match="9 components"):
            f(X, np.ones((9, 10)))
        with pytest.raises(ValueError, match="tol"):
            f(X, H, tol=0.0)
        with pytest.raises(ValueError, match="log_shift"):
            f(X, H, log_shift=0.0)
        with pytest.raises(ValueError, match="max_pass"):
            f(X, H, max_pass=0)
        with pytest.raises(ValueError, match="chunk"):
            f(X, H, chunk=1.5)
        with pytest.raises(ValueError, match="finite and not negative"):
            f(X, -H)
        with pytest.raises(ValueError, match="finite and not negative"):
            f(X, np.where(np.arange(20).reshape(2, 10) == 3, np.nan, 1.0))
        with pytest.raises(ValueError, match="D0 of shape"):
            f(X, H, D0=np.ones((6, 3)))
        with pytest.raises(ValueError, match="D0 holds values"):
            f(X, H, D0=np.full((6, 2), np.inf))
        with pytest.raises(ValueError, match="not finite"):
            f(np.full((6, 10), np.nan), H)
        with pytest.raises(ValueError, match="all zero"):
            f(X, np.stack([np.ones(10), np.zeros(10)]))
    for f in (cml.ml_channels, cml.intervals):
        with pytest.raises(ValueError, match="components"):
            f(X, H, components=[2])
        with pytest.raises(ValueError, match="components"):
            f(X, H, components=[0, 0])
    with pytest.raises(ValueError, match="one component"):
        cml.presence(X, np.ones((1, 10)))
    for level in (0.0, 1.0, -0.5, True):
        with pytest.raises(ValueError, match="level"):
            cml.intervals(X, H, level=level)
    with pytest.raises(ValueError, match="lr_tol"):
        cml.intervals(X, H, lr_tol=0.0)
    with pytest.raises(ValueError, match="max_eval"):
        cml.intervals(X, H, max_eval=0)
    for pin in (2, -1, 0.5, True):
        with pytest.raises(ValueError, match="pin must be"):
            cml.ml_channels_pinned(X, H, pin, 1.0)
    with pytest.raises(ValueError, match="held, not fitted"):
        cml.ml_channels_pinned(X, H, 0, 1.0, components=[0, 1])
    with pytest.raises(ValueError, match="scalar or of shape"):
        cml.ml_channels_pinned(X, H, 0, np.ones(5))


def _fitted(k=3, G=None, **kw):
    from espm_amd.estimators import SmoothNMF
    n, p = 12, 20
    rng = np.random.default_rng(7)
    est = SmoothNMF(n_components=k, shape_2d=(4, 5), max_iter=5, verbose=0, **kw)
    m = n if G is None else G.shape[1]
    est.G_, est._identity_G = (np.eye(n) if G is None else G), G is None
    est.W_, est.H_ = rng.uniform(0.5, 2.0, (m, k)), rng.uniform(0.1, 1.0, (k, p))
    est.X_, est.norm_factor_ = rng.poisson(2.0, (n, p)).astype(np.float64), 1.0
    return est


def test_estimator_refusals_before_the_upload(cml, no_upload):
    est = _fitted()
    bad = np.ones(12)
    for call in (est.spectrum_presence, est.spectrum_intervals):
        with pytest.raises(ValueError, match="X must be 2-D"):
            call(X=bad)
    wide = _fitted(k=9)
    with pytest.raises(NotImplementedError, match="spectrum_presence: 9 components"):
        wide.spectrum_presence()
    with pytest.raises(NotImplementedError, match="spectrum_intervals: 9 components"):
        wide.spectrum_intervals()
    sharded = _fitted()
    sharded._shard_group = object()
    with pytest.raises(NotImplementedError, match=r"spectrum_presence does not cover shard\(\)"):
        sharded.spectrum_presence()
    with pytest.raises(NotImplementedError, match=r"spectrum_intervals does not cover shard\(\)"):
        sharded.spectrum_intervals()
    binned = _fitted()
    binned.bin_ = (2, 2)
    for name in ("spectrum_presence", "spectrum_intervals"):
        with pytest.raises(ValueError, match=name + ": this estimator was fitted by fit_binned"):
            getattr(binned, name)()
    with pytest.raises(ValueError, match="one component"):
        _fitted(k=1).spectrum_presence()
    with pytest.raises(ValueError, match="window 0"):
        est.spectrum_presence(windows=[(3, 40)])
    with pytest.raises(ValueError, match="level"):
        est.spectrum_intervals(level=1.0)
    with pytest.raises(ValueError, match="components"):
        est.spectrum_intervals(components=[5])
    # the dictionary-bound analyses keep refusing an identity G, in the words they had
    with pytest.raises(NotImplementedError, match="element_presence: needs a dictionary or physics model G"):
        est.element_presence()
    with pytest.raises(NotImplementedError, match="concentration_intervals: needs a dictionary or physics model G"):
        est.concentration_intervals()
    from espm_amd import spectra_ml
    with pytest.raises(NotImplementedError, match="without one the problem decouples per channel"):
        spectra_ml.ml_spectra(np.zeros((6, 10), np.uint8), None, np.ones((2, 10)))


def test_adapter_needs_the_tables(cml):
    from espm_amd import hyperspy_adapter
    est = _fitted()
    with pytest.raises(AttributeError, match="spectrum_intervals"):
        hyperspy_adapter.spectrum_bands(est)
    est.D_ml_ = np.arange(36.0).reshape(12, 3)
    est.D_lower_, est.D_upper_, est.D_interval_level_ = est.D_ml_ - 1.0, est.D_ml_ + 1.0, 0.9
    out = hyperspy_adapter.spectrum_bands(est)
    assert set(out) == {"D_ml", "lower", "upper", "level"} and out["upper"].shape == (3, 12) and np.array_equal(out["D_ml"], est.D_ml_.T)
    est.D_presence_lr_, est.D_presence_pvalue_, est.D_excess_deviance_ = est.D_ml_, est.D_ml_, np.zeros(12)
    out = hyperspy_adapter.spectrum_bands(est)
    assert out["lr"].shape == (3, 12) and out["excess_deviance"].shape == (12,)


# ---- line_presence ------------------------------------------------------------------------------------------------------------------------
def test_line_presence_against_the_closed_form(cml):
    from scipy.stats import chi2
    rng = np.random.default_rng(0)
    lr = rng.gamma(1.0, 2.0, (30, 3)) * (rng.random((30, 3)) < 0.6)
    lr[10:14, 1] = 0.0
    windows = [(0, 1), (2, 7), (10, 14), (0, 30), (12, 25)]
    out = cml.line_presence(lr, windows)
    assert out["lr"].shape == out["pvalue"].shape == (5, 3) and list(out["width"]) == [1, 5, 4, 30, 13]
    from math import comb
    for g, (lo, hi) in enumerate(windows):
        w = hi - lo
        for j in range(3):
            total = lr[lo:hi, j].sum()
            assert out["lr"][g, j] == pytest.approx(total, rel=1e-15)
            want = 1.0 if total == 0 else sum(comb(w, i) * 0.5 ** w * chi2.sf(total, i) for i in range(1, w + 1))
            assert out["pvalue"][g, j] == pytest.approx(want, rel=1e-12, abs=1e-300)
    assert out["pvalue"][2, 1] == 1.0 and out["lr"][2, 1] == 0.0
    assert ((out["pvalue"] > 0) & (out["pvalue"] <= 1)).all()


def test_line_presence_of_one_channel_is_the_channel_pvalue(cml):
    rng = np.random.default_rng(1)
    lr = rng.gamma(1.0, 3.0, (17, 2))
    lr[3] = 0.0
    out = cml.line_presence(lr, [(c, c + 1) for c in range(17)])
    assert np.array_equal(out["lr"], lr)
    assert np.array_equal(out["pvalue"], cml.pvalue(lr))
    assert (out["pvalue"][3] == 1.0).all()


def test_line_presence_refusals(cml):
    lr = np.ones((8, 2))
    with pytest.raises(ValueError, match="channels, components"):
        cml.line_presence(np.ones(8), [(0, 2)])
    with pytest.raises(ValueError, match="finite and not negative"):
        cml.line_presence(-lr, [(0, 2)])
    with pytest.raises(ValueError, match="finite and not negative"):
        cml.line_presence(lr * np.nan, [(0, 2)])
    with pytest.raises(ValueError, match="window 0"):
        cml.line_presence(lr, [(0, 9)])
    with pytest.raises(ValueError, match="no window"):
        cml.line_presence(lr, [])


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
SIGNATURES = {
    "ml_channels": "(X, H, D0=None, components=None, tol=0.001, max_pass=128, chunk=4, log_shift=1e-14, layout='cm', device=None)",
    "presence": "(X, H, D0=None, tol=0.001, max_pass=128, chunk=4, log_shift=1e-14, layout='cm', device=None)",
    "line_presence": "(lr, windows)",
    "ml_channels_pinned": "(X, H, pin, t, D0=None, components=None, tol=0.001, max_pass=128, chunk=4, log_shift=1e-14, layout='cm', "
                          "device=None)",
    "intervals": "(X, H, D0=None, level=0.95, components=None, tol=0.001, lr_tol=0.01, max_eval=64, max_pass=128, chunk=4, "
                 "log_shift=1e-14, layout='cm', device=None)",
}
METHODS = {
    "spectrum_presence": "(self, X=None, windows=None, tol=0.001, max_pass=None)",
    "spectrum_intervals": "(self, level=0.95, X=None, components=None, tol=0.001, lr_tol=0.01, max_eval=None, max_pass=None)",
}


def test_signatures(cml):
    from espm_amd import hyperspy_adapter
    from espm_amd.estimators import SmoothNMF
    for name, sig in SIGNATURES.items():
        assert str(inspect.signature(getattr(cml, name))) == sig, name
        assert getattr(cml, name).__doc__, name
    for name, sig in METHODS.items():
        assert str(inspect.signature(getattr(SmoothNMF, name))) == sig, name
        assert getattr(SmoothNMF, name).__doc__, name
    assert str(inspect.signature(hyperspy_adapter.spectrum_bands)) == "(est)"
    assert cml.MAX_K == 8
    for word in ("simplex_W", "mu", "uncertainty of H", "more than 8 components", "more than one GPU", "unmodelled"):
        assert word in cml.__doc__, word


def test_no_torch_at_import(cml):
    import re
    assert not re.search(r"^(import|from) torch", inspect.getsource(cml), flags=re.M)   # (torch is imported where it is used)


def test_header_block(lib):
    name = "espm_channel_ml_step"
    assert name in abi_header.declared_functions() and name in lib.SYMBOLS
    res, args = abi_header.signature(name, C.c_void_p)
    assert (res, args) == lib.SYMBOLS[name] and res is C.c_int and len(args) == 24
    assert args[:4] == [C.c_int] * 4 and args[9] is C.c_uint32 and args[12] is C.c_double and args[15] is C.c_size_t
    assert lib.CML_STATE_EXTRA == 3
    fn = getattr(lib.lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    # the wide builds export the entry point as a stub
    wide = lib.variant(9).lib
    assert getattr(wide, name)(*([0] * 4 + [None] * 5 + [0] + [None] * 2 + [0.0] + [None] * 2 + [0] + [None] * 8)) == lib.EUNSUPPORTED


# ---- what the GPU tests rest on: the definition converges everywhere, within half of the caps ---------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_cases_are_what_they_are_meant_to_be(name):
    X, H, D = R.case(name)
    c = R.CASES[name]
    assert X.shape == (c["n"], c["p"]) and H.shape == (c["k"], c["p"]) and X.dtype == np.uint8
    N = X.sum(axis=1)
    assert sorted(np.flatnonzero(N == 0)) == sorted(c["rows"])          # exactly the planted empty channels
    for lo, hi, j in c["holes"]:
        assert (D[lo:hi, j] == 0).all()
    if c["k"] > 1:
        assert 0.4 < (H[1] == 0).mean() < 0.6 and (H.sum(axis=1) > 0).all()
    if name == "B":
        from espm_amd import _abi
        d = _abi.parse_defines(_abi.header_text())
        assert -(-c["n"] // d["ESPM_CDIAG_BLOCK"]) == 2 and -(-c["p"] // d["ESPM_CDIAG_PCHUNK"]) == 2


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_full_and_nested_fits_converge(name):
    X, H, _ = R.case(name)
    full = R.ml_channels(X, H)
    assert full["converged"].all() and full["n_pass"].max() <= 9 and (full["gap"] <= 1e-3).all()
    opt = R.optimum(name)
    excess = full["deviance"] - opt["deviance"]
    assert (excess <= 1e-3 + 1e-9 * np.maximum(1.0, opt["deviance"])).all() and (excess >= -1e-9 * np.maximum(1.0, opt["deviance"])).all()
    empty = full["N"] == 0
    assert (full["D"][empty] == 0).all() and (full["deviance"][empty] == 0).all() and (full["n_pass"][empty] == 0).all()
    if H.shape[0] == 1:
        return
    nested = R.solved(name)
    free = R.presence_free(X, H)
    # the reduced fits by either rule: the free-scale one within 30 passes; the pinned one at t = 0 - what the device batches - needs
    # more (no scale onto the ray) and stays within half of the cap
    assert free["converged"].all() and free["n_pass"][1:].max() <= 30
    assert nested["converged"].all() and nested["n_pass"][1:].max() <= R.MAX_PASS // 2
    assert np.abs(nested["lr"] - free["lr"]).max() <= 2e-3                  # two certified minima each: within 2 tol
    assert (nested["lr"][nested["D_ml"] == 0] == 0).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_intervals_converge(name):
    X, H, _ = R.case(name)
    iv = R.solved_intervals(name)
    assert iv["converged"].all()
    assert iv["n_eval"].max() <= 8 and iv["max_fit_pass"] <= 21 and iv["n_pass"].max() <= 38
    assert iv["n_eval"].max() <= R.MAX_EVAL // 2 and iv["max_fit_pass"] <= R.MAX_PASS // 2
    assert (iv["lower"] <= iv["D_ml"]).all() and (iv["D_ml"] <= iv["upper"]).all()
    assert (iv["lower"][iv["D_ml"] == 0] == 0).all()


def test_planted_holes_have_the_smallest_lr_of_their_column():
    X, H, D = R.case("A")
    lr = R.solved("A")["lr"]
    live = X.sum(axis=1) > 0
    for lo, hi, j in R.CASES["A"]["holes"]:
        rest = np.setdiff1d(np.flatnonzero(live), np.arange(lo, hi))
        assert lr[lo:hi, j].max() <= lr[rest, j].min()
