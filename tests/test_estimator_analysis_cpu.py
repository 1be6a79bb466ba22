"""The set-up the estimator's post-fit methods share (espm_amd/estimators/analysis.py) and the surface they keep, without a device:
``_image_argument``, ``_model_counts``, the attribute tuples, the signatures of the nine public methods, ``clone`` and pickling.  The
estimator is "fitted" by hand (the fit itself needs the device): 6 channels, 20 pixels, 2 components."""
import inspect
import pickle

import numpy as np
import pytest

N, P, K = 6, 20, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


def _fitted(G=None, **kw):
    from espm_amd.estimators import SmoothNMF
    rng = np.random.default_rng(5)
    est = SmoothNMF(n_components=K, shape_2d=(4, 5), max_iter=5, verbose=0, **kw)
    m = N if G is None else G.shape[1]
    est.G_, est._identity_G = (np.eye(N) if G is None else G), G is None
    est.W_, est.H_ = rng.uniform(0.5, 2.0, (m, K)), rng.uniform(0.1, 1.0, (K, P))
    est.X_, est.norm_factor_ = rng.uniform(0.0, 4.0, (N, P)), 0.25
    return est


# ---- _image_argument -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hspy_comp", [False, True])
def test_image_argument_none_is_the_unscaled_fitted_image(lib, hspy_comp):
    est = _fitted(hspy_comp=hspy_comp)   # (X_ is channel-major whatever hspy_comp is)
    X, layout = est._image_argument(None, "pixel_diagnostics")
    assert layout == "cm" and np.array_equal(X, est.X_)
    est = _fitted(normalize=True, hspy_comp=hspy_comp)
    X, layout = est._image_argument(None, "pixel_diagnostics")
    assert layout == "cm" and np.array_equal(X, est.X_ / est.norm_factor_) and X.shape == (N, P)


def test_image_argument_none_needs_a_fitted_image(lib):
    from sklearn.exceptions import NotFittedError
    est = _fitted()
    del est.X_
    with pytest.raises(NotFittedError):
        est._image_argument(None, "pixel_diagnostics")


@pytest.mark.parametrize("who", ["pixel_diagnostics", "spectral_diagnostics", "attribute_counts"])
def test_image_argument_none_is_refused_after_fit_binned(lib, who):
    est = _fitted()
    est.bin_ = (2, 2)
    with pytest.raises(ValueError) as e:
        est._image_argument(None, who)
    assert str(e.value) == (f"{who}: this estimator was fitted by fit_binned with bin (2, 2): X_ holds the binned image, "
                            "H_ the full-resolution pixels - pass the full-resolution X")
    X = np.ones((N, P), np.uint8)
    assert est._image_argument(X, who)[0] is X   # (a given X is what fit_binned's estimator asks for)


@pytest.mark.parametrize("hspy_comp", [False, True])
def test_image_argument_given(lib, hspy_comp):
    est = _fitted(hspy_comp=hspy_comp)
    shape = (lambda n, p: (p, n)) if hspy_comp else (lambda n, p: (n, p))
    good = np.ones(shape(N, P), np.uint8)
    X, layout = est._image_argument(good, "attribute_counts")
    assert X is good and layout == ("pm" if hspy_comp else "cm")
    X, layout = est._image_argument(good.tolist(), "attribute_counts")   # (anything numpy reads as 2-D)
    assert isinstance(X, np.ndarray) and X.shape == good.shape and layout == ("pm" if hspy_comp else "cm")
    for bad in (np.ones(N), np.ones((N, 4, 5))):
        with pytest.raises(ValueError) as e:
            est._image_argument(bad, "attribute_counts")
        assert str(e.value) == "X must be 2-D"
    with pytest.raises(ValueError) as e:
        est._image_argument(np.ones(shape(N + 1, P)), "attribute_counts")
    assert str(e.value) == f"X has {N + 1} channels, the fitted G_ has {N}"
    with pytest.raises(ValueError) as e:
        est._image_argument(np.ones(shape(N, P - 1)), "attribute_counts")
    assert str(e.value) == f"X has {P - 1} pixels, the fitted H_ has {P}"
    if N != P:   # (read the other way round, the good image has the wrong channel count)
        with pytest.raises(ValueError, match=f"X has {P} channels"):
            est._image_argument(good.T, "attribute_counts")


def test_callers_keep_their_own_refusals_in_front(lib, monkeypatch):
    """The component limit and the fixed_W refusal come before X is looked at; X before the device modules are called."""
    from espm_amd import attribution, measures
    from espm_amd.estimators import SmoothNMF
    for mod, name in ((measures, "pixel_diagnostics"), (measures, "spectral_diagnostics"), (attribution, "expected")):
        monkeypatch.setattr(mod, name, lambda *a, **k: pytest.fail("the device module was reached"))
    bad = np.ones(N)
    est = _fitted()
    for call in (est.pixel_diagnostics, est.spectral_diagnostics, est.attribute_counts):
        with pytest.raises(ValueError, match="X must be 2-D"):
            call(bad)
    wide = SmoothNMF(n_components=9, verbose=0)
    wide.G_, wide.W_, wide.H_, wide._identity_G = np.eye(N), np.ones((N, 9)), np.ones((9, P)), True
    with pytest.raises(NotImplementedError, match="pixel_diagnostics: 9 components"):
        wide.pixel_diagnostics(bad)
    with pytest.raises(NotImplementedError, match="spectral_diagnostics: 9 components"):
        wide.spectral_diagnostics(bad)
    held = _fitted(fixed_W=np.where(np.arange(N * K).reshape(N, K) == 0, 1.0, -1.0))
    with pytest.raises(NotImplementedError, match="imposed fixed_W"):
        held.spectral_diagnostics(bad)
    binned = _fitted()
    binned.bin_ = (2, 2)
    for name in ("pixel_diagnostics", "spectral_diagnostics", "attribute_counts"):
        with pytest.raises(ValueError, match=name + ": this estimator was fitted by fit_binned"):
            getattr(binned, name)()


# ---- the model in counts -------------------------------------------------------------------------------------------------------------
def test_model_counts(lib):
    est = _fitted()
    est.W_, est.H_ = est.W_.astype(np.float32), est.H_.astype(np.float32)
    D, H = est._model_counts()
    assert D.dtype == H.dtype == np.float64 and np.array_equal(D, est.W_) and np.array_equal(H, est.H_)
    assert D.shape == (N, K) and H.shape == (K, P)
    G = np.random.default_rng(2).uniform(0.0, 1.0, (N, 4))
    est = _fitted(G=G)
    D, H = est._model_counts()
    assert D.dtype == H.dtype == np.float64 and np.array_equal(D, G @ est.W_) and np.array_equal(H, est.H_) and D.shape == (N, K)
    Gf, Wf, Hf = est._model_factors()
    assert all(a.dtype == np.float64 for a in (Gf, Wf, Hf)) and np.array_equal(Gf, G) and np.array_equal(Wf, est.W_) and np.array_equal(Hf, H)
    assert _fitted()._model_factors()[0] is None   # (an identity G is not multiplied out)


def test_layout_and_counts_for_fit(lib):
    assert _fitted()._layout() == "cm" and _fitted(hspy_comp=True)._layout() == "pm"
    counts = np.array([[0, 1], [255, 65535]], np.uint16)
    est = _fitted()
    assert est._counts_for_fit(counts).dtype == np.float32 and np.array_equal(est._counts_for_fit(counts), counts)
    est.set_precision("fp64")
    assert est._counts_for_fit(counts).dtype == np.float64 and np.array_equal(est._counts_for_fit(counts), counts)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
SIGNATURES = {
    "fit_binned": "(self, X, bin, y=None, W=None)",
    "fit_split": "(self, X, q=0.8, seed=0, y=None, W=None, H=None)",
    "pixel_diagnostics": "(self, X=None)",
    "spectral_diagnostics": "(self, X=None)",
    "attribute_counts": "(self, X=None)",
    "assign_counts": "(self, X, seed=0, device=False)",
    "simulate": "(self, seed=0, replicate=0, device=False)",
    "calibrate_deviance": "(self, X=None, n_rep=100, seed=0)",
    "bootstrap": "(self, n_boot=20, seed=0, max_iter=None, return_samples=False)",
}


def test_signatures_and_where_the_names_are_reached(lib):
    from espm_amd.estimators import NMFEstimator, SmoothNMF, analysis, base
    for name, sig in SIGNATURES.items():
        assert str(inspect.signature(getattr(SmoothNMF, name))) == sig, name
        assert getattr(SmoothNMF, name).__doc__, name
    mro = NMFEstimator.__mro__
    names = [c.__name__ for c in mro]
    assert names.index("_PixelTransform") < mro.index(analysis._FitAnalysis) < names.index("TransformerMixin")
    assert "__init__" not in vars(analysis._FitAnalysis)
    for name in ("_split_refusal", "_fit_split_stages", "_bootstrap_copy", "_bootstrap_start", "_refuse_binned_X", "_sampling_model"):
        assert callable(getattr(_fitted(), name)), name
    assert "_make_engine" in vars(base.NMFEstimator) and "_transform_refusal" in vars(base.NMFEstimator)


def test_attribute_tuples(lib):
    est = _fitted()
    assert est._SPLIT_ATTRIBUTES == ("split_q_", "split_seed_", "heldout_deviance_", "train_deviance_", "heldout_deviance_map_",
                                     "train_deviance_map_", "heldout_counts_")
    assert est._BINNED_ATTRIBUTES == ("bin_", "binned_shape_2d_", "W_binned_", "H_binned_")


def test_a_plain_fit_forgets_fit_binned_and_the_split(lib, monkeypatch):
    est = _fitted()
    for name in est._BINNED_ATTRIBUTES + est._SPLIT_ATTRIBUTES:
        setattr(est, name, 1.0)

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop

    monkeypatch.setattr(type(est), "_fit_validate", stop)
    with pytest.raises(Stop):
        est.fit_transform(np.ones((N, P)))
    assert not any(hasattr(est, name) for name in est._BINNED_ATTRIBUTES + est._SPLIT_ATTRIBUTES)
    assert hasattr(est, "W_")   # (the names of the two tuples are all that is cleared ahead of the stages)


def test_clone_and_pickle(lib):
    from sklearn.base import clone
    est = _fitted(normalize=True, hspy_comp=True, mu=0.3, lambda_L=2.0)
    twin = clone(est)
    assert type(twin) is type(est) and not hasattr(twin, "W_")
    mine, theirs = est.get_params(), twin.get_params()
    assert list(mine) == list(theirs) and all(mine[n] == theirs[n] for n in mine if n != "shape_2d") and theirs["shape_2d"] == (4, 5)
    back = pickle.loads(pickle.dumps(est))
    assert type(back) is type(est) and back.get_params().keys() == mine.keys()
    for name in ("G_", "W_", "H_", "X_"):
        assert np.array_equal(getattr(back, name), getattr(est, name)), name
    assert back.norm_factor_ == est.norm_factor_ and back._identity_G is True
    Xb, layout = back._image_argument(None, "pixel_diagnostics")
    assert layout == "cm" and np.array_equal(Xb, est.X_ / est.norm_factor_)
