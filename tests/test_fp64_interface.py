"""The fp64 mode's interface without a GPU: set_precision, get_params, pickling, and the refusals that fit raises before
anything is uploaded (an engine is never built for them)."""
import pickle

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


def test_set_precision_validates_and_returns_self(lib):
    from espm_amd.estimators import SmoothNMF
    est = SmoothNMF(n_components=3)
    assert est.set_precision("fp64") is est
    assert est._precision == "fp64"
    assert est.set_precision("fp32") is est
    with pytest.raises(ValueError):
        est.set_precision("fp16")


def test_precision_is_not_a_parameter_and_survives_pickling(lib):
    from espm_amd.estimators import SmoothNMF
    plain = SmoothNMF(n_components=3).get_params()
    est = SmoothNMF(n_components=3).set_precision("fp64")
    assert est.get_params() == plain
    assert "precision" not in est.get_params()
    again = pickle.loads(pickle.dumps(est))
    assert again._precision == "fp64"


def _refused(est, X=None):
    X = np.ones((12, 20)) if X is None else X
    with pytest.raises(NotImplementedError, match="fp64 mode"):
        est.set_precision("fp64").fit(X)
    assert getattr(est, "_engine", None) is None


@pytest.mark.parametrize("kw", [dict(algo="l2_surrogate"), dict(algo="bmd"), dict(algo="projected_gradient", gamma=[1.0, 1.0], simplex_W=False),
                                dict(linesearch=True, lambda_L=1.0), dict(algo="l2_surrogate", l2=True), dict(n_components=9)],
                         ids=["l2_surrogate", "bmd", "projected_gradient", "linesearch", "l2", "k9"])
def test_fp64_refusals(lib, kw):
    from espm_amd.estimators import SmoothNMF
    kw = dict(kw)
    _refused(SmoothNMF(n_components=kw.pop("n_components", 2), verbose=0, **kw))


def test_fp64_refuses_truth_tracking_and_shard(lib):
    from espm_amd.estimators import SmoothNMF
    _refused(SmoothNMF(n_components=2, verbose=0, true_D=np.ones((12, 2)), true_H=np.ones((2, 20))))
    est = SmoothNMF(n_components=2, verbose=0)
    est._shard_group = object()   # (what shard(group) stores; the refusal comes before the group is used)
    _refused(est)


def test_wide_builds_refuse_fp64_entry_points(lib):
    for k in (9, 17):
        v = lib.variant(k)
        assert v.lib.espm_f64_gw(None, None, 1, 1, k, 1e-14, None, None, None, None) == lib.EUNSUPPORTED
