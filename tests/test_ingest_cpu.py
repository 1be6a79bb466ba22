"""CPU-only checks of what a fit or an unmix does before an engine exists (espm_amd/estimators/ingest.py: the per-chunk scans of the
upload, on CPU tensors against numpy) and of the stop rules the fit's and the unmix's loops share (estimators/base.py::stop_message)."""
import numpy as np
import pytest
import torch

LOG_SHIFT = 1e-14


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def _array(dtype, dirty):
    """12 x 20 counts with a non-integer entry, an all-zero row and an all-zero column; ``dirty``: also one NaN, one infinity, one negative entry."""
    X = np.random.default_rng(11).poisson(1.5, size=(12, 20)).astype(dtype)
    X[4, :] = 0
    X[:, 13] = 0
    X[2, 5] = 2.5
    if dirty:
        X[1, 3], X[7, 9], X[10, 0] = np.nan, np.inf, -3.0
    return X


def _numpy_scans(X):
    Xd = X.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return dict(row_sum=Xd.sum(axis=1), col_sum=Xd.sum(axis=0), bad=np.array([(~np.isfinite(X)).sum(), np.isnan(X).sum(), (X < 0).sum()]),
                    s1=Xd.sum(), s2=(Xd * np.log(np.maximum(Xd, LOG_SHIFT))).sum(),
                    facts=np.array([(X != np.round(X)).sum(), (X != 0).sum(), X.max()], dtype=np.float64))


def _assert_scans(got, want):
    """Counts (and the largest entry) exactly, the fp64 sums to 1e-12 (a NaN or an infinity where numpy has one)."""
    assert got["bad"].dtype == torch.int64 and all(got[key].dtype == torch.float64 for key in ("row_sum", "col_sum", "s1", "s2", "facts"))
    np.testing.assert_array_equal(got["bad"].numpy(), want["bad"])
    np.testing.assert_array_equal(got["facts"].numpy(), want["facts"])
    for key in ("row_sum", "col_sum", "s1", "s2"):
        np.testing.assert_allclose(got[key].numpy(), want[key], rtol=1e-12, atol=0, err_msg=key)


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "nan_inf_negative"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scan_chunk_against_numpy_and_accumulated_over_row_chunks(dtype, dirty):
    from espm_amd.estimators.ingest import add_chunk_scans, scan_chunk
    X = _array(dtype, dirty)
    want = _numpy_scans(X)
    assert list(want["bad"]) == ([2, 1, 1] if dirty else [0, 0, 0]) and want["facts"][0] == (2 if dirty else 1)   # (NaN is no integer)
    assert (want["row_sum"] == 0).sum() == 1 and (want["col_sum"] == 0).sum() == 1
    assert np.isfinite(want["s2"]) != dirty
    whole = scan_chunk(torch.from_numpy(X), LOG_SHIFT)
    _assert_scans(whole, want)
    # three row chunks, accumulated the way _upload_with_scans does
    f64 = dict(dtype=torch.float64)
    acc = dict(row_sum=torch.empty(12, **f64), col_sum=torch.zeros(20, **f64), bad=torch.zeros(3, dtype=torch.int64), s1=torch.zeros((), **f64),
               s2=torch.zeros((), **f64), facts=torch.zeros(3, **f64))
    for a, b in ((0, 5), (5, 9), (9, 12)):
        add_chunk_scans(acc, a, scan_chunk(torch.from_numpy(X[a:b]), LOG_SHIFT))
    _assert_scans(acc, want)
    _assert_scans(acc, {key: whole[key].numpy() for key in whole})


def test_device_prep_predicate_without_a_device_or_below_the_threshold(monkeypatch):
    from espm_amd.estimators import ingest
    X = np.zeros((40, 50), dtype=np.float32)
    monkeypatch.setattr(ingest, "_DEVICE_PREP_MIN_SIZE", 2000)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert ingest.device_prep_applies(X, False) and ingest.device_prep_applies(X.astype(np.float64).T, False)
    assert not ingest.device_prep_applies(X, True)                                # fp64 mode: the host passes
    assert not ingest.device_prep_applies(X.astype(np.int32), False)              # validate_data converts it on the host
    assert not ingest.device_prep_applies(X[:39], False) and not ingest.device_prep_applies(X.tolist(), False) and not ingest.device_prep_applies(X[0], False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert not ingest.device_prep_applies(X, False)


def test_ingest_host_fills_the_empty_lines_and_refuses_negative_values():
    from espm_amd.estimators import SmoothNMF, ingest
    X = _array(np.float32, False)
    rec = ingest.ingest_host(X, LOG_SHIFT, SmoothNMF().remove_zeros_lines)
    want = X.copy()
    want[4, :] = want[:, 13] = LOG_SHIFT
    np.testing.assert_array_equal(rec.X_fixed, want)
    assert rec.fill and list(np.flatnonzero(rec.empty_ch)) == [4] and list(np.flatnonzero(rec.empty_px)) == [13]
    assert rec.Xd_raw is None and rec.Xd is None and rec.lazy is None and rec.mean_x is None and rec.layout == "cm" and not rec.x_local
    assert rec.without_x().X_fixed is None and rec.without_x().fill
    assert not ingest.ingest_host(X[:4, :13] + 1, LOG_SHIFT, SmoothNMF().remove_zeros_lines).fill
    with pytest.raises(ValueError, match="Negative values in data"):
        ingest.ingest_host(-X, LOG_SHIFT, SmoothNMF().remove_zeros_lines)


TOL = 1e-4
STOPS = {
    # name: ((rel_W, rel_H, eval_before, eval_after, eval_init), message) - the decreases are powers of two: 0.5 / 8192 = 6.103515625e-05
    "rel": ((1e-5, 2e-5, 8.0, 7.0, 8.0), "exits because of relative change rel_A 2e-05 and rel_P 1e-05 < tol "),
    "loss": ((0.5, 0.25, 8.0, 7.5, 8192.0), "exits because of relative change < tol: 6.103515625e-05"),
    "nan": ((0.5, 0.25, 8.0, float("nan"), 8.0), "exit because of the presence of NaN"),
    "negative_decrease": ((0.5, 0.25, 7.5, 8.0, 8.0), "exit because of negative decrease -0.5: 7.5, 8.0"),
    "goes_on": ((0.5, 0.25, 8.0, 7.0, 8.0), None),
    # two rules at once: the earlier one in the reference's order speaks
    "rel_before_loss": ((1e-5, 2e-5, 8.0, 7.5, 8192.0), "exits because of relative change rel_A 2e-05 and rel_P 1e-05 < tol "),
    "rel_before_nan": ((1e-5, 2e-5, 8.0, float("nan"), 8.0), "exits because of relative change rel_A 2e-05 and rel_P 1e-05 < tol "),
    "nan_with_rel_not_met": ((0.5, 2e-5, float("nan"), float("nan"), 8.0), "exit because of the presence of NaN"),
    "small_negative_decrease_is_the_loss_rule": ((0.5, 0.25, 7.5, 8.0, 8192.0), "exits because of relative change < tol: -6.103515625e-05"),
    "rel_before_negative_decrease": ((1e-5, 2e-5, 7.5, 8.0, 8.0), "exits because of relative change rel_A 2e-05 and rel_P 1e-05 < tol "),
    "one_of_rel_W_rel_H_is_not_enough": ((0.5, 2e-5, 8.0, 7.0, 8.0), None),
    # the first iteration: eval_before = inf
    "first_iteration": ((0.5, 0.25, float("inf"), 7.0, 8.0), None),
    "first_iteration_nan": ((0.5, 0.25, float("inf"), float("nan"), 8.0), "exit because of the presence of NaN"),
    # unmix: rel_W = 0.0
    "unmix_rel": ((0.0, 2e-5, 8.0, 7.0, 8.0), "exits because of relative change rel_A 2e-05 and rel_P 0.0 < tol "),
    "unmix_goes_on": ((0.0, 0.25, 8.0, 7.0, 8.0), None),
}


@pytest.mark.parametrize("name", sorted(STOPS))
def test_stop_message_rules_order_and_wording(name):
    from espm_amd.estimators.base import stop_message
    args, want = STOPS[name]
    assert stop_message(*args, TOL) == want
