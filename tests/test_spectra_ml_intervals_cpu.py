"""The pinned spectra rule and its root finder in numpy (tests/spectra_ml_pinned_reference.py, the definition of
``espm_amd.spectra_ml.ml_spectra_pinned`` and ``intervals``): what the GPU tests of test_gpu_spectra_ml_intervals.py rest on, and the
argument refusals of the new Python functions, which need no GPU.  Host only.

The caps are conditions, with a factor two or more of room over what the rule needs at level 0.95, tol 1e-3, lr_tol 1e-2: the most
passes of one pinned fit were 18 (k8 and planted), the most evaluations of an end 7."""
import numpy as np
import pytest

import spectra_ml_pinned_reference as P
import spectra_ml_reference as R

CASES = ("k1", "k3", "k8", "seams", "planted")   # "planted": over P.PLANTED_SUBSET (the whole case takes a minute in numpy)


@pytest.mark.parametrize("name", CASES)
def test_every_end_converges_within_the_caps_and_the_intervals_are_ordered(name):
    out = P.solved(name)
    E = len(out["entries"])
    tested = np.zeros(out["W_ml"].shape, dtype=bool)
    tested[out["entries"][:, 0], out["entries"][:, 1]] = True
    print(f"{name}: {2 * E} ends, {out['n_pass'].sum()} passes, most in one fit {out['max_fit_pass']}, most evaluations {out['n_eval'].max()}, "
          f"lower == 0 at {(out['lower'] == 0).sum()}")
    assert out["converged"].shape == out["n_eval"].shape == out["n_pass"].shape == (E, 2)
    assert out["converged"].all()
    assert out["max_fit_pass"] <= P.MAX_PASS // 2 and out["n_eval"].max() <= P.MAX_EVAL // 2
    lo, hi, W = out["lower"][tested], out["upper"][tested], out["W_ml"][tested]
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo >= 0).all() and (lo <= W).all() and (W <= hi).all()
    assert np.isnan(out["lower"][~tested]).all() and np.isnan(out["upper"][~tested]).all()


def test_planted_entries_get_an_upper_limit_and_the_others_an_error_bar():
    out = P.solved("planted")
    for e, j in P.PLANTED_SUBSET:
        lo, hi = out["lower"][e, j], out["upper"][e, j]
        if (e, j) in R.PLANTED_AT:
            assert lo == 0.0 and hi > 0 and np.isfinite(hi)
        else:
            assert lo > 0 and np.isfinite(hi)


@pytest.mark.parametrize("name", CASES)
def test_ends_against_the_long_runs(name):
    """|g*(t) - dev* - q_level| <= lr_tol + tol + 1e-9 dev* with both deviances from runs at tol = 1e-8 (``P.check_ends`` asserts it
    at every end, and g*(0) - dev* - q_level <= the same at ends that are 0)."""
    worst, worst0, passes = P.check_ends(name, P.solved(name))
    print(f"{name}: |phi| <= {worst:.3g} at the ends that are not 0, phi <= {worst0:.3g} at those that are; long runs within {passes} passes")


def test_the_pinned_rule_alone():
    X, G, _, H = R.case("k3")
    W_ml = R.solved("k3")["W"]
    pin = (5, 2)
    at_ml = P.ml_spectra_pinned(X, G, H, pin, W_ml[pin], W_ml)
    # the pin at its ML value: the minimum is the full one (within the two gaps), and the profile is flat there
    assert at_ml["converged"] and abs(at_ml["deviance"] - R.solved("k3")["deviance"]) <= 2e-3 and at_ml["W"][pin] == W_ml[pin]
    ev = P.evaluate(X, G, H, at_ml["W"], pin)
    assert ev["deviance"] == at_ml["deviance"] and ev["gap"] == at_ml["gap"] and ev["slope"] == at_ml["slope"]
    lo, hi = P.ml_spectra_pinned(X, G, H, pin, 0.0, W_ml), P.ml_spectra_pinned(X, G, H, pin, 2 * W_ml[pin] + 1, W_ml)
    assert lo["converged"] and hi["converged"] and lo["slope"] < 0 < hi["slope"] and min(lo["deviance"], hi["deviance"]) > at_ml["deviance"]
    # a free set of the pin alone: one evaluating pass, gap 0
    one = np.zeros((6, 3), dtype=bool)
    one[pin] = True
    alone = P.ml_spectra_pinned(X, G, H, pin, 1.5, free=one)
    assert alone["converged"] and alone["n_pass"] == 1 and alone["gap"] == 0 and alone["W"].sum() == 1.5
    # a bad t: not converged after 0 passes; a bad pin raises
    for t in (-1.0, np.nan, np.inf):
        bad = P.ml_spectra_pinned(X, G, H, pin, t, W_ml)
        assert not bad["converged"] and bad["n_pass"] == 0
    for p in ((6, 0), (0, 3), (-1, 0)):
        with pytest.raises(ValueError, match="pin"):
            P.ml_spectra_pinned(X, G, H, p, 1.0)
    with pytest.raises(ValueError, match="pin"):
        P.ml_spectra_pinned(X, G, H, (0, 0), 1.0, free=~one & (np.arange(6)[:, None] > 0))


# ---- the refusals of the package's functions: before anything is uploaded, so they need no GPU -----------------------------------------
def test_refusals_of_ml_spectra_pinned():
    from espm_amd import spectra_ml as S
    X, G, _, H = R.case("k1")
    for pin in ((3, 0), (0, 1), (-1, 0), (0,), "ab", (0.5, 0)):
        with pytest.raises(ValueError, match="pin"):
            S.ml_spectra_pinned(X, G, H, pin, 1.0)
    hole = np.ones((3, 1), dtype=bool)
    hole[1, 0] = False
    with pytest.raises(ValueError, match="pin"):
        S.ml_spectra_pinned(X, G, H, (1, 0), 1.0, free=hole)
    for t in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="t must be finite and not negative"):
            S.ml_spectra_pinned(X, G, H, (0, 0), t)
    with pytest.raises(NotImplementedError, match="G is required"):
        S.ml_spectra_pinned(X, None, H, (0, 0), 1.0)
    with pytest.raises(ValueError, match="tol"):
        S.ml_spectra_pinned(X, G, H, (0, 0), 1.0, tol=0.0)


def test_refusals_of_intervals():
    from espm_amd import spectra_ml as S
    X, G, _, H = R.case("k1")
    for level in (0.0, 1.0, -0.5, True):
        with pytest.raises(ValueError, match="level"):
            S.intervals(X, G, H, level=level)
    with pytest.raises(ValueError, match="lr_tol"):
        S.intervals(X, G, H, lr_tol=0.0)
    for key in ("max_eval", "batch", "max_pass"):
        for v in (0, -1, 1.5):
            with pytest.raises(ValueError, match=key):
                S.intervals(X, G, H, **{key: v})
    for ent in ([[3, 0]], [[0, 1]], [[0, 0], [0, 0]], [0, 0], [[0.0, 0.0]]):
        with pytest.raises(ValueError, match="entries"):
            S.intervals(X, G, H, entries=np.array(ent))
    with pytest.raises(ValueError, match="no free entry"):
        S.intervals(X, G, H, free=np.zeros((3, 1), dtype=bool))
    with pytest.raises(NotImplementedError, match="G is required"):
        S.intervals(X, None, H)
    with pytest.raises(ValueError, match="W0"):
        S.intervals(X, G, H, W0=np.ones((2, 1)))
    assert S.BATCH_SCRATCH_BYTES == 1 << 30 and S.BATCH_INFO_BYTES == 256 << 20
