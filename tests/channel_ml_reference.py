"""The channel ML of espm_amd/channel_ml.py in numpy: with H held, channel c is one pixel problem whose observations are the p pixels of
row c of X and whose design is H^T, so the definition is the pixel rules themselves (tests/pixel_ml_newton_reference.py: the free-scale
rule; tests/pixel_ml_pinned_reference.py: the pinned rule, the root finder and ``_advance``) run on (X^T, H^T), with every result
transposed back.  Nothing of the rules is restated here.  Host only.

The cases (``case``): D = pixel_ml_reference.lines(n, k) with holes (entries of one column set to 0 over a range of channels) and whole
rows set to 0 (channels without a count), H = gamma(1, 1, (k, p)) dose with row 1 zeroed in about half of the pixels (k > 1),
X = poisson(D H) - drawn in that order from default_rng(seed):

    A    40 x  600, k = 3, dose 20, seed 3, holes D[5:9, 2],                    row 30 empty
    B   300 x 2500, k = 5, dose  4, seed 4, holes D[100:140, 0], D[200:260, 4], rows 17 and 299 empty: two workgroups of channels, two
                                                                                 2048-pixel chunks of the pass
    C8   64 x  400, k = 8, dose  8, seed 5: the widest instance
    C1   33 x  257, k = 1, dose  6, seed 6,                                     row 2 empty: one component, nothing to pin against"""
import functools

import numpy as np

import pixel_ml_newton_reference as nr
import pixel_ml_pinned_reference as pn
import pixel_ml_reference as pr
from pixel_ml_reference import LOG_SHIFT  # noqa: F401  (shared with the GPU tests)

MAX_PASS, MAX_EVAL = 128, 64     # what the GPU tests pass: every fit of the reference converges within HALF of each
CASES = dict(A=dict(n=40, p=600, k=3, dose=20.0, seed=3, holes=((5, 9, 2),), rows=(30,)),
             B=dict(n=300, p=2500, k=5, dose=4.0, seed=4, holes=((100, 140, 0), (200, 260, 4)), rows=(17, 299)),
             C8=dict(n=64, p=400, k=8, dose=8.0, seed=5, holes=(), rows=()),
             C1=dict(n=33, p=257, k=1, dose=6.0, seed=6, holes=(), rows=(2,)))


def generate(n, p, k, dose, seed, holes=(), rows=()):
    """(X uint8 (n, p), H (k, p), D (n, k) the truth), read-only."""
    rng = np.random.default_rng(seed)
    D = pr.lines(n, k).copy()
    for lo, hi, j in holes:
        D[lo:hi, j] = 0.0
    for c in rows:
        D[c] = 0.0
    H = rng.gamma(1.0, 1.0, (k, p)) * dose
    if k > 1:
        H[1, rng.random(p) < 0.5] = 0.0
    X = rng.poisson(D @ H)
    assert X.max() <= 255
    X = X.astype(np.uint8)
    for a in (X, H, D):
        a.setflags(write=False)
    return X, H, D


@functools.lru_cache(maxsize=None)
def case(name):
    return generate(**CASES[name])


def _t(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)


def ml_channels(X, H, D0=None, components=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """The free-scale rule on every channel: dict(D (n, k), deviance, gap, n_pass, converged, N (n,), unmodelled, n_reject)."""
    out = nr.ml_unmix(np.asarray(X).T, np.asarray(H).T, _t(D0), components, tol, max_pass, log_shift)
    return dict(D=out["H"].T, deviance=out["deviance"], gap=out["gap"], n_pass=out["n_pass"], converged=out["converged"], N=out["N"],
                unmodelled=out["unmodelled"], n_reject=out["n_reject"])


def ml_channels_pinned(X, H, pin, t, D0=None, components=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """The pinned rule on every channel: ``ml_channels``'s dict plus slope (n,) and nonfinite."""
    out = pn.ml_unmix_pinned(np.asarray(X).T, np.asarray(H).T, pin, t, _t(D0), components, tol, max_pass, log_shift)
    return dict(D=out["H"].T, deviance=out["deviance"], gap=out["gap"], slope=out["slope"], n_pass=out["n_pass"], converged=out["converged"],
                N=out["N"], nonfinite=out["nonfinite"], n_reject=out["n_reject"])


def presence(X, H, D0=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """The nested fits of espm_amd.channel_ml.presence: the full fit by the free-scale rule, then for every j the pinned rule at
    t = 0 over the other components from the full solution: dict(D_ml, deviance_ml, lr (n, k), converged, gap, n_pass (k + 1, n),
    deviance_without (n, k))."""
    k = np.asarray(H).shape[0]
    full = ml_channels(X, H, D0, None, tol, max_pass, log_shift)
    rows = [full] + [ml_channels_pinned(X, H, j, 0.0, full["D"], None, tol, max_pass, log_shift) for j in range(k)]
    without = np.stack([r["deviance"] for r in rows[1:]], axis=1)
    lr = np.where(full["D"] == 0, 0.0, np.maximum(without - full["deviance"][:, None], 0.0))
    return dict(D_ml=full["D"], deviance_ml=full["deviance"], lr=lr, converged=np.stack([r["converged"] for r in rows]),
                gap=np.stack([r["gap"] for r in rows]), n_pass=np.stack([r["n_pass"] for r in rows]), deviance_without=without)


def presence_free(X, H, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """The same statistic with the reduced fits by the FREE-scale rule over the other components (pixel_ml_newton_reference.presence):
    another path to the same two minima - dict(lr (n, k), n_pass (k + 1, n), converged (k + 1, n))."""
    out = nr.presence(np.asarray(X).T, np.asarray(H).T, None, tol, max_pass, log_shift)
    return dict(lr=out["lr"].T, n_pass=out["n_pass"], converged=out["converged"])


def intervals(X, H, D0=None, level=0.95, components=None, tol=1e-3, lr_tol=1e-2, max_eval=MAX_EVAL, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """pixel_ml_pinned_reference.intervals on (X^T, H^T): dict(D_ml, lower, upper (n, k), deviance_ml (n,), threshold, converged, n_eval,
    n_pass (k, 2, n), max_fit_pass)."""
    out = pn.intervals(np.asarray(X).T, np.asarray(H).T, _t(D0), level, components, tol, lr_tol, max_eval, max_pass, log_shift)
    return dict(D_ml=out["H_ml"].T, deviance_ml=out["deviance_ml"], lower=out["lower"].T, upper=out["upper"].T, threshold=out["threshold"],
                converged=out["converged"], n_eval=out["n_eval"], n_pass=out["n_pass"], max_fit_pass=out["max_fit_pass"])


def profile(X, H, pin, t, D0=None, tol=1e-8, max_pass=20000, log_shift=LOG_SHIFT):
    """g*(t) (n,): the pinned deviance of every channel at t (n,) to ``tol`` - the long run that an interval end is held against."""
    out = ml_channels_pinned(X, H, pin, t, D0, None, tol, max_pass, log_shift)
    assert out["converged"].all()
    return out["deviance"]


@functools.lru_cache(maxsize=None)
def optimum(name):
    """The full fit's long run (tol = 1e-10): dict(D, deviance, gap, ...), shared - treat as read-only."""
    X, H, _ = case(name)
    out = ml_channels(X, H, None, None, 1e-10, 20000)
    assert out["converged"].all()
    return out


@functools.lru_cache(maxsize=None)
def solved(name):
    """``presence`` of a case (k > 1) at the tests' tol from the default start, shared - treat as read-only."""
    X, H, _ = case(name)
    return presence(X, H)


@functools.lru_cache(maxsize=None)
def solved_intervals(name):
    """``intervals`` of a case at the tests' tolerances from the default start, shared - treat as read-only."""
    X, H, _ = case(name)
    return intervals(X, H)
