"""The pinned rule and the root finder of ``espm_amd.spectra_ml.ml_spectra_pinned`` / ``intervals`` restated in numpy, beside the rule
of tests/spectra_ml_reference.py whose cases, sums and free set it shares, and with the bracket of tests/pixel_ml_pinned_reference.py
(``_advance``, ``threshold``).  Host only.  This file is the definition of the two, as the other ``*_reference.py`` files are of theirs.

The pinned rule.  X, G, H, a, N, F, log_shift, tol as in the spectra rule; ``pin`` = (e*, j*) an entry of F held at t >= 0;
M = F \\ {pin} (possibly empty):

    entry   W_pin = t; W = 0 outside F; N == 0: W_M = 0; a start in M that is not > 0 becomes N / (|M| a_ej) * 1e-3
    a pass  NO scale onto the ray.  y = max(G W H, log_shift), the pinned entry included; dev, q = G^T Q and A as in the rule;
            r = q / a on M;
            gap = 2 sum_M (a - q) W + 2 N max(max_M r - 1, 0);   slope = 2 (a_pin - q_pin), the derivative of the profile deviance in t
            REJECT / ACCEPT, the tau schedule and the stop gap <= tol: the rule's
            e = W * r on M, the pin kept at t
            B = F_obs[M, M] + tau diag(a / W), delta = B^-1 (q - a)_M by Cholesky
            W_M <- max(W + delta, 0.01 W, H_FLOOR N / a): without the scale onto the ray nothing else keeps an entry from underflowing
            a factorisation or a delta that is not finite: W_M <- e, trial <- False, counted
    M empty the fit is the one evaluating pass, gap 0
    bad t   negative or not finite: not converged after 0 passes
    Every pass is counted, the certifying one included.  At the cap the last ACCEPTED point is reported.

THE CERTIFICATE is the pixel pinned rule's with s -> a.  g(W_M) = dev at W_pin = t is convex with gradient
2 (a - q) on M, so for its minimiser W* over {W_M >= 0}
    dev(W) - dev(W*) <= 2 sum_M (a - q) (W - W*) = 2 sum_M (a - q) W + 2 sum_M (q - a) W*  <=  2 sum_M (a - q) W + 2 max(max_M r - 1, 0) sum_M a W*
and at the pinned optimum complementary slackness gives sum_M a W* = sum_M q W* = sum_cp (x / y) (y - t g_e* h_j*) over the entries that
are not floored <= the counts in them <= N: the right side is ``gap``.  The caveat is the rule's: with counted entries under the
floor (``unmodelled``: U counts in them) sum_M q W counts only N - U of the counts, and the bound holds for the floored model - the
deviance with y = max(., log_shift) - as it does there.

The root finder, per tested entry (e, j) of F and side, on phi(t) = g(t) - deviance_ml - q_level with g the certified pinned deviance
and q_level = 2 erfinv(level)^2; it stops where the fit converged and |phi| <= lr_tol.  It is pixel_ml_pinned_reference.intervals with
h_ml -> W_ml[e, j] and s_j -> a_ej:

    upper   bracket [W_ml, inf); first t = W_ml + w0, w0 = sqrt(q_level) sqrt(a W_ml + q_level) / a; then ``_advance``
    lower   exactly 0 where W_ml == 0 (no evaluation); first t = 0, and exactly 0 where phi(0) <= 0; then the bracket (0, W_ml), second
            t = max(W_ml - w0, W_ml / 2), then ``_advance``
    every evaluation is one pinned fit from the W of the evaluation before (the first: W_ml) with every entry of M lifted to at least
    N / ((|F| - 1) a) * 1e-3; a pinned fit that does not converge ends that end as not converged."""
import functools

import numpy as np

import spectra_ml_reference as R
from pixel_ml_newton_reference import H_FLOOR
from pixel_ml_pinned_reference import _advance, threshold
from spectra_ml_reference import LOG_SHIFT, START, TAU0, TAU_MAX, TAU_MIN, TAU_STEP, THETA, column_sums, free_set, information, sums

MAX_PASS = 128     # what the GPU tests pass as max_pass: every pinned fit of the reference converges within HALF of it
MAX_EVAL = 64      # ... and every end within half of this


def _pin(pin, F):
    e, j = (int(v) for v in pin)
    if not (0 <= e < F.shape[0] and 0 <= j < F.shape[1]) or not F[e, j]:
        raise ValueError(f"the pin {pin} is no free entry that the model sees")
    return e, j


def evaluate(X, G, H, W, pin, free=None, log_shift=LOG_SHIFT):
    """Deviance, gap and slope of the pinned rule at the given W, recomputed: dict(deviance, gap, slope, q, a, N, unmodelled)."""
    X, G, H, W = (np.asarray(v, dtype=np.float64) for v in (X, G, H, W))
    F, _ = free_set(G, H, free)
    pin = _pin(pin, F)
    M = F.copy()
    M[pin] = False
    a = column_sums(G, H)
    s = sums(X, G @ W, H, log_shift)
    q = G.T @ s["Q"]
    N = X.sum()
    gap = 0.0
    if M.any():
        gap = 2.0 * float((a[M] - q[M]) @ W[M]) + 2.0 * N * max((q[M] / a[M]).max() - 1.0, 0.0)
    return dict(deviance=s["dev"].sum(), gap=gap, slope=2.0 * (a[pin] - q[pin]), q=q, a=a, N=N, unmodelled=s["unmodelled"])


def ml_spectra_pinned(X, G, H, pin, t, W0=None, free=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """The pinned rule.  dict(W, deviance, channel_deviance, gap, slope, n_pass, n_rejected, n_fallback, converged, inert, unmodelled, N)."""
    X, G, H = (np.asarray(v, dtype=np.float64) for v in (X, G, H))
    m, k = G.shape[1], H.shape[0]
    a = column_sums(G, H)
    F, inert = free_set(G, H, free)
    pin = _pin(pin, F)
    M = F.copy()
    M[pin] = False
    nM = int(M.sum())
    N = X.sum()
    t = float(t)
    out = dict(W=np.zeros((m, k)), deviance=0.0, channel_deviance=np.zeros(G.shape[0]), gap=0.0, slope=0.0, n_pass=0, n_rejected=0,
               n_fallback=0, converged=False, inert=inert, unmodelled=0, N=N)
    if not t >= 0 or not np.isfinite(t):
        return out
    W = np.where(M, np.ones((m, k)) if W0 is None else np.array(W0, dtype=np.float64), 0.0)
    if N == 0:
        W[:] = 0.0
    elif nM:
        bad = M & ~(W > 0)
        W[bad] = N / (nM * a[bad]) * START
    W[pin] = t
    idx = np.flatnonzero(M.ravel())
    tau, dev_acc, trial, e = TAU0, np.inf, False, None
    for _ in range(max_pass):
        s = sums(X, G @ W, H, log_shift)
        q = G.T @ s["Q"]
        dev = s["dev"].sum()
        out["n_pass"] += 1
        if trial and not dev <= dev_acc:
            W, trial, tau = e, False, min(tau * TAU_STEP, TAU_MAX)
            out["n_rejected"] += 1
            continue
        r = np.zeros_like(a)
        r[M] = q[M] / a[M]
        gap = 2.0 * float((a[M] - q[M]) @ W[M]) + 2.0 * N * max(r[M].max() - 1.0, 0.0) if nM else 0.0
        dev_acc = dev
        out.update(W=W.copy(), deviance=dev, channel_deviance=s["dev"], gap=gap, slope=2.0 * (a[pin] - q[pin]), unmodelled=s["unmodelled"])
        if gap <= tol:
            out["converged"] = True
            break
        if trial:
            tau = max(tau / TAU_STEP, TAU_MIN)
        e = W * r
        e[pin] = t
        with np.errstate(all="ignore"):
            B = information(G, s["A"])[np.ix_(idx, idx)]
            B[np.arange(idx.size), np.arange(idx.size)] += tau * (a[M] / W[M])
            try:
                L = np.linalg.cholesky(B)
                z = np.linalg.solve(L, (q - a)[M])
                delta = np.linalg.solve(L.T, z)
                ok = bool(np.isfinite(delta).all())
            except np.linalg.LinAlgError:
                ok = False
        if not ok:
            W, trial = e, False
            out["n_fallback"] += 1
            continue
        step = W.copy()
        step[M] = np.maximum(np.maximum(W[M] + delta, THETA * W[M]), H_FLOOR * N / a[M])
        W, trial = step, True
    return out


def intervals(X, G, H, W0=None, free=None, entries=None, level=0.95, tol=1e-3, lr_tol=1e-2, max_eval=MAX_EVAL, max_pass=MAX_PASS,
              log_shift=LOG_SHIFT):
    """``espm_amd.spectra_ml.intervals`` on the host: the same dict, plus ``max_fit_pass`` - the most passes any single pinned fit took."""
    X, G, H = (np.asarray(v, dtype=np.float64) for v in (X, G, H))
    a = column_sums(G, H)
    F, inert = free_set(G, H, free)
    ql = threshold(level)
    full = R.ml_spectra(X, G, H, W0, free, tol, max_pass, log_shift)
    W_ml, dev_ml, N = full["W"], full["deviance"], full["N"]
    ent = np.argwhere(F) if entries is None else np.asarray(entries, dtype=np.int64).reshape(-1, 2)
    E = len(ent)
    lower, upper = np.full(F.shape, np.nan), np.full(F.shape, np.nan)
    conv, n_eval, n_pass = np.zeros((E, 2), dtype=bool), np.zeros((E, 2), dtype=np.int64), np.zeros((E, 2), dtype=np.int64)
    max_fit_pass = 0
    nF = int(F.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        lift = np.where(F, N / ((nF - 1) * a) * START, 0.0) if nF > 1 else np.zeros(F.shape)
    for i, (e, j) in enumerate(ent):
        if not F[e, j]:
            conv[i] = True      # outside the free set: no fit, as ``presence`` has it
            continue
        if not full["converged"]:
            continue
        M = F.copy()
        M[e, j] = False
        w_ml, ae = W_ml[e, j], a[e, j]
        w0 = np.sqrt(ql) * np.sqrt(ae * w_ml + ql) / ae
        for side in (0, 1):
            up = side == 1
            out = upper if up else lower
            if up:
                lo, hi, t = w_ml, np.inf, w_ml + w0
            else:
                lo, hi, t = 0.0, w_ml, 0.0
                if w_ml == 0:
                    out[e, j], conv[i, side] = 0.0, True
                    continue
            Wc = W_ml.copy()
            for ev in range(max_eval):
                Wc[M] = np.maximum(Wc[M], lift[M])
                fit = ml_spectra_pinned(X, G, H, (e, j), t, Wc, free, tol, max_pass, log_shift)
                Wc = fit["W"].copy()
                n_eval[i, side] += 1
                n_pass[i, side] += fit["n_pass"]
                max_fit_pass = max(max_fit_pass, fit["n_pass"])
                if not fit["converged"]:
                    break
                phi = fit["deviance"] - dev_ml - ql
                if abs(phi) <= lr_tol or (not up and ev == 0 and phi <= 0):     # the boundary: the interval reaches 0
                    out[e, j], conv[i, side] = t, True
                    break
                tn, lo, hi = (float(v) for v in _advance(np.float64(t), np.float64(phi), np.float64(fit["slope"]), np.float64(lo),
                                                         np.float64(hi), np.float64(w_ml), up))
                t = max(w_ml - w0, 0.5 * w_ml) if (not up and ev == 0) else tn
    return dict(W_ml=W_ml, deviance_ml=dev_ml, lower=lower, upper=upper, level=level, threshold=ql, entries=ent, converged=conv,
                n_eval=n_eval, n_pass=n_pass, n_full_pass=full["n_pass"], inert=inert, unmodelled=full["unmodelled"],
                max_fit_pass=max_fit_pass)


# the entries of "planted" that the CPU test walks (the whole case takes a minute in numpy): the two planted at zero and two positive ones
PLANTED_SUBSET = tuple(R.PLANTED_AT) + ((0, 0), (3, 3))


@functools.lru_cache(maxsize=None)
def solved(name):
    """``intervals`` of a named case over all its entries ("planted": over PLANTED_SUBSET) from W = 1 at level 0.95, tol 1e-3,
    lr_tol 1e-2, computed once and shared (treat as read-only)."""
    X, G, _, H = R.case(name)
    return intervals(X, G, H, entries=np.array(PLANTED_SUBSET) if name == "planted" else None)


@functools.lru_cache(maxsize=None)
def full_optimum(name):
    """The full fit's long run: the rule at tol = 1e-8 from the solution at the tests' tol - a point certified by its own gap."""
    X, G, _, H = R.case(name)
    return R.ml_spectra(X, G, H, R.solved(name)["W"], None, 1e-8, 20000)


def long_run_phi(name, W_ml, entry, t, dev_opt, level=0.95):
    """phi at an end from the long runs: the pinned rule at tol = 1e-8 from ``W_ml`` with ``entry`` held at t, less the full optimum's
    deviance and the quantile: (phi, the long fit)."""
    X, G, _, H = R.case(name)
    fit = ml_spectra_pinned(X, G, H, entry, t, W_ml, None, 1e-8, 20000)
    return fit["deviance"] - dev_opt - threshold(level), fit


def check_ends(name, out, lr_tol=1e-2, tol=1e-3, level=0.95):
    """The long-run check of every end that ``out`` (an ``intervals`` dict of case ``name``) reports: |g*(t) - dev* - q_level| <=
    lr_tol + tol + 1e-9 dev* at ends that are not 0, g*(0) - dev* - q_level <= the same bound at ends that are 0.  The bound is derived:
    each reported deviance lies within its gap <= tol of its minimum, and the stop is lr_tol on reported values.  Returns the worst
    |phi| of the ends that are not 0, the largest phi of the ends that are 0 (-inf without one) and the most passes of a long run."""
    opt = full_optimum(name)
    assert opt["converged"]
    bound = lr_tol + tol + 1e-9 * opt["deviance"]
    worst, worst0, passes = 0.0, -np.inf, 0
    for (e, j) in out["entries"]:
        for side, ends in enumerate((out["lower"], out["upper"])):
            t = ends[e, j]
            if np.isnan(t):
                continue
            phi, fit = long_run_phi(name, out["W_ml"], (e, j), t, opt["deviance"], level)
            assert fit["converged"], (name, e, j, side)
            passes = max(passes, fit["n_pass"])
            if t == 0:
                assert side == 0
                worst0 = max(worst0, phi)
                assert phi <= bound, (name, e, j, side, phi)
            else:
                worst = max(worst, abs(phi))
                assert abs(phi) <= bound, (name, e, j, side, phi)
    return worst, worst0, passes
