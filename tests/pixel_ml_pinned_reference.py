"""The pinned rule of include/espm_mu.h ("pixel ML, pinned") and the root finder of ``espm_amd.presence.intervals`` restated in numpy,
beside the Newton rule of tests/pixel_ml_newton_reference.py whose cases, start and step it shares.  Host only.

The rule, per pixel; x, N, s, log_shift, tol as in the Newton rule; M the fitted set (m = |M|, possibly 0), ``pin`` outside it, t >= 0:

    entry   h_pin = t; h_j = 0 outside M and pin; N == 0: h_M = 0; a start in M that is not > 0 becomes N / (m s_j) * 1e-3
    a pass  NO scale onto the ray.  y = max(D h, log_shift) over all components, the pinned one included; w, dev, q = D^T w, A as in
            the Newton rule; r_j = q_j / s_j, j in M;
            gap = 2 sum_M (s_j - q_j) h_j + 2 N max(max_M r_j - 1, 0);   slope = 2 (s_pin - q_pin)
            REJECT / ACCEPT, the stop gap <= tol, tau, e, the blended Cholesky step over M and the clamps: the Newton rule's
    bad t   negative or not finite: the pixel stops at once, not converged, counted in ``nonfinite``

The root finder, per (component j, side) and pixel, on phi(t) = g(t) - deviance_ml - q with g the certified pinned deviance and
q = 2 erfinv(level)^2; it stops at |phi| <= lr_tol:

    upper   bracket [h_ml, inf); first t = h_ml + w0, w0 = sqrt(q) sqrt(s_j h_ml + q) / s_j; while no t with phi > 0 is known the
            next t is the Newton step t - phi / slope, at most h_ml + 8 (t - h_ml), or h_ml + 2 (t - h_ml) where that step does not
            pass t; afterwards the Newton step where it falls strictly inside the bracket, else the midpoint
    lower   0 exactly where h_ml == 0 (no evaluation); first t = 0, and 0 exactly where phi(0) <= 0; then bracket (0, h_ml), second
            t = max(h_ml - w0, h_ml / 2) (the slope at t = 0 belongs to the floor where M is empty), then as above
    every evaluation is one pinned fit from the H of the evaluation before (the first: H_ml) with every fitted abundance lifted to at
    least N / ((k - 1) s_i) * 1e-3 - the rule's own fill of a start that is not positive: an abundance that the evaluation before
    drove to 1e-13 and that has to come back grows from there by a factor 1 + (r_i - 1) / tau a pass, which near the stop, where the
    accept / reject test works at the rounding of the deviance and tau climbs, is no growth at all -, passes counted from 0"""
import functools

import numpy as np

import pixel_ml_newton_reference as nr
import pixel_ml_reference as pr
from pixel_ml_newton_reference import H_FLOOR, TAU0, TAU_MAX, TAU_MIN, TAU_STEP, THETA, _solve, case  # noqa: F401
from pixel_ml_reference import LOG_SHIFT, mask_of, start_from  # noqa: F401  (shared with the GPU tests)

MAX_PASS = 128     # what the GPU tests pass as max_pass: every pinned fit of the reference converges within HALF of it
MAX_EVAL = 64      # ... and every endpoint within half of this
CASES = ("planted", "low8", "collinear", "tall", "img16", "img96_k1", "img96_k5")


def threshold(level):
    """The chi2_1 quantile: 2 erfinv(level)^2."""
    from scipy.special import erfinv
    return float(2.0 * erfinv(level) ** 2)


def evaluate(X, D, H, pin, components=None, log_shift=LOG_SHIFT):
    """Deviance, gap and slope of the pinned rule at the given H (k, p), recomputed: dict(deviance, gap, slope (p,), N)."""
    x = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    k = D.shape[1]
    M = mask_of(k, [j for j in range(k) if j != pin] if components is None else components)
    s, N = D.sum(axis=0), x.sum(axis=0)
    Y = D @ H
    Y = np.where(Y >= log_shift, Y, log_shift)
    w = x * (1.0 / Y)
    t = Y - x
    pos = x > 0
    t[pos] += x[pos] * np.log(w[pos])
    q = D.T @ w
    lin = ((s[M, None] - q[M]) * H[M]).sum(axis=0)
    rmax = (q[M] / s[M, None]).max(axis=0) if M.any() else np.full(N.shape, -np.inf)
    return dict(deviance=2.0 * t.sum(axis=0), gap=2.0 * (lin + N * np.maximum(rmax - 1.0, 0.0)), slope=2.0 * (s[pin] - q[pin]), N=N)


def ml_unmix_pinned(X, D, pin, t, H0=None, components=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT, history=False):
    """The pinned rule on every pixel of X (n, p): dict(H, deviance, gap, slope, n_pass, converged, nonfinite, N, n_reject) and with
    ``history`` also ``monotone``.  ``t``: a scalar or (p,).  ``components``: the fitted set (None: all but ``pin``).  ``H0`` None:
    N / sum_M s in M."""
    x = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    n, p = x.shape
    k = D.shape[1]
    M = mask_of(k, [j for j in range(k) if j != pin] if components is None else components)
    if M[pin]:
        raise ValueError("the pinned component is in the set")
    s = D.sum(axis=0)
    if not (s[M] > 0).all() or not s[pin] > 0:
        raise ValueError("a component of the set, or the pinned one, has an all-zero spectrum")
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (p,)).copy()
    N = x.sum(axis=0)
    m = int(M.sum())
    H = np.zeros((k, p))
    if m:
        if H0 is None:
            H[M] = N[None, :] / s[M].sum()
        else:
            H[M] = np.array(H0, dtype=np.float64)[M]
        fill = N[None, :] / (m * s[:, None]) * pr.START
        bad = ~(H > 0) & M[:, None]
        H[bad] = fill[bad]
        H[:, N == 0] = 0.0
    H[pin] = t
    nonfin = ~(t >= 0) | ~np.isfinite(t)
    done = nonfin.copy()
    conv = np.zeros(p, dtype=bool)
    dev, gap, slope = np.zeros(p), np.zeros(p), np.zeros(p)
    n_pass, n_reject = np.zeros(p, dtype=np.int64), np.zeros(p, dtype=np.int64)
    E = np.zeros((k, p))
    dev_acc, tau, trial = np.full(p, np.inf), np.full(p, TAU0), np.zeros(p, dtype=bool)
    monotone = np.ones(p, dtype=bool)
    DM, sM, dp = D[:, M], s[M], D[:, pin]
    live = np.flatnonzero(~done)
    for _ in range(max_pass):
        if live.size == 0:
            break
        h = H[:, live][M]
        xl = x[:, live]
        Y = DM @ h + dp[:, None] * t[live][None, :]
        Y = np.where(Y >= log_shift, Y, log_shift)
        w = xl * (1.0 / Y)
        tt = Y - xl
        pos = xl > 0
        tt[pos] += xl[pos] * np.log(w[pos])
        dv = 2.0 * tt.sum(axis=0)
        q = DM.T @ w
        r = q / sM[:, None]
        rmax = r.max(axis=0) if m else np.full(live.size, -np.inf)
        g = 2.0 * (((sM[:, None] - q) * h).sum(axis=0) + N[live] * np.maximum(rmax - 1.0, 0.0))
        sl = 2.0 * (s[pin] - dp @ w)
        rej = trial[live] & ~(dv <= dev_acc[live])
        acc = ~rej
        li = live[rej]
        H[:, li] = E[:, li]
        H[pin, li] = t[li]
        trial[li] = False
        tau[li] = np.minimum(tau[li] * TAU_STEP, TAU_MAX)
        n_reject[li] += 1
        la = live[acc]
        monotone[la] &= dv[acc] <= dev_acc[la]
        dev[la], gap[la], slope[la], dev_acc[la] = dv[acc], g[acc], sl[acc], dv[acc]
        stop = acc & (g <= tol)
        done[live[stop]] = True
        conv[live[stop]] = True
        go = acc & ~stop
        lg = live[go]
        if lg.size:
            hg = h[:, go]
            em = np.zeros((k, lg.size))
            em[M] = hg * r[:, go]
            E[:, lg] = em
            tau[lg] = np.where(trial[lg], np.maximum(tau[lg] / TAU_STEP, TAU_MIN), tau[lg])
            wy = w[:, go] * (1.0 / Y[:, go])
            B = np.einsum("cj,cl,cq->qjl", DM, DM, wy)
            with np.errstate(divide="ignore", over="ignore"):
                B[:, np.arange(m), np.arange(m)] += (tau[lg][None, :] * (sM[:, None] / hg)).T
            delta, singular = _solve(B, (sM[:, None] - q[:, go]).T)
            new = np.maximum(np.maximum(hg + delta.T, THETA * hg), H_FLOOR * N[lg][None, :] / sM[:, None])
            cand = np.zeros((k, lg.size))
            cand[M] = new
            cand[:, singular] = em[:, singular]
            cand[pin] = t[lg]
            H[:, lg] = cand
            trial[lg] = ~singular
        n_pass[live[~stop]] += 1
        live = live[~stop]
    out = dict(H=H, deviance=dev, gap=gap, slope=slope, n_pass=n_pass, converged=conv, nonfinite=int(nonfin.sum()), N=N, n_reject=n_reject)
    if history:
        out["monotone"] = monotone
    return out


def _advance(t, phi, slope, lo, hi, h_ml, upper):
    """The bracket with the evaluated point taken in, and the next point: (t, lo, hi), elementwise."""
    inner = phi < 0 if upper else phi > 0     # the evaluated point replaces the lower end of the bracket
    lo, hi = np.where(inner, t, lo), np.where(inner, hi, t)
    with np.errstate(all="ignore"):
        tn = t - phi / slope
        open_ = np.isinf(hi)
        good = np.isfinite(tn) & (tn > lo) & (tn < hi)
        tn = np.where(open_, np.minimum(tn, h_ml + 8.0 * (t - h_ml)), tn)
        mid = np.where(open_, h_ml + 2.0 * (t - h_ml), 0.5 * (lo + hi))
    return np.where(good, tn, mid), lo, hi


def intervals(X, D, H0=None, level=0.95, components=None, tol=1e-3, lr_tol=1e-2, max_eval=MAX_EVAL, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """``espm_amd.presence.intervals`` on the host: the same dict, plus ``max_fit_pass`` - the most passes any single pinned fit took."""
    x = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    n, p = x.shape
    k = D.shape[1]
    comps = list(range(k)) if components is None else sorted(components)
    s = D.sum(axis=0)
    q = threshold(level)
    full = nr.ml_unmix(X, D, H0, None, tol, max_pass, log_shift)
    H_ml, dev_ml, ok_full = full["H"], full["deviance"], full["converged"]
    lower, upper = np.full((k, p), np.nan), np.full((k, p), np.nan)
    conv, n_eval, n_pass = np.zeros((k, 2, p), dtype=bool), np.zeros((k, 2, p), dtype=np.int64), np.zeros((k, 2, p), dtype=np.int64)
    max_fit_pass = 0
    lift = None if k == 1 else x.sum(axis=0)[None, :] / ((k - 1) * s)[:, None] * pr.START
    for j in comps:
        rest = [i for i in range(k) if i != j]
        h_ml = H_ml[j]
        w0 = np.sqrt(q) * np.sqrt(s[j] * h_ml + q) / s[j]
        for side in (0, 1):
            up = side == 1
            out = upper[j] if up else lower[j]
            active = ok_full.copy()
            if up:
                lo, hi, t = h_ml.copy(), np.full(p, np.inf), h_ml + w0
            else:
                lo, hi, t = np.zeros(p), h_ml.copy(), np.zeros(p)
                zero = active & (h_ml == 0)
                out[zero], conv[j, side, zero] = 0.0, True
                active &= ~zero
            Hc = H_ml.copy()
            for ev in range(max_eval):
                idx = np.flatnonzero(active)
                if idx.size == 0:
                    break
                if rest:
                    Hc[rest] = np.maximum(Hc[rest], lift[rest])
                fit = ml_unmix_pinned(x[:, idx], D, j, t[idx], Hc[:, idx], rest, tol, max_pass, log_shift)
                Hc[:, idx] = fit["H"]
                n_eval[j, side, idx] += 1
                n_pass[j, side, idx] += fit["n_pass"]
                max_fit_pass = max(max_fit_pass, int(fit["n_pass"].max()))
                phi = fit["deviance"] - dev_ml[idx] - q
                fin = fit["converged"] & (np.abs(phi) <= lr_tol)
                if not up and ev == 0:
                    fin |= fit["converged"] & (phi <= 0)     # the boundary: the interval reaches 0
                out[idx[fin]] = t[idx[fin]]
                conv[j, side, idx[fin]] = True
                active[idx[fin | ~fit["converged"]]] = False
                go = ~fin & fit["converged"]
                ig = idx[go]
                tn, lo[ig], hi[ig] = _advance(t[ig], phi[go], fit["slope"][go], lo[ig], hi[ig], h_ml[ig], up)
                if not up and ev == 0:
                    tn = np.maximum(h_ml[ig] - w0[ig], 0.5 * h_ml[ig])
                t[ig] = tn
    return dict(H_ml=H_ml, deviance_ml=dev_ml, lower=lower, upper=upper, level=level, threshold=q, converged=conv, n_eval=n_eval, n_pass=n_pass,
                unmodelled=full["unmodelled"], nonfinite=0, max_fit_pass=max_fit_pass)


def flipped_intervals(X, D, **kw):
    """``intervals`` with the channels and the components in reverse order (the results in the caller's order): a second order of
    every sum."""
    out = intervals(np.asarray(X)[::-1], np.asarray(D)[::-1, ::-1], **kw)
    for key in ("H_ml", "lower", "upper", "converged", "n_eval", "n_pass"):
        out[key] = out[key][::-1]
    return out


def flipped_pinned(X, D, pin, t, H0=None, **kw):
    """``ml_unmix_pinned`` over all other components under the second summation order."""
    k = np.asarray(D).shape[1]
    out = ml_unmix_pinned(np.asarray(X)[::-1], np.asarray(D)[::-1, ::-1], k - 1 - pin, t, None if H0 is None else np.asarray(H0)[::-1], **kw)
    out["H"] = out["H"][::-1]
    return out


@functools.lru_cache(maxsize=None)
def solved(name, level=0.95):
    """``intervals`` of a named case from the default start, computed once and shared (treat as read-only)."""
    X, D = case(name)
    return intervals(X, D, level=level)


@functools.lru_cache(maxsize=None)
def full_optimum(name):
    """The full fit's long run: the Newton rule at tol = 1e-10 from the default start - a point certified by its own gap."""
    X, D = case(name)
    return nr.ml_unmix(X, D, None, None, 1e-10, 20000)


def pins(name):
    """The pinned values the pinned-fit tests use, for component ``pin`` = the last one: dict(label -> t (p,)) with
    t in {0, h_ml, 2 h_ml + 1, 10 N / s} - the last drives every free abundance to the boundary."""
    X, D = case(name)
    h = solved(name)["H_ml"][D.shape[1] - 1]
    N, s = np.asarray(X, dtype=np.float64).sum(axis=0), D.sum(axis=0)[-1]
    return dict(zero=np.zeros_like(h), ml=h.copy(), twice=2.0 * h + 1.0, far=10.0 * N / s)


LABELS = ("zero", "ml", "twice", "far")


@functools.lru_cache(maxsize=None)
def pinned(name, label, tol=1e-3):
    """The pinned fit of the LAST component of a case at one of ``pins``' values, over all the others, from the full solution: at the
    tests' tol within MAX_PASS, at any other (the long run: tol = 1e-10) within 20000.  Shared: treat as read-only."""
    X, D = case(name)
    return ml_unmix_pinned(X, D, D.shape[1] - 1, pins(name)[label], solved(name)["H_ml"], None, tol, MAX_PASS if tol == 1e-3 else 20000, history=True)
