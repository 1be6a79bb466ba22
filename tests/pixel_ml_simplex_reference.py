"""The simplex rule of include/espm_mu.h ("pixel ML, simplex") and the root finder of ``espm_amd.presence.intervals(simplex=True)``
restated in numpy, beside the pinned rule of tests/pixel_ml_pinned_reference.py whose cases (brought to the data's dose), accept /
reject test and Cholesky it shares.  Host only.  This file is the rule's definition; the kernel follows its operation order.

The problem, per pixel with counts x, spectra D (n, k), column sums s, fitted set M (m = |M|) and an optional pinned component
``pin`` outside M held at t in [0, 1]: minimise f = 2 sum_c (x ln(x / y) - x + y), y = max(D h, log_shift), over h_M >= 0,
sum_M h = total, total = 1 - t (1 without a pin); h_pin = t, h = 0 elsewhere.  There is no free scale: no step onto the ray, no N.

    bad t   negative, above 1 or not finite: the pixel stops at once, not converged, counted in ``nonfinite``
    start   h_j <- max(h0_j, 1e-3 total / m) over M, then h_M <- h_M (total / sum_M h); no start: total / m; m == 1 or total == 0:
            h_M = total exactly.  e = 0, dev_acc = +inf, tau = 1e-2, trial = 0
    a pass  y over all k components, the floor, w = x / y, dev, q = D^T w, A = D^T diag(x / y^2) D (the pinned rule's walk)
            g = s - q;  lin = sum_M g_j h_j;  hq = sum_M h_j q_j;  gmin = min_M g_j
            gap = 2 (lin - total gmin), 0 with M empty                      (a Frank-Wolfe gap: f(h) - f* <= grad . (h - h*), and
                                                                              grad . h* >= 2 total gmin over the scaled simplex)
            slope = 2 (g_pin - lin / total); 2 (g_pin - gmin) where total == 0; 2 g_pin with M empty   (the envelope theorem: the
                                                                              multiplier of the sum is -2 lin / total at the optimum)
            dev or gap not finite: stopped, not converged, counted
            REJECT (trial and not dev <= dev_acc): h_M <- e, trial <- 0, tau <- min(10 tau, 1); the pass is counted
            ACCEPT: dev, gap, slope reported, dev_acc <- dev.  gap <= tol: done.  Else
              hq == 0 (no count that M models: f is linear in h_M, its gradient 2 s): h <- total at argmin_M s (lowest index on
              ties), e <- h, trial <- 0; counted; the next pass certifies with gap = 0 exactly.  Else
              if trial, tau <- max(tau / 10, 1e-8)
              e: n_j = h_j q_j / total; over P = {n_j > 0}: nu_0 = max_P (n_j - s_j); Newton on psi(nu) = sum_P n_j / (s_j + nu) - 1
                 (convex, decreasing, psi(nu_0) >= 0: the iteration rises) until a step no longer raises nu, at most 64;
                 e_j = total n_j / (s_j + nu), 0 off P; e <- e (total / sum e)           (the multiplicative step under the simplex)
              trial: over the ACTIVE set {j in M: h_j > 0} B = A, B_jj += tau max(q_j, s_j) / h_j; identity rows elsewhere; one
                 root-free Cholesky; u = B^-1 (-g), v = B^-1 1; delta = u - (sum u / sum v) v;
                 h_j <- max(h_j + delta_j, 0.01 h_j), then h <- h (total / sum h); trial <- 1.  A pivot that is no pivot or an h that
                 is not finite: h <- e, trial <- 0.  The pass is counted.

sum_M h = total to within k ulps of total after every step: each of the m products h_j (total / sum) rounds once, and the
sum behind the scale rounds m - 1 times; adding the m rounded values up again to check costs as much again, so a recomputed sum is
within 2 k eps total.

The root finder is tests/pixel_ml_pinned_reference.py's with the bracket capped at 1: every candidate t is min(., 1); a point at t = 1
with phi <= 0 finishes with upper == 1 exactly; h_ml >= 1 gives upper = 1 with no evaluation.  The warm start needs no lift of its
own: the rule's start lifts to 1e-3 total / (k - 1) and rescales to the new total.  The empty pixel takes the general path."""
import functools

import numpy as np

import pixel_ml_newton_reference as nr
import pixel_ml_pinned_reference as pp
from pixel_ml_newton_reference import TAU0, TAU_MAX, TAU_MIN, TAU_STEP, THETA, _solve
from pixel_ml_pinned_reference import MAX_EVAL, MAX_PASS, _advance, threshold  # noqa: F401  (shared with the GPU tests)
from pixel_ml_reference import LOG_SHIFT, START, mask_of  # noqa: F401

NU_ITER = 64
EPS = float(np.finfo(np.float64).eps)
MISFIT = ("bright3", "dim03")
CASES = pp.CASES + ("img96_k8",) + MISFIT + ("zero_row",)


def sum_bound(k, total):
    """What a recomputed sum_M h may differ from ``total`` by: 2 k eps total (module docstring)."""
    return 2.0 * k * EPS * np.abs(total)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X (n, p) read-only, D (n, k)): a case of the pinned tests with D multiplied by the scalar that makes mean_p N = mean_j s_j (the
    simplex model at the data's dose), and
    img96_k8   the same for pixel_ml_reference's k = 8 image: where register pressure is highest
    bright3    ``planted`` with D a further factor 3 too bright;  dim03: 0.3, too dim (a misfit dose)
    zero_row   ``planted`` with channel 0 of D zeroed and no count there but in the LAST pixel, which has counts nowhere else"""
    base = "planted" if name in MISFIT + ("zero_row",) else name
    X, D = nr.case(base)
    X, D = np.array(X), np.array(D, dtype=np.float64)
    if name == "zero_row":
        D[0] = 0.0
        X[0] = 0
        X[:, -1] = 0
        X[0, -1] = 5
    D = D * (X.sum(axis=0, dtype=np.float64).mean() / D.sum(axis=0).mean())
    D = D * {"bright3": 3.0, "dim03": 0.3}.get(name, 1.0)
    X.setflags(write=False), D.setflags(write=False)
    return X, D


def _sets(k, pin, components):
    if pin is None:
        M = mask_of(k, components)
        if not M.any():
            raise ValueError("an empty set and nothing pinned")
    else:
        M = mask_of(k, [j for j in range(k) if j != pin] if components is None else components)
        if M[pin]:
            raise ValueError("the pinned component is in the set")
    return M


def _asc(rows):
    """The rows added up one by one, ascending: (L,)."""
    out = np.zeros(rows.shape[1])
    for r in rows:
        out = out + r
    return out


def evaluate(X, D, H, pin=None, components=None, log_shift=LOG_SHIFT):
    """Deviance, gap, slope and sum_M h of the simplex rule at the given H (k, p), recomputed: dict(deviance, gap, slope, sum, total,
    scale (p,)).  ``total`` is 1 - H[pin]; ``slope`` is NaN without a pin.  ``scale``: max over M and pin of s_j + q_j, the magnitude
    whose rounding a recomputed g = s - q carries: gap and slope are sums of a few such terms with weights that add up to at most
    ``total`` <= 1 (gap), and to 1 (slope)."""
    x = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    k, p = H.shape
    M = _sets(k, pin, components)
    s = D.sum(axis=0)
    total = np.ones(p) if pin is None else 1.0 - H[pin]
    Y = D @ H
    Y = np.where(Y >= log_shift, Y, log_shift)
    w = x * (1.0 / Y)
    t = Y - x
    pos = x > 0
    t[pos] += x[pos] * np.log(w[pos])
    q = D.T @ w
    g = s[:, None] - q
    big = M.copy()
    if pin is not None:
        big[pin] = True
    scale = (s[:, None] + q)[big].max(axis=0)
    lin = (g[M] * H[M]).sum(axis=0)
    if M.any():
        gmin = g[M].min(axis=0)
        gap = 2.0 * (lin - total * gmin)
    else:
        gmin, gap = np.full(p, np.inf), np.zeros(p)
    slope = np.full(p, np.nan)
    if pin is not None:
        with np.errstate(all="ignore"):
            slope = 2.0 * (g[pin] if not M.any() else np.where(total == 0, g[pin] - gmin, g[pin] - lin / total))
    return dict(deviance=2.0 * t.sum(axis=0), gap=gap, slope=slope, sum=H[M].sum(axis=0), total=total, scale=scale)


def _em_successor(hg, qg, sg, totg, M):
    """e (k, G): the multiplicative step under sum_M e = total, the multiplier by Newton from the left."""
    with np.errstate(all="ignore"):
        nj = np.where(M[:, None], (hg * qg) * (1.0 / totg)[None, :], 0.0)
        P = nj > 0
        nu = np.where(P, nj - sg[:, None], -np.inf).max(axis=0)
        rising = np.ones(nu.size, dtype=bool)
        for _ in range(NU_ITER):
            iv = 1.0 / (sg[:, None] + nu[None, :])
            c = np.where(P, nj * iv, 0.0)
            nxt = nu + (_asc(c) - 1.0) / _asc(c * iv)
            rising &= nxt > nu
            if not rising.any():
                break
            nu = np.where(rising, nxt, nu)
        e = np.where(P, totg[None, :] * (nj * (1.0 / (sg[:, None] + nu[None, :]))), 0.0)
        return e * (totg / _asc(e))[None, :]


def ml_unmix(X, D, H0=None, components=None, pin=None, t=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT, history=False):
    """The simplex rule on every pixel of X (n, p): dict(H, deviance, gap, slope, n_pass, converged, nonfinite, unmodelled, n_reject,
    total) and with ``history`` also ``monotone``.  ``pin`` None: nothing pinned (``slope`` stays 0); else ``t``: a scalar or (p,).
    ``components``: the fitted set (None: all, or all but ``pin``)."""
    x = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    n, p = x.shape
    k = D.shape[1]
    M = _sets(k, pin, components)
    s = D.sum(axis=0)
    if not (s[M] > 0).all() or (pin is not None and not s[pin] > 0):
        raise ValueError("a component of the set, or the pinned one, has an all-zero spectrum")
    m = int(M.sum())
    tt = np.zeros(p) if pin is None else np.broadcast_to(np.asarray(t, dtype=np.float64), (p,)).copy()
    nonfin = ~((tt >= 0) & (tt <= 1))
    total = 1.0 - tt
    H = np.zeros((k, p))
    if m:
        with np.errstate(all="ignore"):
            hm = np.full((m, p), 1.0 / m) if H0 is None else np.array(H0, dtype=np.float64)[M]
            hm = np.maximum(hm, (START * total / m)[None, :])
            hm = hm * (total / _asc(hm))[None, :]
            if m == 1:
                hm[:] = total
            hm[:, total == 0] = 0.0
        H[M] = hm
    if pin is not None:
        H[pin] = tt
    if nonfin.any():   # (as the call found them)
        H[:, nonfin] = 0.0 if H0 is None else np.asarray(H0, dtype=np.float64)[:, nonfin]
    done = nonfin.copy()
    conv = np.zeros(p, dtype=bool)
    dev, gap, slope = np.zeros(p), np.zeros(p), np.zeros(p)
    n_pass, n_reject = np.zeros(p, dtype=np.int64), np.zeros(p, dtype=np.int64)
    E = np.zeros((k, p))
    dev_acc, tau, trial = np.full(p, np.inf), np.full(p, TAU0), np.zeros(p, dtype=bool)
    monotone = np.ones(p, dtype=bool)
    unmodelled, n_nonfin = 0, int(nonfin.sum())
    Mi = np.flatnonzero(M)
    best = int(Mi[np.argmin(s[Mi])]) if m else -1
    live = np.flatnonzero(~done)
    for _ in range(max_pass):
        if live.size == 0:
            break
        h = H[:, live]
        xl = x[:, live]
        tot = total[live]
        Y = D @ h
        floored = ~(Y >= log_shift)
        Y = np.where(floored, log_shift, Y)
        w = xl * (1.0 / Y)
        tm = Y - xl
        pos = xl > 0
        tm[pos] += xl[pos] * np.log(w[pos])
        dv = 2.0 * tm.sum(axis=0)
        q = D.T @ w
        g = s[:, None] - q
        lin, hq = _asc(g[M] * h[M]), _asc(h[M] * q[M])
        with np.errstate(all="ignore"):
            if m:
                gmin = g[M].min(axis=0)
                gp_ = 2.0 * (lin - tot * gmin)
            else:
                gmin, gp_ = np.full(live.size, np.inf), np.zeros(live.size)
            if pin is None:
                sl = np.zeros(live.size)
            else:
                sl = 2.0 * (g[pin] if m == 0 else np.where(tot == 0, g[pin] - gmin, g[pin] - lin / tot))
        broken = ~np.isfinite(dv) | ~np.isfinite(gp_)
        lb = live[broken]
        dev[lb], gap[lb], slope[lb] = dv[broken], gp_[broken], sl[broken]
        n_nonfin += int(broken.sum())
        rej = ~broken & trial[live] & ~(dv <= dev_acc[live])
        acc = ~broken & ~rej
        li = live[rej]
        H[:, li] = E[:, li]
        if pin is not None:
            H[pin, li] = tt[li]
        trial[li] = False
        tau[li] = np.minimum(tau[li] * TAU_STEP, TAU_MAX)
        n_reject[li] += 1
        la = live[acc]
        monotone[la] &= dv[acc] <= dev_acc[la]
        dev[la], gap[la], slope[la], dev_acc[la] = dv[acc], gp_[acc], sl[acc], dv[acc]
        stop = acc & (gp_ <= tol)
        done[live[stop]] = True
        conv[live[stop]] = True
        unmodelled += int((floored & pos)[:, stop].sum())
        vert = acc & ~stop & (hq == 0)
        lv = live[vert]
        if lv.size:
            hv = np.zeros((k, lv.size))
            hv[best] = tot[vert]
            E[:, lv] = hv
            if pin is not None:
                hv[pin] = tt[lv]
            H[:, lv] = hv
            trial[lv] = False
        go = acc & ~stop & ~vert
        lg = live[go]
        if lg.size:
            hg, qg, totg = h[:, go], q[:, go], tot[go]
            tau[lg] = np.where(trial[lg], np.maximum(tau[lg] / TAU_STEP, TAU_MIN), tau[lg])
            em = _em_successor(hg, qg, s, totg, M)
            E[:, lg] = em
            act = M[:, None] & (hg > 0)
            wy = w[:, go] * (1.0 / Y[:, go])
            B = np.einsum("cj,cl,cq->qjl", D, D, wy)
            pair = act.T[:, :, None] & act.T[:, None, :]
            B[~pair] = 0.0
            idx = np.arange(k)
            with np.errstate(all="ignore"):
                B[:, idx, idx] = np.where(act, B[:, idx, idx].T + tau[lg][None, :] * (np.maximum(qg, s[:, None]) / hg), 1.0).T
                u, singular = _solve(B, np.where(act, g[:, go], 0.0).T)
                v, _ = _solve(B, -act.T.astype(np.float64))
                mult = _asc(u.T) / _asc(v.T)
                delta = u.T - mult[None, :] * v.T
                cand = np.where(act, np.maximum(hg + delta, THETA * hg), 0.0)
                cand = cand * (totg / _asc(cand))[None, :]
            singular = singular | ~np.isfinite(cand).all(axis=0)
            cand[:, singular] = em[:, singular]
            if pin is not None:
                cand[pin] = tt[lg]
            H[:, lg] = cand
            trial[lg] = ~singular
        keep = ~stop & ~broken
        n_pass[live[keep]] += 1
        done[lb] = True
        live = live[keep]
    out = dict(H=H, deviance=dev, gap=gap, slope=slope, n_pass=n_pass, converged=conv, nonfinite=n_nonfin, unmodelled=unmodelled,
               n_reject=n_reject, total=total)
    if history:
        out["monotone"] = monotone
    return out


def flipped(X, D, H0=None, pin=None, t=None, **kw):
    """``ml_unmix`` over the default set with the channels and the components in reverse order (the results in the caller's order): a
    second order of every sum."""
    k = np.asarray(D).shape[1]
    out = ml_unmix(np.asarray(X)[::-1], np.asarray(D)[::-1, ::-1], None if H0 is None else np.asarray(H0)[::-1], None,
                   None if pin is None else k - 1 - pin, t, **kw)
    out["H"] = out["H"][::-1]
    return out


def presence(X, D, H0=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """The nested fits under the simplex: the full fit and, for every j, the fit over M \\ {j} with sum 1 from the full solution with row
    j zeroed (the rule's start rescales it); lr = 0 exactly where the full fit has h_j == 0.  k = 1: ValueError, nothing is fitted under the simplex."""
    k = np.asarray(D).shape[1]
    if k == 1:
        raise ValueError("one component: nothing is fitted under the simplex")
    full = ml_unmix(X, D, H0, None, None, None, tol, max_pass, log_shift)
    p = full["deviance"].size
    conv, gap, npass = [full["converged"]], [full["gap"]], [full["n_pass"]]
    without = np.empty((k, p))
    for j in range(k):
        start = full["H"].copy()
        start[j] = 0.0
        red = ml_unmix(X, D, start, [i for i in range(k) if i != j], None, None, tol, max_pass, log_shift)
        without[j] = red["deviance"]
        conv.append(red["converged"]), gap.append(red["gap"]), npass.append(red["n_pass"])
    # where the full fit has h_j == 0 its point is a point of the reduced problem: the reduced minimum is not above it, lr is 0 (the
    # rule's start lifts the zeros of that point, so the reduced fit may certify within tol ABOVE it)
    lr = np.where(full["H"] == 0, 0.0, np.maximum(without - full["deviance"][None, :], 0.0))
    return dict(H_ml=full["H"], deviance_ml=full["deviance"], lr=lr, converged=np.stack(conv), gap=np.stack(gap), n_pass=np.stack(npass),
                deviance_without=without)


def intervals(X, D, H0=None, level=0.95, components=None, tol=1e-3, lr_tol=1e-2, max_eval=MAX_EVAL, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """``espm_amd.presence.intervals(simplex=True)`` on the host: the same dict, plus ``max_fit_pass`` - the most passes any single
    pinned fit took."""
    x = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    n, p = x.shape
    k = D.shape[1]
    comps = list(range(k)) if components is None else sorted(components)
    s = D.sum(axis=0)
    q = threshold(level)
    full = ml_unmix(X, D, H0, None, None, None, tol, max_pass, log_shift)
    H_ml, dev_ml, ok_full = full["H"], full["deviance"], full["converged"]
    lower, upper = np.full((k, p), np.nan), np.full((k, p), np.nan)
    conv, n_eval, n_pass = np.zeros((k, 2, p), dtype=bool), np.zeros((k, 2, p), dtype=np.int64), np.zeros((k, 2, p), dtype=np.int64)
    max_fit_pass = 0
    for j in comps:
        rest = [i for i in range(k) if i != j]
        h_ml = H_ml[j]
        w0 = np.sqrt(q) * np.sqrt(s[j] * h_ml + q) / s[j]
        for side in (0, 1):
            up = side == 1
            out = upper[j] if up else lower[j]
            active = ok_full.copy()
            if up:
                lo, hi, t = h_ml.copy(), np.full(p, np.inf), np.minimum(h_ml + w0, 1.0)
                one = active & (h_ml >= 1)
                out[one], conv[j, side, one] = 1.0, True
                active &= ~one
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
                fit = ml_unmix(x[:, idx], D, Hc[:, idx], rest, j, t[idx], tol, max_pass, log_shift)
                Hc[:, idx] = fit["H"]
                n_eval[j, side, idx] += 1
                n_pass[j, side, idx] += fit["n_pass"]
                max_fit_pass = max(max_fit_pass, int(fit["n_pass"].max()))
                phi = fit["deviance"] - dev_ml[idx] - q
                fin = fit["converged"] & (np.abs(phi) <= lr_tol)
                if up:
                    fin |= fit["converged"] & (t[idx] == 1) & (phi <= 0)     # the cap: the interval reaches 1
                elif ev == 0:
                    fin |= fit["converged"] & (phi <= 0)     # the boundary: the interval reaches 0
                out[idx[fin]] = t[idx[fin]]
                conv[j, side, idx[fin]] = True
                active[idx[fin | ~fit["converged"]]] = False
                go = ~fin & fit["converged"]
                ig = idx[go]
                tn, lo[ig], hi[ig] = _advance(t[ig], phi[go], fit["slope"][go], lo[ig], hi[ig], h_ml[ig], up)
                if up:
                    tn = np.minimum(tn, 1.0)
                elif ev == 0:
                    tn = np.maximum(h_ml[ig] - w0[ig], 0.5 * h_ml[ig])
                t[ig] = tn
    return dict(H_ml=H_ml, deviance_ml=dev_ml, lower=lower, upper=upper, level=level, threshold=q, converged=conv, n_eval=n_eval, n_pass=n_pass,
                unmodelled=full["unmodelled"], nonfinite=full["nonfinite"], max_fit_pass=max_fit_pass)


# ---- shared, computed once (treat as read-only) ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solved(name, tol=1e-3):
    """The full simplex fit of a case from the default start: at the tests' tol within MAX_PASS, at any other (the long run:
    tol = 1e-10) within 20000."""
    X, D = case(name)
    return ml_unmix(X, D, tol=tol, max_pass=MAX_PASS if tol == 1e-3 else 20000, history=True)


def pins(name):
    """The pinned values of the pinned-fit tests, for ``pin`` = the last component: dict(label -> t (p,)) with t in {0, h_ml, the
    midpoint of h_ml and 1, 1}."""
    h = solved(name)["H"][-1]
    return dict(zero=np.zeros_like(h), ml=h.copy(), mid=0.5 * (h + 1.0), one=np.ones_like(h))


LABELS = ("zero", "ml", "mid", "one")


@functools.lru_cache(maxsize=None)
def pinned(name, label, tol=1e-3):
    """The pinned simplex fit of the LAST component of a case at one of ``pins``' values, over all the others, from the full solution."""
    X, D = case(name)
    k = D.shape[1]
    return ml_unmix(X, D, solved(name)["H"], None, k - 1, pins(name)[label], tol, MAX_PASS if tol == 1e-3 else 20000, history=True)


@functools.lru_cache(maxsize=None)
def presence_solved(name):
    X, D = case(name)
    return presence(X, D)


@functools.lru_cache(maxsize=None)
def intervals_solved(name, level=0.95):
    X, D = case(name)
    return intervals(X, D, level=level)
