"""The Newton rule of include/espm_mu.h ("pixel ML, Newton") restated in numpy, beside the EM rule of tests/pixel_ml_reference.py
whose cases, ``evaluate``, ``start_from`` and ``optimum`` it shares, and the two images the rule exists for.  Host only.

The rule, per pixel; x, N, M (m = |M|), s, log_shift, tol and the start are the EM rule's.  Extra state: e (k,), dev_acc = +inf,
tau = 1e-2, trial = 0.

    a pass  1-4  as in EM: hn = h N / sum_M s_j h_j; y = max(D hn, log_shift); w = x / y; dev; q = D^T w; r = q / s;
                 gap = 2 N (max_M r - 1); and in the same walk A_jl = sum_c d_cj d_cl x_c / y_c^2, j <= l in M
            5    REJECT, if trial and not dev <= dev_acc: h <- e, trial <- 0, tau <- min(10 tau, 1); the pass is counted; the reported
                 deviance and gap stay those of the accepted point
                 ACCEPT, otherwise: dev_acc <- dev; dev and gap are reported.  gap <= tol: done, h = hn frozen.  Else, in this order:
                 if trial, tau <- max(tau / 10, 1e-8); e_j <- hn_j r_j (the EM successor); g_j = s_j - q_j;
                 B = A_MM + tau diag(s_j / hn_j); B delta = -g by the root-free Cholesky B = L diag(p) L^T;
                 h_j <- max(hn_j + delta_j, 0.01 hn_j, 1e-30 N / s_j), trial <- 1; a pivot p_j that is not positive or not finite:
                 h <- e, trial <- 0 instead.  The pass is counted.

Why each piece is there: a step clamped at exactly zero is rejected for ever on a pixel with several abundances at the boundary (the
clamp of 0.01 hn is a fraction-to-boundary rule); A alone is singular where a pixel has fewer counts than components (the blend
with EM's own diagonal metric s_j / hn_j makes B positive definite); and after a rejected trial the stored EM successor of the
accepted point is a step that cannot raise the deviance.  The certificate is a property of the point, not of the path: it stays the
stop rule.

numpy sums in its own order where the kernel adds the channels one by one with fma: an accept / reject decision within rounding of a
tie may fall the other way, after which the two paths differ.  ``flipped`` is the second summation order on the host."""
import functools

import numpy as np

import pixel_ml_reference as pr
from pixel_ml_reference import LOG_SHIFT, evaluate, lines, mask_of, start_from  # noqa: F401  (shared with the GPU tests)

MAX_PASS = 128     # what the GPU tests pass as max_pass: the reference must converge everywhere within HALF of it
TAU0, TAU_MIN, TAU_MAX, TAU_STEP = 1e-2, 1e-8, 1.0, 10.0
THETA, H_FLOOR = 0.01, 1e-30


def _solve(B, g):
    """B delta = -g for a stack of symmetric systems (P, m, m), (P, m) by the root-free Cholesky B = L diag(d) L^T of the kernel:
    (delta (P, m), bad (P,): a pivot that is not positive or not finite)."""
    P, m = g.shape
    L = np.zeros((P, m, m))
    d = np.zeros((P, m))
    bad = np.zeros(P, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(m):
            dj = B[:, j, j] - np.einsum("pm,pm->p", L[:, j, :j] ** 2, d[:, :j])
            bad |= ~(dj > 0) | ~np.isfinite(dj)
            d[:, j] = dj
            for i in range(j + 1, m):
                L[:, i, j] = (B[:, i, j] - np.einsum("pm,pm,pm->p", L[:, i, :j], L[:, j, :j], d[:, :j])) / dj
        z = np.zeros((P, m))
        for j in range(m):   # L z = -g
            z[:, j] = -g[:, j] - np.einsum("pm,pm->p", L[:, j, :j], z[:, :j])
        z = z / d
        delta = np.zeros((P, m))
        for j in range(m - 1, -1, -1):   # L^T delta = z
            delta[:, j] = z[:, j] - np.einsum("pm,pm->p", L[:, j + 1:, j], delta[:, j + 1:])
    return delta, bad


def ml_unmix(X, D, H0=None, components=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT, history=False):
    """The Newton rule on every pixel of X (n, p): the dict of ``pixel_ml_reference.ml_unmix`` plus ``n_reject`` (p,).  ``history``:
    also ``monotone`` (p,) bool - the accepted deviances of the pixel never increased."""
    x = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    n, p = x.shape
    k = D.shape[1]
    M = mask_of(k, components)
    s = D.sum(axis=0)
    if not (s[M] > 0).all():
        raise ValueError("a component of the set has an all-zero spectrum")
    N = x.sum(axis=0)
    m = int(M.sum())
    H = np.zeros((k, p))
    if H0 is None:
        H[M] = N[None, :] / s[M].sum()
    else:
        H[M] = np.array(H0, dtype=np.float64)[M]
    with np.errstate(divide="ignore", invalid="ignore"):
        fill = N[None, :] / (m * s[:, None]) * pr.START
    bad = ~(H > 0) & M[:, None]
    H[bad] = fill[bad]
    done = N == 0
    H[:, done] = 0.0
    dev, gap = np.zeros(p), np.zeros(p)
    n_pass, n_reject = np.zeros(p, dtype=np.int64), np.zeros(p, dtype=np.int64)
    E = np.zeros((k, p))
    dev_acc, tau, trial = np.full(p, np.inf), np.full(p, TAU0), np.zeros(p, dtype=bool)
    monotone = np.ones(p, dtype=bool)
    unmodelled = 0
    DM, sM = D[:, M], s[M]
    live = np.flatnonzero(~done)
    for _ in range(max_pass):
        if live.size == 0:
            break
        h = H[:, live][M]
        h = h * (N[live] / (sM @ h))
        xl = x[:, live]
        Y = DM @ h
        floored = ~(Y >= log_shift)
        Y = np.where(floored, log_shift, Y)
        w = xl * (1.0 / Y)
        t = Y - xl
        pos = xl > 0
        t[pos] += xl[pos] * np.log(w[pos])
        dv = 2.0 * t.sum(axis=0)
        q = DM.T @ w
        r = q / sM[:, None]
        g = 2.0 * N[live] * (r.max(axis=0) - 1.0)
        rej = trial[live] & ~(dv <= dev_acc[live])
        acc = ~rej
        # rejected: the EM successor of the accepted point
        li = live[rej]
        H[:, li] = E[:, li]
        trial[li] = False
        tau[li] = np.minimum(tau[li] * TAU_STEP, TAU_MAX)
        n_reject[li] += 1
        # accepted
        la = live[acc]
        monotone[la] &= dv[acc] <= dev_acc[la]
        dev[la], gap[la], dev_acc[la] = dv[acc], g[acc], dv[acc]
        stop = acc & (g <= tol)
        Hs = np.zeros((k, int(stop.sum())))
        Hs[M] = h[:, stop]
        H[:, live[stop]] = Hs
        unmodelled += int((floored & pos)[:, stop].sum())
        done[live[stop]] = True
        go = acc & ~stop
        lg = live[go]
        if lg.size:
            hg = h[:, go]
            em = np.zeros((k, lg.size))
            em[M] = hg * r[:, go]
            E[:, lg] = em
            tau[lg] = np.where(trial[lg], np.maximum(tau[lg] / TAU_STEP, TAU_MIN), tau[lg])
            wy = w[:, go] * (1.0 / Y[:, go])   # x / y^2
            A = np.einsum("cj,cl,cq->qjl", DM, DM, wy)
            B = A
            with np.errstate(divide="ignore", over="ignore"):
                B[:, np.arange(m), np.arange(m)] += (tau[lg][None, :] * (sM[:, None] / hg)).T
            delta, singular = _solve(B, (sM[:, None] - q[:, go]).T)
            new = np.maximum(np.maximum(hg + delta.T, THETA * hg), H_FLOOR * N[lg][None, :] / sM[:, None])
            cand = np.zeros((k, lg.size))
            cand[M] = new
            cand[:, singular] = em[:, singular]
            H[:, lg] = cand
            trial[lg] = ~singular
        n_pass[live[~stop]] += 1
        live = live[~stop]
    out = dict(H=H, deviance=dev, gap=gap, n_pass=n_pass, converged=done.copy(), unmodelled=unmodelled, N=N, n_reject=n_reject)
    if history:
        out["monotone"] = monotone
    return out


def flipped(X, D, H0=None, components=None, **kw):
    """``ml_unmix`` with the channels and the components in reverse order (the results in the caller's order)."""
    k = np.asarray(D).shape[1]
    comp = None if components is None else [k - 1 - j for j in components]
    out = ml_unmix(np.asarray(X)[::-1], np.asarray(D)[::-1, ::-1], None if H0 is None else np.asarray(H0)[::-1], comp, **kw)
    out["H"] = out["H"][::-1]
    return out


def presence(X, D, H0=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """The nested fits of ``pixel_ml_reference.presence`` under the Newton rule: the one method for all k + 1 fits."""
    k = np.asarray(D).shape[1]
    full = ml_unmix(X, D, H0, None, tol, max_pass, log_shift)
    p = full["deviance"].size
    conv, gap, npass = [full["converged"]], [full["gap"]], [full["n_pass"]]
    without = np.empty((k, p))
    for j in range(k):
        if k == 1:
            without[j] = pr.empty_model_deviance(X, log_shift)
            conv.append(np.ones(p, dtype=bool)), gap.append(np.zeros(p)), npass.append(np.zeros(p, dtype=np.int64))
            continue
        start = full["H"].copy()
        start[j] = 0.0
        red = ml_unmix(X, D, start, [i for i in range(k) if i != j], tol, max_pass, log_shift)
        without[j] = red["deviance"]
        conv.append(red["converged"]), gap.append(red["gap"]), npass.append(red["n_pass"])
    lr = np.maximum(without - full["deviance"][None, :], 0.0)
    return dict(H_ml=full["H"], deviance_ml=full["deviance"], lr=lr, converged=np.stack(conv), gap=np.stack(gap), n_pass=np.stack(npass),
                deviance_without=without)


# ---- the images ---------------------------------------------------------------------------------------------------------------------------
def low8(n=64, p=400, k=8, dose=8.0, seed=5):
    """(X uint8 (n, p), D (n, k)): 8 counts per pixel over 8 components, half of the abundances zero - fewer counts than components in
    many pixels, several abundances at the boundary in most."""
    rng = np.random.default_rng(seed)
    D = lines(n, k)
    H = rng.random((k, p)) * (rng.random((k, p)) < 0.5)
    H[rng.integers(0, k, p), np.arange(p)] += 0.5
    H = dose * H / H.sum(axis=0)
    X = rng.poisson(D @ H).astype(np.uint8)
    X.setflags(write=False), D.setflags(write=False)
    return X, D


def collinear(n=64, p=300, seed=2):
    """(X uint8 (n, p), D (n, 4)): column 3 is 0.999 column 2 + 0.001 column 0 - a likelihood all but flat along one direction."""
    D = lines(n, 4).copy()
    D[:, 3] = 0.999 * D[:, 2] + 0.001 * D[:, 0]
    rng = np.random.default_rng(seed)
    X = rng.poisson(D @ (rng.random((4, p)) * 10.0)).astype(np.uint8)
    X.setflags(write=False), D.setflags(write=False)
    return X, D


NEW_CASES = ("low8", "collinear")
CASES = pr.CASES + NEW_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    """``pixel_ml_reference.case`` and the two images above:
    low8       64 channels x 400 pixels, k = 8, 8 counts per pixel: where a Newton step clamped at exactly zero stalls
    collinear  64 channels x 300 pixels, k = 4, two spectra 0.1 % apart: where EM does not converge within 20000 passes"""
    if name == "low8":
        return low8()
    if name == "collinear":
        return collinear()
    return pr.case(name)


@functools.lru_cache(maxsize=None)
def solved(name, tol=1e-3, max_pass=MAX_PASS):
    """The Newton rule on a case from ``start_from`` over all components, computed once and shared (treat as read-only)."""
    X, D = case(name)
    return ml_unmix(X, D, start_from(X, D), None, tol, max_pass, history=True)


@functools.lru_cache(maxsize=None)
def optimum(name):
    """dict(deviance (p,), gap (p,)) of the long run: ``pixel_ml_reference.optimum`` (EM at tol = 1e-10) for its own cases; for the two
    images above, where EM does not get there, the Newton rule at tol = 1e-10 - a point certified by its own gap, whatever the path."""
    if name in NEW_CASES:
        X, D = case(name)
        return ml_unmix(X, D, start_from(X, D), None, 1e-10, 20000)
    return pr.optimum(name)
