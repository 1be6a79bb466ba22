"""The spectra ML of espm_amd/spectra_ml.py restated in numpy: the sums of the device pass (include/espm_mu.h, "spectra ML pass")
straight from their definitions, the rule, the named cases its tests share, and the nested likelihood-ratio statistics.  Host only.
This file is the rule's definition, as tests/pixel_ml_newton_reference.py is for the pixel rule.

The problem: W (m, k) >= 0 with the dictionary G (n, m) and the abundances H (k, p) held, D = G W, y = max(D H, log_shift), the
Poisson deviance dev = 2 sum_cp (x ln(x / y) - x + y).  It is ONE pixel problem whose observations are all n p entries of X and whose
design columns are g_e (x) h_j.  a_ej = (G^T 1)_e (H 1)_j is that column's sum, N = sum x, F the free entries (``free``, less the
entries with a_ej = 0: ``inert``); entries outside F are exactly 0.

    start   W0 None: 1 on F.  An entry of F that is not > 0 becomes N / (|F| a_ej) * 1e-3 (the pixel rule's fill).
            tau = 1e-2, dev_acc = +inf, trial = False.  N = 0: W = 0, deviance 0, gap 0, done in 0 passes.
    a pass  1  W <- W N / sum_F a W                                             (the scale of least deviance on the ray)
            2  the device pass at D = G W: dev_c, Q (n, k), A_c (n, k, k), the unmodelled count (``sums``)
            3  q = G^T Q (m, k); r = q / a on F; dev = sum_c dev_c
            4  REJECT, if trial and not dev <= dev_acc: W <- e, trial <- False, tau <- min(10 tau, 1); next pass
            5  ACCEPT, otherwise: dev_acc <- dev, the point is reported; gap = 2 N (max_F r - 1); gap <= tol: done
            6  if trial: tau <- max(tau / 10, 1e-8)
            7  e <- W * r                                                          (the EM successor: the multiplicative W step, mu = 0)
            8  B = F_obs + tau diag(a / W) on F, F_obs[(e,i),(f,j)] = sum_c G_ce G_cf A_c,ij
            9  delta = B^-1 (q - a) by Cholesky; a factorisation or a delta that is not finite: W <- e, trial <- False, counted
            10 W <- max(W + delta, 0.01 W), trial <- True
    Every pass is counted, the certifying one included.  At the cap the last ACCEPTED point is reported.

THE CERTIFICATE.  dev is convex in W, its gradient is 2 (a - q), so for the minimiser W* over {W >= 0 on F}
    dev(W) - dev(W*) <= 2 sum_F (a - q) (W - W*) = 2 (sum_F a W - sum_F q W) + 2 sum_F (q - a) W*
                     <= 2 (N - sum_F q W) + 2 max_F (r - 1) sum_F a W*.
sum_F q W = sum_cp (x / y) (D H)_cp is the counts of the entries that are not floored, N - U with U the counts of the ``unmodelled``
entries; the same identity at W* (complementary slackness) gives sum_F a W* = N - U* <= N.  With no counts under the floor the
right side is gap = 2 N (max_F r - 1).  With counts under it, it is 2 U + gap (1 - U* / N) <= 2 U + max(gap, 0): the floored-model
caveat.  ``evaluate`` returns 2 U as ``certificate_slack`` and ``certificate_bound`` is the right side.
"""
import functools
import os

import numpy as np

import spectral_reference as sr

LOG_SHIFT = sr.LOG_SHIFT
EPS = sr.EPS
MAX_PASS = 64
TAU0, TAU_MIN, TAU_MAX, TAU_STEP = 1e-2, 1e-8, 1.0, 10.0
THETA, START = 0.01, 1e-3
C1, C2 = sr.C1, sr.C2   # the bounds of spectral_reference: deviance, and sums of p non-negative terms
# q and A, C4 = 4:  relative error <= C4 (p + k + 2) eps.  As for M under C2: y is k eps relative, the floor keeps it; q's term
# x / y h_j has the roundings of 1 / y, x i and the product (three), A's term those of 1 / y, x i, w i, h_r v and the product
# (five): two more than the (p + k + 3) eps of a term of M at most, (p + k + 5) eps for either side, twice that between two
# evaluations, and 2 (p + k + 5) <= 4 (p + k + 2) for p + k >= 1.  Nothing cancels: relative to the entry itself.
C4 = 4


def tri_index(k):
    """The lower triangle row by row: (0,0), (1,0), (1,1), (2,0), ... - the order of m_tri and a_tri."""
    return np.tril_indices(k)


def sums(X, D, H, log_shift=LOG_SHIFT):
    """The device pass from its definitions; X is (n, p).  dict(dev (n,), abs_terms (n,), xsum, ysum (n,), Q (n, k), A (n, k, k),
    unmodelled int, floored (n,) bool: the channels with a floored entry)."""
    X, D, H = (np.asarray(a, dtype=np.float64) for a in (X, D, H))
    Y = D @ H
    floored = ~(Y >= log_shift)
    Y = np.where(floored, log_shift, Y)
    w = X / Y
    pos = X > 0
    xl = np.zeros_like(X)
    xl[pos] = X[pos] * np.log(w[pos])
    t = xl - X + Y
    return dict(dev=2.0 * t.sum(axis=1), abs_terms=np.abs(t).sum(axis=1), xsum=X.sum(axis=1), ysum=Y.sum(axis=1), Q=w @ H.T,
                A=np.einsum("ip,jp,cp->cij", H, H, w / Y, optimize=True), unmodelled=int((floored & pos).sum()),
                floored=floored.any(axis=1))


def column_sums(G, H):
    """a (m, k) = (G^T 1)_e (H 1)_j."""
    return np.outer(np.asarray(G, dtype=np.float64).sum(axis=0), np.asarray(H, dtype=np.float64).sum(axis=1))


def free_set(G, H, free=None):
    """(F, inert): the entries the fit moves, and the free entries it cannot see (a_ej = 0)."""
    a = column_sums(G, H)
    free = np.ones(a.shape, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    return free & (a > 0), free & ~(a > 0)


def evaluate(X, G, H, W, free=None, log_shift=LOG_SHIFT):
    """Steps 2 - 5 at the given W, unscaled: dict(deviance, channel_deviance, gap, r (m, k), q (m, k), a, A, N, unmodelled,
    certificate_slack = 2 x the counts under the floor)."""
    X, G, H, W = (np.asarray(v, dtype=np.float64) for v in (X, G, H, W))
    F, _ = free_set(G, H, free)
    s = sums(X, G @ W, H, log_shift)
    a = column_sums(G, H)
    q = G.T @ s["Q"]
    r = np.zeros_like(a)
    r[F] = q[F] / a[F]
    N = X.sum()
    Y = (G @ W) @ H
    under = X[~(Y >= log_shift)].sum()
    return dict(deviance=s["dev"].sum(), channel_deviance=s["dev"], gap=2.0 * N * (r[F].max() - 1.0) if F.any() else 0.0, r=r, q=q, a=a,
                A=s["A"], N=N, unmodelled=s["unmodelled"], certificate_slack=2.0 * under)


def certificate_bound(gap, slack):
    """What dev - dev_opt is bounded by at a point with this gap and 2 U = ``slack`` (the module comment): gap itself without counts
    under the floor."""
    return gap if slack == 0 else slack + max(gap, 0.0)


def information(G, A):
    """F_obs (m k, m k), rows and columns (e, i) as e * k + i."""
    m, k = G.shape[1], A.shape[1]
    return np.einsum("ce,cf,cij->eifj", G, G, A, optimize=True).reshape(m * k, m * k)


def start_fill(W, F, a, N):
    """The start on F: entries that are not > 0 become N / (|F| a) * 1e-3; 0 outside F."""
    W = np.where(F, W, 0.0)
    bad = F & ~(W > 0)
    W[bad] = N / (F.sum() * a[bad]) * START
    return W


def ml_spectra(X, G, H, W0=None, free=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT, history=False):
    """The rule.  dict(W, deviance, channel_deviance, gap, n_pass, n_rejected, n_fallback, converged, inert, unmodelled, N); with
    ``history`` also ``accepted``: the list of (W, deviance, gap, unmodelled counts) of every accepted point."""
    X, G, H = (np.asarray(v, dtype=np.float64) for v in (X, G, H))
    m, k = G.shape[1], H.shape[0]
    a = column_sums(G, H)
    F, inert = free_set(G, H, free)
    if not F.any():
        raise ValueError("no free entry of W that the model can see")
    N = X.sum()
    out = dict(W=np.zeros((m, k)), deviance=0.0, channel_deviance=np.zeros(G.shape[0]), gap=0.0, n_pass=0, n_rejected=0, n_fallback=0,
               converged=True, inert=inert, unmodelled=0, N=N)
    track = []
    if history:
        out["accepted"] = track
    if N == 0:
        return out
    W = start_fill(np.ones((m, k)) if W0 is None else np.array(W0, dtype=np.float64), F, a, N)
    idx = np.flatnonzero(F.ravel())
    tau, dev_acc, trial, e = TAU0, np.inf, False, None
    out["converged"] = False
    for _ in range(max_pass):
        W = W * (N / (a[F] @ W[F]))
        s = sums(X, G @ W, H, log_shift)
        q = G.T @ s["Q"]
        dev = s["dev"].sum()
        out["n_pass"] += 1
        if trial and not dev <= dev_acc:
            W, trial, tau = e, False, min(tau * TAU_STEP, TAU_MAX)
            out["n_rejected"] += 1
            continue
        r = np.zeros_like(a)
        r[F] = q[F] / a[F]
        gap = 2.0 * N * (r[F].max() - 1.0)
        dev_acc = dev
        out.update(W=W.copy(), deviance=dev, channel_deviance=s["dev"], gap=gap, unmodelled=s["unmodelled"])
        if history:
            track.append((W.copy(), dev, gap, s["unmodelled"]))
        if gap <= tol:
            out["converged"] = True
            break
        if trial:
            tau = max(tau / TAU_STEP, TAU_MIN)
        e = W * r
        with np.errstate(all="ignore"):
            B = information(G, s["A"])[np.ix_(idx, idx)]
            B[np.arange(idx.size), np.arange(idx.size)] += tau * (a[F] / W[F])
            try:
                L = np.linalg.cholesky(B)
                z = np.linalg.solve(L, (q - a)[F])
                delta = np.linalg.solve(L.T, z)
                ok = bool(np.isfinite(delta).all())
            except np.linalg.LinAlgError:
                ok = False
        if not ok:
            W, trial = e, False
            out["n_fallback"] += 1
            continue
        step = W.copy()
        step[F] = np.maximum(W[F] + delta, THETA * W[F])
        W, trial = step, True
    return out


def em(X, G, H, W0=None, free=None, n_iter=20000, log_shift=LOG_SHIFT, stop=1e-10):
    """The long EM run W <- W * r (scaled onto the ray each pass), which cannot fail: dict(W, deviance, gap, n_iter).  It stops early
    when its own certificate, less the floored-model slack, is below ``stop``."""
    X, G, H = (np.asarray(v, dtype=np.float64) for v in (X, G, H))
    a = column_sums(G, H)
    F, _ = free_set(G, H, free)
    N = X.sum()
    if N == 0 or not F.any():
        return dict(W=np.zeros(a.shape), deviance=0.0, gap=0.0, n_iter=0)
    W = start_fill(np.ones(a.shape) if W0 is None else np.array(W0, dtype=np.float64), F, a, N)
    for it in range(n_iter):
        s = sums(X, G @ W, H, log_shift)
        q = G.T @ s["Q"]
        r = np.zeros_like(a)
        r[F] = q[F] / a[F]
        # unscaled EM: at its fixed point sum_F a W = the modelled counts, and r = 1 on the support
        gap = 2.0 * (a[F] @ W[F]) * (r[F].max() - 1.0)
        if it > 0 and abs((a[F] - q[F]) @ W[F]) <= stop and gap <= stop:
            break
        W = W * r
    return dict(W=W, deviance=s["dev"].sum(), gap=gap, n_iter=it)


def presence(X, G, H, W0=None, free=None, entries=None, tol=1e-3, max_pass=MAX_PASS, log_shift=LOG_SHIFT):
    """The nested fits: the full one, then for every tested entry the fit without it, warm-started at the full solution.  dict(W_ml,
    deviance_ml, lr (m, k), pvalue (m, k), entries (E, 2), converged, gap, n_pass (1 + E,), deviance_without (m, k))."""
    import pixel_ml_reference as pr
    full = ml_spectra(X, G, H, W0, free, tol, max_pass, log_shift)
    F, _ = free_set(G, H, free)
    ent = np.argwhere(F) if entries is None else np.asarray(entries, dtype=np.int64).reshape(-1, 2)
    lr = np.full(F.shape, np.nan)
    without = np.full(F.shape, np.nan)
    conv, gap, npass = [full["converged"]], [full["gap"]], [full["n_pass"]]
    for e, j in ent:
        sub = F.copy()
        sub[e, j] = False
        if not F[e, j] or not sub.any():
            conv.append(True), gap.append(0.0), npass.append(0)
            continue
        red = ml_spectra(X, G, H, full["W"], sub, tol, max_pass, log_shift)
        without[e, j] = red["deviance"]
        lr[e, j] = max(red["deviance"] - full["deviance"], 0.0)
        conv.append(red["converged"]), gap.append(red["gap"]), npass.append(red["n_pass"])
    pv = np.full(F.shape, np.nan)
    ok = ~np.isnan(lr)
    pv[ok] = pr.pvalue(lr[ok])
    return dict(W_ml=full["W"], deviance_ml=full["deviance"], lr=lr, pvalue=pv, entries=ent, converged=np.array(conv, dtype=bool),
                gap=np.array(gap), n_pass=np.array(npass, dtype=np.int64), deviance_without=without)


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------------------------
# name: (n, p, k, m).  The smallest shapes that cross the seams: one channel past a block of 256, one pixel past a chunk of 2048,
# partial 64-, 32- and 16-pixel tiles, k = 1 and k = 8.
SHAPES = {"k3": (96, 300, 3, 6), "k5": (300, 2125, 5, 6), "k8": (64, 130, 8, 4), "k1": (40, 70, 1, 3), "seams": (257, 2049, 2, 5)}
PLANTED_AT = ((1, 2), (4, 0))   # the entries of W planted at zero in "planted" (the shape of "k5")
CASES = tuple(SHAPES) + ("planted",)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X (n, p) uint8, G (n, m), W (m, k) the truth, H (k, p)), read-only: ``spectral_reference.dict_image`` at the shape of the name -
    with its pixel without counts, its all-zero channel and its zero row of G with one counted entry (so ``unmodelled`` is 1) - and
    "planted": "k5" with the entries PLANTED_AT of W at zero and X redrawn."""
    if name == "planted":
        n, p, k, m = SHAPES["k5"]
        X, G, W, H, facts = sr.dict_image(n, p, k, np.uint8, m)
        W = np.array(W)
        for e, j in PLANTED_AT:
            W[e, j] = 0.0
        rng = np.random.default_rng(77)
        X = np.minimum(rng.poisson(G @ W @ H), 255).astype(np.uint8)
        X[:, facts["empty_pixel"]] = 0
        X[facts["zero_channel"], :] = 0
        X[facts["floor_channel"], :] = 0
        X[facts["floor_channel"], facts["floor_pixel"]] = 3
        X.setflags(write=False), W.setflags(write=False)
        return X, G, W, H
    n, p, k, m = SHAPES[name]
    return sr.dict_image(n, p, k, np.uint8, m)[:4]


@functools.lru_cache(maxsize=None)
def solved(name, tol=1e-3, max_pass=MAX_PASS):
    """The rule on a case from W = 1, computed once and shared (treat as read-only), with the accepted points."""
    X, G, _, H = case(name)
    return ml_spectra(X, G, H, None, None, tol, max_pass, history=True)


@functools.lru_cache(maxsize=None)
def tested(name):
    """``presence`` of a case over all its entries, shared."""
    X, G, _, H = case(name)
    return presence(X, G, H)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectra_ml_optimum.npz")


def rigorous_gap(ev, W, F):
    """2 sum_F (a - q) W + 2 N max(max_F r - 1, 0): the certificate without the scale onto the ray and without the caveat (the first
    term is 2 U at a scaled point), from an ``evaluate`` at W."""
    return 2.0 * float((ev["a"][F] - ev["q"][F]) @ W[F]) + 2.0 * ev["N"] * max(ev["r"][F].max() - 1.0, 0.0)


@functools.lru_cache(maxsize=None)
def optimum(name):
    """dict(W, deviance, gap): the end of the long EM run from W = 1 (``em``: up to 40000 passes over the case, minutes at the
    larger shapes), which ``python tests/spectra_ml_reference.py`` recorded in tests/golden/spectra_ml_optimum.npz.  The record is not
    trusted: the point is evaluated here from the definitions, and its own rigorous certificate says how far above the minimum
    its deviance can be - at most 1e-4, a tenth of the tolerance the tests run at."""
    X, G, _, H = case(name)
    with np.load(GOLDEN) as f:
        W = f[name]
    ev = evaluate(X, G, H, W)
    F, _ = free_set(G, H)
    gap = rigorous_gap(ev, W, F)
    assert (W >= 0).all() and not W[~F].any() and 0 <= gap <= 1e-4, f"{name}: the recorded optimum is certified to {gap:.3g} only"
    return dict(W=W, deviance=ev["deviance"], gap=gap)


def _record(name):
    X, G, _, H = case(name)
    return name, em(X, G, H, n_iter=40000)["W"]


if __name__ == "__main__":
    import multiprocessing as mp
    with mp.Pool(len(CASES)) as pool:
        np.savez(GOLDEN, **dict(pool.map(_record, CASES)))
    for c in CASES:
        print(c, optimum(c)["gap"])

