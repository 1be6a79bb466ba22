"""The pixel ML rule of include/espm_mu.h ("pixel ML") restated in numpy, the images its tests use, and the nested likelihood-ratio
statistics of espm_amd/presence.py built from it.  Host only.

The rule, per pixel with counts x (n,), spectra D (n, k), component set M and s_j = sum_c d_cj, N = sum_c x_c:

    start   h_j = 0 outside M; inside M a start that is not > 0 becomes N / (|M| s_j) * 1e-3 (no start given: N / sum_M s, as
            espm_amd.presence passes it)
    a pass  1  S = sum_{j in M} s_j h_j; h <- h N / S
            2  y = max(D h, log_shift); w = x / y; dev = 2 sum_c (x ln(x / y) - x + y) (the log where x > 0); q = D^T w
            3  r_j = q_j / s_j, j in M
            4  gap = 2 N (max_{j in M} r_j - 1)
            5  gap <= tol: done, h (as scaled in 1), dev, gap and the pass count frozen; else h_j <- h_j r_j and one pass more
    N = 0   done at once: h = 0, dev = 0, gap = 0, no pass

numpy adds in its own order (BLAS, pairwise sums) where the kernel adds the channels one by one with fma: the two agree to rounding,
not bit for bit, and a pixel within rounding of the threshold may stop a pass apart.  ``flipped`` runs the same rule on the channels
and components in reverse order - a second summation order on the host, the yardstick for how often that happens."""
import functools

import numpy as np

LOG_SHIFT = 1e-14
START = 1e-3


def mask_of(k, components=None):
    """The component set as a bool (k,) array: all of them, or the listed ones."""
    m = np.zeros(k, dtype=bool)
    m[list(range(k)) if components is None else list(components)] = True
    return m


def evaluate(X, D, H, mask=None, log_shift=LOG_SHIFT):
    """Steps 2-4 at the given H, unscaled: dict(deviance (p,), gap (p,), r (k, p), unmodelled (p,) int, N (p,))."""
    x = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    k = D.shape[1]
    M = mask_of(k) if mask is None else np.asarray(mask, dtype=bool)
    s = D.sum(axis=0)
    N = x.sum(axis=0)
    Y = D @ H
    floored = ~(Y >= log_shift)
    Y = np.where(floored, log_shift, Y)
    w = x * (1.0 / Y)
    t = Y - x
    pos = x > 0
    t[pos] += x[pos] * np.log(w[pos])
    r = np.zeros_like(H)
    r[M] = (D[:, M].T @ w) / s[M, None]
    return dict(deviance=2.0 * t.sum(axis=0), gap=2.0 * N * (r[M].max(axis=0) - 1.0), r=r, unmodelled=(floored & pos).sum(axis=0), N=N)


def ml_unmix(X, D, H0=None, components=None, tol=1e-3, max_pass=20000, log_shift=LOG_SHIFT, history=False):
    """The rule on every pixel of X (n, p): dict(H (k, p), deviance, gap (p,), n_pass (p,) int, converged (p,) bool, unmodelled: the
    entries with counts under a floored model of the pixels that stopped).  A pixel still running at ``max_pass`` holds the h its next
    pass would start from and the deviance and gap of its last pass, as the kernel leaves it.  ``history``: also (max deviance - final
    deviance - gap) over the passes of every pixel, the certificate checked against the run's own end."""
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
    if H0 is None:   # (espm_amd.presence's default start: the counts spread evenly, N / sum_M s)
        H[M] = N[None, :] / s[M].sum()
    else:
        H[M] = np.array(H0, dtype=np.float64)[M]
    with np.errstate(divide="ignore", invalid="ignore"):
        fill = N[None, :] / (m * s[:, None]) * START
    bad = ~(H > 0) & M[:, None]
    H[bad] = fill[bad]
    dev, gap = np.zeros(p), np.zeros(p)
    n_pass, done = np.zeros(p, dtype=np.int64), N == 0
    H[:, done] = 0.0
    unmodelled = 0
    track = [] if history else None
    live = np.flatnonzero(~done)
    DM = D[:, M]
    for _ in range(max_pass):
        if live.size == 0:
            break
        h = H[:, live]
        S = s[M] @ h[M]
        h = h * (N[live] / S)
        xl = x[:, live]
        Y = D @ h
        floored = ~(Y >= log_shift)
        Y = np.where(floored, log_shift, Y)
        w = xl * (1.0 / Y)
        t = Y - xl
        pos = xl > 0
        t[pos] += xl[pos] * np.log(w[pos])
        dv = 2.0 * t.sum(axis=0)
        r = (DM.T @ w) / s[M, None]
        g = 2.0 * N[live] * (r.max(axis=0) - 1.0)
        dev[live], gap[live] = dv, g
        if history:
            track.append((live, dv, g))
        stop = g <= tol
        H[:, live[stop]] = h[:, stop]
        unmodelled += int((floored & pos)[:, stop].sum())
        go = ~stop
        h[M] = h[M] * r
        H[:, live[go]] = h[:, go]
        n_pass[live[go]] += 1
        done[live[stop]] = True
        live = live[go]
    out = dict(H=H, deviance=dev, gap=gap, n_pass=n_pass, converged=done.copy(), unmodelled=unmodelled, N=N)
    if history:
        worst = np.full(p, -np.inf)
        for idx, dv, g in track:
            worst[idx] = np.maximum(worst[idx], dv - dev[idx] - g)
        out["certificate_excess"] = worst
    return out


def flipped(X, D, H0=None, components=None, **kw):
    """``ml_unmix`` with the channels and the components in reverse order (the results in the caller's order): the same rule under
    another order of every sum."""
    k = np.asarray(D).shape[1]
    comp = None if components is None else [k - 1 - j for j in components]
    out = ml_unmix(np.asarray(X)[::-1], np.asarray(D)[::-1, ::-1], None if H0 is None else np.asarray(H0)[::-1], comp, **kw)
    out["H"] = out["H"][::-1]
    return out


def empty_model_deviance(X, log_shift=LOG_SHIFT):
    """The deviance of the model without a component: y = log_shift in every channel (the floor rule), 0 for a pixel without a count."""
    x = np.asarray(X, dtype=np.float64)
    t = log_shift - x
    pos = x > 0
    t[pos] += x[pos] * np.log(x[pos] * (1.0 / log_shift))
    return np.where(x.sum(axis=0) == 0, 0.0, 2.0 * t.sum(axis=0))


def pvalue(lr):
    """The 1/2 chi2_0 + 1/2 chi2_1 boundary mixture's tail: 1/2 erfc(sqrt(lr / 2)), and 1 where lr == 0."""
    from scipy.special import erfc
    lr = np.asarray(lr, dtype=np.float64)
    return np.where(lr > 0, 0.5 * erfc(np.sqrt(lr / 2.0)), 1.0)


def presence(X, D, H0=None, tol=1e-3, max_pass=20000, log_shift=LOG_SHIFT):
    """The nested fits: the full model, then each component left out, started at the full solution with its row zeroed.  dict(H_ml,
    deviance_ml, lr (k, p), pvalue (k, p), converged (k + 1, p), gap (k + 1, p), n_pass (k + 1, p), deviance_without (k, p))."""
    k = np.asarray(D).shape[1]
    full = ml_unmix(X, D, H0, None, tol, max_pass, log_shift)
    p = full["deviance"].size
    conv, gap, npass = [full["converged"]], [full["gap"]], [full["n_pass"]]
    without = np.empty((k, p))
    for j in range(k):
        if k == 1:
            without[j] = empty_model_deviance(X, log_shift)
            conv.append(np.ones(p, dtype=bool)), gap.append(np.zeros(p)), npass.append(np.zeros(p, dtype=np.int64))
            continue
        start = full["H"].copy()
        start[j] = 0.0
        red = ml_unmix(X, D, start, [i for i in range(k) if i != j], tol, max_pass, log_shift)
        without[j] = red["deviance"]
        conv.append(red["converged"]), gap.append(red["gap"]), npass.append(red["n_pass"])
    lr = np.maximum(without - full["deviance"][None, :], 0.0)
    return dict(H_ml=full["H"], deviance_ml=full["deviance"], lr=lr, pvalue=pvalue(lr), converged=np.stack(conv), gap=np.stack(gap),
                n_pass=np.stack(npass), deviance_without=without)


# ---- the images ---------------------------------------------------------------------------------------------------------------------------
def lines(n, k, width=None, background=0.25):
    """D (n, k): k overlapping Gaussian lines, evenly spread, on a shared flat background; every column sums to 1."""
    c = np.arange(n, dtype=np.float64)[:, None]
    centre = (np.arange(k) + 1.0) * n / (k + 1.0)
    width = n / (2.0 * (k + 1.0)) if width is None else width
    G = np.exp(-0.5 * ((c - centre[None, :]) / width) ** 2)
    G = G / G.sum(axis=0)
    D = (1.0 - background) * G + background / n
    return np.ascontiguousarray(D)


def planted(n=48, p=300, k=4, dose=30.0, absent=0.4, seed=11, empty=(5,)):
    """(X uint8 (n, p), D (n, k), H (k, p) the truth, absent (k, p) bool): a low-dose image whose abundances are planted at exactly zero
    with probability ``absent`` (never all of a pixel's), about ``dose`` counts per pixel; the pixels ``empty`` hold no count."""
    rng = np.random.default_rng(seed)
    D = lines(n, k)
    gone = rng.random((k, p)) < absent
    keep = rng.integers(0, k, p)
    gone[keep, np.arange(p)] = False
    share = rng.random((k, p)) + 0.2
    share[gone] = 0.0
    share /= share.sum(axis=0)
    H = dose * share
    X = rng.poisson(D @ H)
    for e in empty:
        X[:, e] = 0
    assert X.max() <= 255
    X = X.astype(np.uint8)
    for a in (X, D, H, gone):
        a.setflags(write=False)
    return X, D, H, gone


def start_from(X, D, seed=0):
    """A strictly positive start (k, p) of the right scale, away from the solution."""
    rng = np.random.default_rng(1000 + seed)
    k, p = np.asarray(D).shape[1], np.asarray(X).shape[1]
    N = np.asarray(X, dtype=np.float64).sum(axis=0)
    return (0.25 + rng.random((k, p))) * (np.maximum(N, 1.0) / k)[None, :]


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------------------------
MAX_PASS = 20000   # what the GPU tests pass as max_pass: the reference must converge everywhere within HALF of it (test_pixel_ml_cpu)
IMG96_K = (1, 2, 3, 5, 8)


def sharp(n, k):
    """``lines`` with half the width and a fifth of the background: spectra EM separates within hundreds of passes."""
    return lines(n, k, n / (4.0 * (k + 1.0)), 0.05)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X (n, p) read-only, D (n, k)) of a named case:
    img96_k<k>  the splitting / residuals tests' 96 x (40 x 33) 8-bit image (a ragged last wave and workgroup; 96 channels cross a
                transposing tile of 64, 32 or 16 rows) against ``sharp(96, k)``
    planted     48 channels x 300 pixels, ~30 counts per pixel, k = 4, 40 % of the abundances planted at zero
    img16       16 channels x 2118 pixels, k = 3: several workgroups
    tall        300 channels x 70 pixels, k = 3: more than one chunk of D (ESPM_DIAG_CHUNK = 256), restaged every pass"""
    if name.startswith("img96_k"):
        import marginals_reference as mr
        return mr.image(96, (40, 33), np.uint8), sharp(96, int(name[7:]))
    if name == "planted":
        return planted()[:2]
    rng = np.random.default_rng(3)
    n, p = (16, 2118) if name == "img16" else (300, 70)
    D = lines(n, 3)
    X = rng.poisson(D @ (rng.random((3, p)) * 20.0)).astype(np.uint8)
    X.setflags(write=False), D.setflags(write=False)
    return X, D


CASES = tuple(f"img96_k{k}" for k in IMG96_K) + ("planted", "img16", "tall")


@functools.lru_cache(maxsize=None)
def solved(name, tol=1e-3, max_pass=MAX_PASS):
    """``ml_unmix`` of a case from ``start_from`` over all components, computed once and shared (treat as read-only)."""
    X, D = case(name)
    return ml_unmix(X, D, start_from(X, D), None, tol, max_pass)


@functools.lru_cache(maxsize=None)
def optimum(name):
    """The long run: tol = 1e-10 from the same start (EM is monotone: its deviance is below that of every shorter run of the same
    trajectory, and within its own gap of the minimum), with the certificate's history."""
    X, D = case(name)
    return ml_unmix(X, D, start_from(X, D), None, 1e-10, MAX_PASS, history=True)
