"""What count attribution must compute, in numpy (tests/test_attribution_cpu.py, tests/test_gpu_attribution.py): the rule of
include/espm_mu.h ("count attribution") on top of ``splitting_reference.philox4x32``, and the expected attribution in fp64 with the
bound its device counterpart has to keep.

The rule.  The image is logically (n, p_total), channel-major; element (c, j) has the index e = c p_total + j.  Its cumulative rates
are s_0 = d[c, 0] h[0, j], s_i = s_(i-1) + d[c, i] h[i, j], every product and every sum rounded on its own (numpy's ``*`` and ``+`` on
arrays are separate operations: no fused multiply-add), a = s_(k-1).  x > 0 and a not a finite number above 0: invalid, all x counts to
component 0.  Otherwise count t = 0 .. x - 1 takes word (t mod 4) of Philox4x32-10 with the counter
(e low 32, e high 32, 0x80000000 | (t div 4), 0) and the key (seed low 32, seed high 32); with u = (w 2^-32) a it goes to the smallest i
with u < s_i, and to k - 1 if there is none.  ``assign`` applies exactly that, literally (an argmax over the comparisons, not the
running maximum the kernel uses).

The bounds of the expected attribution are derived, not tuned.  u = 2^-53 is the unit roundoff, gamma(m) = m u / (1 - m u) bounds the
relative error of a result that went through m roundings (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  D, H
and X are non-negative, so every sum below is a sum of non-negative terms and its error bound is RELATIVE TO THE RESULT, whatever the
order of the additions: a sum of m terms added in any order carries at most m - 1 roundings per term.

* the k-term product y = sum_i d_i h_i: at most k roundings (k multiply-adds, fused or not); the floor max(y, log_shift) is exact.
* the quotient w = x / Y: one more.  So w carries k + 1 roundings, on the device and here.
* ``pixel_counts`` P_jp = h_jp sum_c w_cp d_cj: the product w d (1), the sum of n terms in channel order (n - 1), the product with h
  (1): k + n + 2 roundings on each side, |P_device - P_here| <= gamma(2 (k + n + 2)) P.
* ``ratio_sums`` R_cj = sum_p w_cp h_jp: the product (1): k + 2 per side; the sum - on the device the two-level order of the
  partials, min(p, PCHUNK) - 1 roundings inside a chunk of PCHUNK pixels and ceil(p / PCHUNK) - 1 for the chunks in ascending order;
  here numpy's order, at most p - 1: |R_device - R_here| <= gamma(2 (k + 2) + min(p, PCHUNK) + ceil(p / PCHUNK) - 2 + p - 1) R.
* ``counts``: integer X is summed in int64, exactly: the bound is 0.  Floating-point X: n - 1 roundings per side, gamma(2 (n - 1)).
* the identity sum_j P_jp = counts_p where y >= log_shift: sum_j d_cj h_jp / y_c is 1 up to the k roundings of y, the rest of P's
  chain follows (the quotient, the two products, the n-term sum) and the host adds k terms: gamma(2 k + n + 2) counts_p
  (``identity_bound``).
* the identity sum_c D_cj R_cj = sum_p P_jp: both are A_j = sum_cp x d h / Y exactly.  The left side: R's chain on the device
  (k + 2 and at most p - 1), the product with d (1), the host's sum over n channels (n - 1); the right side: P's chain (k + n + 2) and
  the host's sum over p pixels (p - 1): gamma(2 k + 2 n + 2 p + 2) A_j (``totals_bound``).
"""
import numpy as np

import splitting_reference as sr

U = 2.0 ** -53
LOG_SHIFT = 1e-14
PCHUNK = 1024   # ESPM_ATTRIB_PCHUNK
MARK = 0x80000000


def gamma(m):
    return m * U / (1.0 - m * U)


def rates(D, H):
    """S (k, n, p): the cumulative rates of every entry, each product and each sum rounded on its own."""
    D, H = np.asarray(D, dtype=np.float64), np.asarray(H, dtype=np.float64)
    k = D.shape[1]
    S = np.empty((k, D.shape[0], H.shape[1]))
    S[0] = D[:, 0][:, None] * H[0][None, :]
    for i in range(1, k):
        S[i] = S[i - 1] + D[:, i][:, None] * H[i][None, :]
    return S


def _place(w, live_left, S, a):
    """Which component every draw of one block goes to: w four arrays of words (m,), live_left (m,) the draws left from this block
    on, S (k, m), a (m,).  Returns (k, m) counts."""
    k = S.shape[0]
    out = np.zeros((k, len(a)), dtype=np.int64)
    for t in range(4):
        u = (w[t].astype(np.float64) * 2.0 ** -32) * a
        below = u[None, :] < S
        idx = np.where(below.any(axis=0), below.argmax(axis=0), k - 1)
        use = live_left > t
        np.add.at(out, (idx[use], np.nonzero(use)[0]), 1)
    return out


def assign(X, D, H, seed, p_total=None, j0=0):
    """(parts (k, n, p) in X's dtype, invalid): X (n, p), channel-major, holding the pixels j0 .. j0 + p - 1 of an image of p_total
    pixels, split by the rule; H holds those p pixels."""
    X = np.asarray(X)
    n, p = X.shape
    p_total = p if p_total is None else int(p_total)
    x = X.astype(np.int64)
    S = rates(D, H)
    k = S.shape[0]
    a = S[-1]
    e = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(p_total) + (np.uint64(j0) + np.arange(p, dtype=np.uint64))[None, :]
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(a) & (a > 0)
    bad = (x > 0) & ~ok
    parts = np.zeros((k, n, p), dtype=np.int64)
    parts[0][bad] = x[bad]
    small = ok & (x < 64)
    for b in range(16):   # the elements below 64: block b of all that still have draws in it
        live = small & (x > 4 * b)
        if not live.any():
            break
        w = sr.philox4x32((e[live] & sr.MASK, e[live] >> sr.S32, np.uint64(MARK | b), np.uint64(0)), key)
        parts[:, live] += _place(w, x[live] - 4 * b, S[:, live], a[live])
    for c, j in zip(*np.nonzero(ok & (x >= 64))):   # the others one by one: all blocks of an element at once
        b = np.arange((x[c, j] + 3) // 4, dtype=np.uint64)
        w = sr.philox4x32((e[c, j] & sr.MASK, e[c, j] >> sr.S32, b | np.uint64(MARK), np.uint64(0)), key)
        got = _place(w, x[c, j] - 4 * b.astype(np.int64), np.repeat(S[:, c, j][:, None], len(b), axis=1), np.full(len(b), a[c, j]))
        parts[:, c, j] = got.sum(axis=1)
    return parts.astype(X.dtype), int(bad.sum())


def words(e, x, seed):
    """The (counter, key) tuples the rule uses for an element of index e with x counts: one per block of four draws."""
    return {((e & 0xFFFFFFFF, e >> 32, MARK | b, 0), (seed & 0xFFFFFFFF, seed >> 32)) for b in range((x + 3) // 4)}


def multinomial_z(X, D, H, parts):
    """z (k,) of the per-component totals of ``parts`` against their multinomial expectation over the valid entries."""
    S = rates(D, H)
    a = S[-1]
    ok = np.isfinite(a) & (a > 0)
    x = np.where(ok, np.asarray(X, dtype=np.float64), 0.0)
    z = np.empty(S.shape[0])
    for i in range(S.shape[0]):
        pr = np.where(ok, (S[i] - (S[i - 1] if i else 0.0)) / np.where(ok, a, 1.0), 0.0)
        mean, var = (x * pr).sum(), (x * pr * (1.0 - pr)).sum()
        z[i] = (np.asarray(parts[i], dtype=np.float64)[ok].sum() - mean) / np.sqrt(var) if var > 0 else 0.0
    return z


def expected(X, D, H, log_shift=LOG_SHIFT):
    """dict(pixel_counts (k, p), ratio_sums (n, k), channel_counts (n, k), counts (p,), unattributed (p,)) of X (n, p) and the model
    D (n, k), H (k, p), and the bounds of the module's docstring: pixel_bound, ratio_bound, counts_bound, identity_bound (p,),
    totals_bound (k,)."""
    X = np.asarray(X)
    D, H = np.asarray(D, dtype=np.float64), np.asarray(H, dtype=np.float64)
    n, k = D.shape
    p = H.shape[1]
    x = X.astype(np.float64)
    Y = np.maximum(D @ H, log_shift)
    w = np.where(x != 0, x / Y, 0.0)
    P = H * (D.T @ w)
    R = w @ H.T
    integer = X.dtype.kind in "iub"
    counts = X.astype(np.int64).sum(axis=0) if integer else x.sum(axis=0)
    chunks = -(-p // PCHUNK)
    out = dict(pixel_counts=P, ratio_sums=R, channel_counts=D * R, counts=counts, unattributed=counts - P.sum(axis=0))
    out["pixel_bound"] = gamma(2 * (k + n + 2)) * P
    out["ratio_bound"] = gamma(2 * (k + 2) + min(p, PCHUNK) + chunks - 2 + p - 1) * R
    out["counts_bound"] = np.zeros(p) if integer else gamma(2 * (n - 1)) * counts
    out["identity_bound"] = gamma(2 * k + n + 2) * np.asarray(counts, dtype=np.float64)
    out["totals_bound"] = gamma(2 * k + 2 * n + 2 * p + 2) * P.sum(axis=1)
    return out


def planted_model(n, p, k, channel=20, pixel=500, seed=3):
    """``splitting_reference.model`` with one all-zero row of D (``channel``) and one all-zero column of H (``pixel``) on top of its
    own zero column 11: the entries of that channel and of those pixels have y = 0."""
    D, H = sr.model(n, p, k, seed=seed)
    D, H = D.copy(), H.copy()
    D[channel, :] = 0.0
    H[:, pixel] = 0.0
    return D, H
