"""What Poisson sampling must compute, in numpy: the rule of include/espm_mu.h ("Poisson sampling") on tests/splitting_reference.py's
Philox4x32-10, and the deviance of a materialised replicate in fp64 (tests/test_sampling_cpu.py, tests/test_gpu_sampling.py).

The rule.  The image is logically (n, p_total), channel-major; element (c, j) has the index e = c p_total + j.  Its rate
y = sum_i d[c, i] h[i, j] is a plain loop over i ascending from +0 - every product and every sum rounded on its own, which numpy's
separate ``*`` and ``+`` do.  y not finite or negative: 0, counted invalid.  y > 65535: the dtype's maximum, counted saturated.
Otherwise m = floor(y), thr = floor((y - m) 2^32); block b of the element is Philox4x32-10 with the counter (e low 32, e high 32, b,
replicate + 1) and the key (seed low 32, seed high 32); N(w) = #{i : w >= UNIT_CDF[i]}; and with word_i = word (i mod 4) of block
(i div 4), N0 = N(word_0):

    x = sum_{i < m} N(word (i mod 4) of block (4 + i div 4)) + #{i in 1 .. N0 : word_i < thr},

stored as the dtype's maximum and counted saturated when it is above it.

The deviance bound is derived as in tests/splitting_reference.py (eps = 2^-52).  The kernel forms y by the rule, so its y and this
reference's are the same bits and the floor Y = max(y, log_shift) is exact: the (k + 1) eps |y - x| of the product there has no
counterpart here.  What remains per entry c of a pixel and its term t = x ln(x / Y) - x + Y:

* the term's own operations - the quotient, the logarithm (within 1 ulp, plus eps / 2 of argument error), the product with x and the
  two additions: below 2 eps (x (1 + |ln(x / Y)|) + |Y - x| + |t|) per side, 4 eps (...) for the two;
* the sum over the n channels, in order: at most (n - 1) eps / 2 of sum_c |t_c| per side.

Doubled for the factor 2 of the deviance, the two sides together:

    bound_j = 8 eps sum_c (x (1 + |ln(x / Y)|) + |Y - x| + |t|) + 2 n eps sum_c |t_c|.
"""
import numpy as np

import splitting_reference as sr

EPS = sr.EPS
LOG_SHIFT = sr.LOG_SHIFT
MAX_RATE = 65535.0
HEAVY = 256
UNIT_CDF = np.array([0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f, 0xfffffe21,
                     0xffffffd4, 0xfffffffc], dtype=np.uint64)


def rates(D, H):
    """y (n, p): sum_i D[:, i] H[i, :] for i ascending from +0, every product and sum rounded on its own."""
    D, H = np.asarray(D, dtype=np.float64), np.asarray(H, dtype=np.float64)
    y = np.zeros((D.shape[0], H.shape[1]))
    with np.errstate(all="ignore"):
        for i in range(D.shape[1]):
            t = D[:, i:i + 1] * H[i:i + 1, :]
            y = y + t
    return y


def unit(w):
    """N(w) of 32-bit words: the number of thresholds the word reaches."""
    return (np.asarray(w).astype(np.uint64)[..., None] >= UNIT_CDF).sum(axis=-1).astype(np.int64)


def draw(m, thr, e, seed, replicate):
    """x of the entries with m unit pieces, threshold thr and index e (1-D arrays), unclipped, int64."""
    m, thr, e = np.asarray(m, dtype=np.int64), np.asarray(thr, dtype=np.uint64), np.asarray(e, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    rep1 = np.uint64(replicate + 1)
    lo, hi = e & sr.MASK, e >> sr.S32
    x = np.zeros(m.shape, dtype=np.int64)
    # the fractional part: a unit draw thinned by thr
    w = sr.philox4x32((lo, hi, np.uint64(0), rep1), key)
    n0 = unit(w[0])
    for i in (1, 2, 3):
        x += ((n0 >= i) & (w[i] < thr)).astype(np.int64)
    for b in (1, 2, 3):
        live = n0 >= 4 * b
        if live.any():
            w = sr.philox4x32((lo[live], hi[live], np.uint64(b), rep1), key)
            x[live] += sum(((n0[live] >= 4 * b + t) & (w[t] < thr[live])).astype(np.int64) for t in range(4))
    # the unit pieces: below 1024 block by block over all entries, the others one by one with all their blocks at once
    small = m < 1024
    for b in range(256):
        live = small & (m > 4 * b)
        if not live.any():
            break
        w = sr.philox4x32((lo[live], hi[live], np.uint64(4 + b), rep1), key)
        left = m[live] - 4 * b
        x[live] += sum(unit(w[t]) * (left > t) for t in range(4))
    for q in np.nonzero(~small)[0]:
        b = np.arange((m[q] + 3) // 4, dtype=np.uint64)
        w = sr.philox4x32((lo[q], hi[q], np.uint64(4) + b, rep1), key)
        left = m[q] - 4 * b.astype(np.int64)
        x[q] = x[q] + sum(int((unit(w[t]) * (left > t)).sum()) for t in range(4))
    return x


def raw_rates(y, seed, replicate, p_total=None, j0=0):
    """(x (n, p) int64 unclipped, invalid, saturated): the draws of the rates y, which are the pixels j0 .. j0 + p - 1 of an image of
    p_total pixels, before they are stored in a dtype; the two masks are the entries that are not drawn."""
    y = np.asarray(y, dtype=np.float64)
    n, p = y.shape
    p_total = p if p_total is None else int(p_total)
    with np.errstate(invalid="ignore"):
        invalid = ~(np.isfinite(y) & (y >= 0))
        saturated = ~invalid & (y > MAX_RATE)
    ok = ~invalid & ~saturated
    yo = np.where(ok, y, 0.0)
    m = np.floor(yo)
    thr = np.floor((yo - m) * 2.0 ** 32).astype(np.uint64)
    e = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(p_total) + (np.uint64(j0) + np.arange(p, dtype=np.uint64))[None, :]
    x = np.zeros(y.shape, dtype=np.int64)
    x[ok] = draw(m[ok].astype(np.int64), thr[ok], e[ok], seed, replicate)
    return x, invalid, saturated


def store(raw, dtype=np.uint16):
    """(X, info): the draws of ``raw_rates`` as the sampler stores them in ``dtype``."""
    x, invalid, saturated = raw
    top = int(np.iinfo(dtype).max)
    over = saturated | (~invalid & (x > top))
    out = np.where(over, top, x)
    out[invalid] = 0
    return out.astype(dtype), dict(saturated=int(over.sum()), invalid=int(invalid.sum()))


def sample_rates(y, seed, replicate, dtype=np.uint16, p_total=None, j0=0):
    """(X, info) of the rates y (n, p)."""
    return store(raw_rates(y, seed, replicate, p_total, j0), dtype)


def sample(D, H, seed, replicate, dtype=np.uint16, p_total=None, j0=0):
    """(X (n, p) channel-major, info) of the model D (n, k), H (k, p): the slab's columns of the abundances."""
    return sample_rates(rates(D, H), seed, replicate, dtype, p_total, j0)


def deviance(X, D, H, log_shift=LOG_SHIFT):
    """dict(map (p,), bound (p,), abs_terms (p,)): 2 sum_c (x ln(x / Y) - x + Y) of the materialised replicate X against
    Y = max(rates, log_shift), and the derived bound of a kernel that has the same y."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    Y = np.maximum(rates(D, H), log_shift)
    t, scale = sr._terms(X, Y)
    return dict(map=2.0 * t.sum(axis=0), bound=8.0 * EPS * scale.sum(axis=0) + 2.0 * n * EPS * np.abs(t).sum(axis=0),
                abs_terms=np.abs(t).sum(axis=0))


# ---- the seeded model of the tests: ~0.6 counts per entry with planted rates ----------------------------------------------------------
# (channel, pixel, rate, d): the rate is the product of D[c, 0] = d and H[0, j] = rate / d, both exact in binary
PLANTED = [(2, 20, 0.0, 1.0), (4, 70, 1e-14, 1.0), (6, 130, 7.0, 1.0), (8, 200, 0.99999999, 1.0), (10, 300, 255.5, 1.0), (12, 400, 256.0, 1.0),
           (14, 500, 300.25, 1.0), (16, 640, 65535.0, 256.0), (18, 800, 65536.5, 256.0)]


def model(n=96, p=1320, k=3, seed=3):
    """(D, H) of splitting_reference.model with the rates of PLANTED at entries (c, j), set by scaling row c of D and column j of H: the
    row and the column are zero but for component 0, whose product d (rate / d) is the rate - exactly.  The rest of such a row and
    column holds rates of its own: up to 269 down the columns of the two largest (counts the wave shares among them)."""
    D, H = sr.model(n, p, k, seed=seed)
    D, H = D.copy(), H.copy()
    for c, j, rate, d in PLANTED:
        D[c, :], H[:, j] = 0.0, 0.0
    for c, j, rate, d in PLANTED:
        D[c, 0], H[0, j] = d, rate / d
    D.setflags(write=False), H.setflags(write=False)
    return D, H
