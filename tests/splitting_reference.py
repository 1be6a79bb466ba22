"""What count splitting must compute, in numpy: Philox4x32-10, the thinning rule of include/espm_mu.h ("count splitting") and both
deviances in fp64 (tests/test_splitting_cpu.py, tests/test_gpu_splitting.py).

The rule.  The image is logically (n, p_total), channel-major; element (c, j) has the index e = c p_total + j.  thr = round(q 2^32)
(ties to even, as Python's ``round`` of the exact product), held inside 1 .. 2^32 - 1.  Draw d = 0 .. x - 1 of element e is word
(d mod 4) of Philox4x32-10 with the counter (e low 32, e high 32, d div 4, 0) and the key (seed low 32, seed high 32); count d goes to
part A iff its word < thr.  x_a = the number of such d, x_b = x - x_a.

The deviance bound is derived, not tuned.  With eps = 2^-52 (a rounding is at most eps / 2 relative), per entry c of a pixel and its
term t = x ln(x / y) - x + y (x: x_a against y = Y = max(d h, log_shift), or x_b against y = r Y):

* y.  The product d h is k multiply-adds of non-negative terms: whatever their order, the computed value is within k eps / 2 of the
  exact one, relative; the factor r adds one rounding; the floor is exact.  The kernel and this reference each carry such an error, so
  their y differ by at most (k + 1) eps y.  t depends on y with the slope dt/dy = 1 - x / y: the two terms differ by
  (k + 1) eps |y - x| from this cause.  (This is what the k-term product adds to tests/diag_reference.py's derivation, and it cannot be
  folded into a multiple of t: near a good fit |y - x| ~ sqrt(2 y t) is far above t.)
* the term's own operations: the quotient x / y (eps / 2), the logarithm (its result within 1 ulp - eps |ln| - plus eps / 2 of
  argument error as an absolute error of the logarithm), the product with x and the two additions.  Together below
  eps (2 x + 2 x |ln(x / y)| + |y - x| + |t|) <= 2 eps (x (1 + |ln(x / y)|) + |y - x| + |t|) per side, 4 eps (...) for the two.
* the sum over the n channels, in order: at most (n - 1) eps / 2 of sum_c |t_c| per side.

Doubled for the factor 2 of the deviance, the two sides together:

    bound_j = 2 eps sum_c [ (k + 1) |y - x| + 4 (x (1 + |ln(x / y)|) + |y - x| + |t|) ] + 2 n eps sum_c |t_c|.

A total over p pixels, summed on the host in index order, adds (p - 1) eps / 2 of sum_j |dev_j| per side: ``total_bound``.
"""
import numpy as np

EPS = 2.0 ** -52
LOG_SHIFT = 1e-14
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11).  counter: four arrays (or scalars) of 32-bit words, key: two; returns four
    uint32 arrays.  The 32 x 32 -> 64 products are taken in uint64."""
    c = [np.asarray(v).astype(np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(q):
    """(thr, q_eff): thr = round(q 2^32) inside 1 .. 2^32 - 1, and the fraction thr / 2^32 that the split really has."""
    if not 0.0 < q < 1.0:
        raise ValueError(q)
    thr = min(max(int(round(q * 2.0 ** 32)), 1), 2 ** 32 - 1)
    return thr, thr / 2.0 ** 32


def thin(X, thr, seed, p_total=None, j0=0):
    """(X_a, X_b) of X (n, p), channel-major, by the rule; X holds the pixels j0 .. j0 + p - 1 of an image of p_total pixels."""
    X = np.asarray(X)
    n, p = X.shape
    p_total = p if p_total is None else int(p_total)
    x = X.astype(np.int64)
    e = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(p_total) + (np.uint64(j0) + np.arange(p, dtype=np.uint64))[None, :]
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    xa = np.zeros(x.shape, dtype=np.int64)
    small = x < 64
    for b in range(16):   # the elements below 64: block b of all that still have draws in it
        live = small & (x > 4 * b)
        if not live.any():
            break
        w = philox4x32((e[live] & MASK, e[live] >> S32, np.uint64(b), np.uint64(0)), key)
        left = x[live] - 4 * b
        xa[live] += sum(((w[i] < np.uint64(thr)) & (left > i)).astype(np.int64) for i in range(4))
    for c, j in zip(*np.nonzero(~small)):   # the others one by one: all blocks of an element at once
        b = np.arange((x[c, j] + 3) // 4, dtype=np.uint64)
        w = philox4x32((e[c, j] & MASK, e[c, j] >> S32, b, np.uint64(0)), key)
        left = x[c, j] - 4 * b.astype(np.int64)
        xa[c, j] = sum(int(((w[i] < np.uint64(thr)) & (left > i)).sum()) for i in range(4))
    return xa.astype(X.dtype), (x - xa).astype(X.dtype)


def _terms(x, y):
    """t = x ln(x / y) - x + y (the first term 0 where x == 0), and the per-entry scale of its rounding."""
    pos = x > 0
    ln = np.zeros_like(y)
    ln[pos] = np.log(x[pos] / y[pos])
    t = x * ln - x + y
    return t, x * (1.0 + np.abs(ln)) + np.abs(y - x) + np.abs(t)


def deviances(Xa, Xb, D, H, thr, log_shift=LOG_SHIFT):
    """dict(train_map, heldout_map (p,), heldout_counts (p,) int64, train_bound, heldout_bound (p,)) of the model D H of the training
    part: X_a against Y = max(D H, log_shift), X_b against r Y with r = (2^32 - thr) / thr."""
    Xa, Xb, D, H = (np.asarray(a, dtype=np.float64) for a in (Xa, Xb, D, H))
    n, k = D.shape
    Y = np.maximum(D @ H, log_shift)
    r = float(2 ** 32 - thr) / float(thr)
    out = {}
    for name, x, y in (("train", Xa, Y), ("heldout", Xb, r * Y)):
        t, scale = _terms(x, y)
        out[name + "_map"] = 2.0 * t.sum(axis=0)
        out[name + "_bound"] = 2.0 * EPS * ((k + 1) * np.abs(y - x) + 4.0 * scale).sum(axis=0) + 2.0 * n * EPS * np.abs(t).sum(axis=0)
    out["heldout_counts"] = np.asarray(Xb, dtype=np.int64).sum(axis=0)
    return out


def total_bound(dev_map, bound_map):
    """The bound of a total summed in index order from per-pixel values that each keep ``bound_map``."""
    return float(bound_map.sum() + len(dev_map) * EPS * np.abs(dev_map).sum())


def image(n=96, shape=(40, 33), dtype=np.uint16, seed=12345, rate=0.6):
    """The seeded test image (n, ny nx): Poisson(rate) counts with planted entries - 1, 255 and, in a 16-bit image, 256, 300 and 65535
    (the first count the wave shares, one with a ragged last block of draws, the largest)."""
    rng = np.random.default_rng(seed)
    p = shape[0] * shape[1]
    X = rng.poisson(rate, size=(n, p)).astype(np.int64)
    planted = [(0, 0, 1), (5, 7, 255), (n - 1, p - 1, 255)]
    if np.dtype(dtype) == np.uint16:
        planted += [(3, 64, 256), (17, 700, 300), (n // 2, p // 2, 65535), (n - 1, 0, 65535), (40, 1319, 257)]
    for c, j, v in planted:
        X[c, j] = v
    X = X.astype(dtype)
    X.setflags(write=False)
    return X


def model(n, p, k, seed=3, counts=0.6):
    """(D (n, k), H (k, p)): positive spectra and abundances whose product is ~``counts`` per entry; pixel 11 has h = 0: it sits at
    the ``log_shift`` floor."""
    rng = np.random.default_rng(seed + 100 * k)
    D = rng.random((n, k)) + 0.05
    H = rng.random((k, p)) + 0.05
    H *= counts / (D @ H).mean()
    H[:, 11] = 0.0
    return D, H
