"""What the weighted marginals must compute, in numpy fp64 straight from the definition (tests/test_marginals_cpu.py,
tests/test_gpu_marginals.py): the three sums, the rules of the weight builders restated, the sums once more in the kernel's order in
any precision, and the bounds the device has to keep.

    Y = max(D H, log_shift);  t = Y - x + x ln(x / Y), the last term 0 where x == 0
    pixel side,   weights W (g, n) over the channels:  counts = W x,  model = W Y,  deviance = 2 W t           (g, p)
    channel side, weights V (g, p) over the pixels:    counts = V x^T, model = V Y^T, deviance = 2 V t^T       (g, n)

The bounds are derived, not tuned.  u = 2^-53 is the unit roundoff and gamma(m) = m u / (1 - m u) bounds the relative error of a result
that went through m roundings (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1); gamma(a) + gamma(b) <= gamma(a + b).
The weights are SIGNED (a net line subtracts its background), so a sum can cancel to nothing and no bound can be relative to the
result: every bound is relative to the sum of the MAGNITUDES, sum |w| mag, with

    mag(x) = x,   mag(Y) = Y,   mag(t) = Y + x + x |ln(x / Y)|   - the sizes of the pieces t is put together from: t itself cancels
                                                                    (it is 0 at x == Y).

* a sum of m terms w v.  The device adds them with one fused multiply-add per walk index, the sum so far rounded each time:
  m roundings, |error| <= gamma(m) sum |w v| (Higham section 3.1, for any order).  On the pixel side m = n.  On the channel side the
  pixels of a chunk of PCHUNK are added first, min(p, PCHUNK) roundings, then the chunks in ascending order, ceil(p / PCHUNK) more.
  numpy's product here is a sum of m products in some order, with or without fused multiply-adds: gamma(m) as well, m = n or p.
* ``counts``: x and w are given, so that is all: gamma(2 n) on the pixel side, gamma(min(p, PCHUNK) + chunks + p) on the channel side,
  times sum |w| x.  For integer X under integer-valued weights with sum |w| x < 2^53 every partial sum on either side is an integer
  below 2^53: exact, the bound is 0 and the result is bit-equal to the int64 sum (``counts_exact``).
* ``model``: y = sum_i d_i h_i is k multiply-adds of non-negative numbers on the device and k products and k - 1 sums here: gamma(k)
  relative to y on either side; the floor max(y, log_shift) is exact.  gamma(2 (k + m)) sum |w| Y, the m's as above.
* ``deviance``: the term, piece by piece, on the device: Y carries k roundings; r = 1 / Y one more and x r another, so the argument of
  the logarithm carries k + 2 and the logarithm moves by (k + 2) u ABSOLUTELY (ln(a (1 + e)) = ln a + e) on top of its own error, which
  is counted as two roundings of its value (the device's fp64 log is good to one unit in the last place); Y - x is rounded once, u (Y + x),
  and inherits k u Y; the closing multiply-add is rounded once, u |t| <= u mag(t).  Collected by piece: (k + 2) u Y + (k + 4) u x +
  3 u x |ln|, at most (k + 4) u mag(t).  Here: D H carries k roundings, x / Y one, the logarithm two, its product with x one, Y - x and the
  last sum one each: (k + 2) u Y + (k + 3) u x + 4 u x |ln| <= (k + 4) u mag(t) as well.  That is to first order; one spare rounding and
  gamma's denominator cover the products of the errors: TERM_ROUNDINGS(k) = k + 5.  The doubling of the stored deviance is exact.
  2 gamma(2 (k + 5 + m)) sum |w| mag(t), the m's as above.

tests/test_marginals_cpu.py evaluates the sums in the kernel's order in extended precision (``in_kernel_order`` with np.longdouble)
against the fp64 values here: the room these bounds leave is printed there."""
import numpy as np

import splitting_reference as sr

U = 2.0 ** -53
LOG_SHIFT = 1e-14
PCHUNK = 2048   # ESPM_MARG_PCHUNK
MAX_G, MAX_K = 8, 8


def gamma(m):
    return m * U / (1.0 - m * U)


def term_roundings(k):
    return k + 5


# ---- the weight builders, restated ----------------------------------------------------------------------------------------------------
def window_weights(n, windows):
    c = np.arange(n)
    return np.stack([((c >= lo) & (c < hi)).astype(np.float64) for lo, hi in windows])


def line_weights(n, integration, background=None):
    """1 on I; with a background, minus w_I times the per-channel means of L and R interpolated between their centres at I's."""
    c = np.arange(n)

    def ind(r):
        return ((c >= r[0]) & (c < r[1])).astype(np.float64)

    def centre(r):
        return (r[0] + r[1] - 1) / 2

    u = ind(integration)
    if background is not None:
        L, R = background
        s = (centre(integration) - centre(L)) / (centre(R) - centre(L))
        u = u - (integration[1] - integration[0]) * ((1 - s) * ind(L) / (L[1] - L[0]) + s * ind(R) / (R[1] - R[0]))
    return u


def label_weights(labels, n_regions=None):
    lab = np.asarray(labels).reshape(-1)
    L = int(lab.max()) + 1 if n_regions is None else n_regions
    return np.stack([(lab == r).astype(np.float64) for r in range(L)])


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------
def pieces(X, D=None, H=None, log_shift=LOG_SHIFT):
    """(x, Y, t, mag_t) of X (n, p), each (n, p) fp64; Y, t, mag_t None without a model."""
    x = np.asarray(X).astype(np.float64)
    if D is None:
        return x, None, None, None
    Y = np.maximum(np.asarray(D, dtype=np.float64) @ np.asarray(H, dtype=np.float64), log_shift)
    lg = np.where(x > 0, np.log(np.where(x > 0, x, 1.0) / Y), 0.0)
    xl = x * lg
    return x, Y, (Y - x) + xl, Y + x + np.abs(xl)


def sums(X, W, D=None, H=None, side="pixels", log_shift=LOG_SHIFT):
    """dict(counts, model, deviance, counts_bound, model_bound, deviance_bound, counts_exact) of X (n, p) under the weights W - (g, n)
    for side "pixels", (g, p) for "channels" - every array (g, p) or (g, n): the lane index last, as the entry point stores them.
    ``counts_exact``: whether ``counts`` is promised bit for bit (then it is the int64 sum and its bound 0)."""
    X = np.asarray(X)
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    n, p = X.shape
    k = 0 if D is None else np.asarray(D).shape[1]
    x, Y, t, mag = pieces(X, D, H, log_shift)
    A = np.abs(W)
    if side == "pixels":
        def dot(M, v):
            return M @ v
        dev_m, here_m = n, n
    else:
        def dot(M, v):
            return M @ v.T
        dev_m, here_m = min(p, PCHUNK) + -(-p // PCHUNK), p
    m2 = dev_m + here_m
    out = dict(counts=dot(W, x), model=None, deviance=None, model_bound=None, deviance_bound=None)
    size = dot(A, x)
    exact = X.dtype.kind in "iub" and bool((W == np.round(W)).all()) and float(size.max()) < 2.0 ** 53
    if exact:
        out["counts"] = dot(W.astype(np.int64), X.astype(np.int64)).astype(np.float64)
    out["counts_exact"] = exact
    out["counts_bound"] = np.zeros_like(size) if exact else gamma(m2) * size
    if k:
        out["model"], out["model_bound"] = dot(W, Y), gamma(2 * k + m2) * dot(A, Y)
        out["deviance"], out["deviance_bound"] = 2.0 * dot(W, t), 2.0 * gamma(2 * term_roundings(k) + m2) * dot(A, mag)
    return out


def in_kernel_order(X, W, D=None, H=None, side="pixels", log_shift=LOG_SHIFT, ft=np.longdouble):
    """(counts, model, deviance) by the header's rule in the kernel's order - y component by component, the term through r = 1 / Y,
    one walk index after the other, on the channel side in chunks of PCHUNK pixels added afterwards - in the floating-point type ``ft``
    (without the fused multiply-adds: in extended precision that is beside the point)."""
    X = np.asarray(X)
    W = np.atleast_2d(np.asarray(W, dtype=np.float64)).astype(ft)
    n, p = X.shape
    x = X.astype(ft)
    k = 0 if D is None else np.asarray(D).shape[1]
    if k:
        Df, Hf = np.asarray(D, dtype=np.float64).astype(ft), np.asarray(H, dtype=np.float64).astype(ft)
        y = np.zeros((n, p), dtype=ft)
        for i in range(k):
            y = y + Df[:, i][:, None] * Hf[i][None, :]
        Y = np.maximum(y, ft(log_shift))
        r = ft(1) / Y
        t = Y - x
        t = t + np.where(x > 0, x * np.log(np.where(x > 0, x * r, ft(1))), ft(0))
    vals = [x] + ([Y, t] if k else [])
    if side == "pixels":
        acc = [np.zeros((W.shape[0], p), dtype=ft) for _ in vals]
        for c in range(n):
            for a, v in zip(acc, vals):
                a += W[:, c][:, None] * v[c][None, :]
    else:
        acc = [np.zeros((W.shape[0], n), dtype=ft) for _ in vals]
        for q0 in range(0, p, PCHUNK):
            part = [np.zeros((W.shape[0], n), dtype=ft) for _ in vals]
            for j in range(q0, min(p, q0 + PCHUNK)):
                for a, v in zip(part, vals):
                    a += W[:, j][:, None] * v[:, j][None, :]
            for a, b in zip(acc, part):
                a += b
    return acc[0], (acc[1] if k else None), (ft(2) * acc[2] if k else None)


# ---- the images ---------------------------------------------------------------------------------------------------------------------------
def image(n, shape, dtype):
    """``splitting_reference.image`` for any shape and dtype: its 8-bit image (whose planted entries fit every shape used here) widened, a
    16-bit, float32 or float64 one with two counts above 255 planted on top."""
    X = sr.image(n, shape, np.uint8).astype(dtype)
    if np.dtype(dtype) != np.uint8:
        p = X.shape[1]
        X[n // 2, p // 2], X[n - 1, 0] = 65535, 300
    X.setflags(write=False)
    return X


def planted_model(n, p, k, channel, pixel):
    """``attribution_reference.planted_model``: an all-zero row of D and all-zero columns of H (``pixel`` and the model's own 11), where
    Y = log_shift under whatever counts are there."""
    import attribution_reference as ar
    D, H = ar.planted_model(n, p, k, channel=channel, pixel=pixel)
    D.setflags(write=False), H.setflags(write=False)
    return D, H


LINE = ((40, 48), ((28, 36), (54, 62)))   # the planted line: integration window, two background windows
LINE_SHARE = 0.005                        # of the pixels may miss the planted counts by more than 5 net_std


def planted_line(n=96, shape=(40, 33), seed=7, background=2.0):
    """(X (n, p) uint8, planted (p,)): Poisson counts of a flat background of ``background`` counts per channel and pixel plus one line
    on the channels of LINE's integration window, with ``planted[j]`` expected counts in pixel j (10 .. 60, varying over the image)."""
    rng = np.random.default_rng(seed)
    p = shape[0] * shape[1]
    planted = 10.0 + 50.0 * (np.arange(p) % 97) / 96.0
    rate = np.full((n, p), background)
    lo, hi = LINE[0]
    rate[lo:hi] += planted[None, :] / (hi - lo)
    X = rng.poisson(rate)
    assert X.max() <= 255
    return X.astype(np.uint8), planted


def line_misses(net, net_std, planted):
    """The share of the pixels whose net counts are further than 5 net_std from the planted ones."""
    return float((np.abs(net - planted) > 5.0 * net_std).mean())
