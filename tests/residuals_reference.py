"""What the residual products must compute, in numpy fp64 straight from the definition (tests/test_residuals_cpu.py,
tests/test_gpu_residuals.py): the Pearson residual matrix with its floor rule, its products with a block of vectors from either side,
the products once more in the kernel's order in any precision, the bounds the device has to keep, and the three-phase image the
missing-phase conditions are stated on.

    y = D H;  floored = not (y >= log_shift);  e = 0 where floored, else (x - y) / sqrt(y)
    pixel side,   vectors U (g, n) over the channels:  out = U E   (g, p),  chi2 = sum_c e^2  (p,)
    channel side, vectors V (g, p) over the pixels:    out = V E^T (g, n),  chi2 = sum_j e^2  (n,)
    unmodelled = #{floored and x > 0}

The bounds are derived, not tuned.  u = 2^-53 is the unit roundoff and gamma(m) = m u / (1 - m u) bounds the relative error of a result
that went through m roundings (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1); gamma(a) + gamma(b) <= gamma(a + b).
The vectors are SIGNED and e is signed, so a sum can cancel to nothing and no bound can be relative to the result: every bound is
relative to a sum of MAGNITUDES, with

    mag(e) = (x + y) / sqrt(y)   - the sizes of the pieces e is put together from: e itself cancels (it is 0 at x == y).

* one entry.  D and H are not negative, so y = sum_i d_i h_i, k multiply-adds on the device and k products and k - 1 sums here, carries
  k roundings: y^ = y (1 + t), |t| <= gamma(k).  That error enters e twice.  The numerator x - y^ is rounded once and inherits t y:
  its error is at most (k + 1) u (x + y) to first order.  The square root is rounded once and inherits t / 2: sqrt(y^)^ = sqrt(y)
  (1 + s), |s| <= (k / 2 + 1) u; the quotient is rounded once.  Together |e^ - e| <= ((k + 1) + (k / 2 + 1) + 1) u mag(e), since
  |x - y| <= x + y.  That is to first order; rounded up to whole roundings, with one spare that together with gamma's denominator covers
  the products of the errors: ENTRY_ROUNDINGS(k) = 2 k + 4.  An entry that is floored is exactly 0 on both sides (the planted zeros
  of the tests' models are exact zeros in any order of summation).
* a sum of m terms v e.  The device adds them with one fused multiply-add per walk index, the sum so far rounded each time:
  m roundings, |error| <= gamma(m) sum |v| |e| <= gamma(m) sum |v| mag(e) (Higham section 3.1, for any order).  On the pixel side
  m = n.  On the channel side the pixels of a chunk of PCHUNK are added first, min(p, PCHUNK) roundings, then the chunks in ascending
  order, ceil(p / PCHUNK) more.  numpy's product here is a sum of m products in some order, with or without fused multiply-adds:
  gamma(m) as well, m = n or p.
* ``out``: both sides form every entry (ENTRY_ROUNDINGS each) and sum: gamma(2 ENTRY_ROUNDINGS(k) + m_device + m_here) sum |v| mag(e).
* ``chi2``: the analogous bound.  The term e^2 moves by 2 |e| |e^ - e| (and the square of that error, which the spare covers) and is
  rounded with the sum; e^2 cancels as e does, so the bound cannot be relative to sum e^2 where x is close to y - it is relative to
  sum |e| mag(e) >= sum e^2:  gamma(2 (2 ENTRY_ROUNDINGS(k) + 1) + m_device + m_here) sum |e| mag(e).

tests/test_residuals_cpu.py evaluates the products in the kernel's order in extended precision (``in_kernel_order`` with
np.longdouble) against the fp64 values here: the room these bounds leave is printed there (worst error / bound: 0.0005 .. 0.06).

THE NUMBERS the conditions of the tests rest on, measured with numpy on ``three_phase()`` (96 channels x 40 x 33 pixels, 198237
counts, maximum count 27; the analytic edge sqrt(96) + sqrt(1320) is 46.13):

* against the TRUE two-phase model (the third phase left out, ``two_phase_H``) numpy.linalg.svd of E gives 433.7, 101.2, 93.2, 85.9,
  78.4, ... with s_9 = 63.0: four values are separated by the tests' own criterion (s_i >= 1.25 s_9).  The third peak's channels hold
  counts over a model of 0.08 per channel there, so e is heavy-tailed and the disc is not one triplet.  The subspace iteration of
  espm_amd.residuals on ``make_products`` here stops by tol = 1e-10 after 19 iterations with relative errors 3e-16, 0, 3e-14, 2e-11
  and Ritz residuals 3e-13, 1e-6, 2e-5, 4e-4 (the rate of a value is (s_9 / s_i)^4 per iteration: the block holds 8); the leading map
  correlates with the disc at 0.98 and the leading spectrum with the third one at 0.997.  Against the true three-phase model: 45.6.
* against the independence model: 188.6, 155.7, 46.1, 45.5, ... - two values above the bulk for three phases, as correspondence
  analysis predicts; over sqrt(T) they are 0.42362, 0.34978, the values after the trivial 1 of svd(X / sqrt(r c^T)).
* FITTED by plain KL multiplicative updates (800 iterations from a random start) with k = 2: s_1 = 144.1 against 45.6 .. 46.6 for
  the top value of 10 replicates of the fitted model (3.1 times the largest), |corr| of the leading map with the disc 0.94 and of
  the leading spectrum with the third one 0.94.  With k = 3: s_1 = 45.30 against 45.2 .. 46.3 - nothing above the null."""
import numpy as np

U = 2.0 ** -53
LOG_SHIFT = 1e-14
PCHUNK = 2048   # ESPM_RESID_PCHUNK
MAX_G, MAX_K = 8, 8


def gamma(m):
    return m * U / (1.0 - m * U)


def entry_roundings(k):
    return 2 * k + 4


# ---- the matrix and its products --------------------------------------------------------------------------------------------------------
def pearson(X, D, H, log_shift=LOG_SHIFT):
    """(e, mag, floored, unmodelled) of X (n, p): e and mag fp64 (n, p), both 0 where the model is below log_shift."""
    x = np.asarray(X).astype(np.float64)
    y = np.asarray(D, dtype=np.float64) @ np.asarray(H, dtype=np.float64)
    floored = ~(y >= log_shift)
    ys = np.where(floored, 1.0, y)
    root = np.sqrt(ys)
    e = np.where(floored, 0.0, (x - ys) / root)
    mag = np.where(floored, 0.0, (x + ys) / root)
    return e, mag, floored, int((floored & (x > 0)).sum())


def _roundings(n, p, side):
    """(on the device, here): the roundings of a sum along the side's summed axis."""
    if side == "pixels":
        return n, n
    return min(p, PCHUNK) + -(-p // PCHUNK), p


def products(X, V, D, H, side="pixels", log_shift=LOG_SHIFT):
    """dict(out, chi2, out_bound, chi2_bound, unmodelled) of X (n, p) under the vectors V - (g, n) for side "pixels", (g, p) for
    "channels": out (g, p) or (g, n), chi2 (p,) or (n,) - the lane index last, as the entry point stores them."""
    X = np.asarray(X)
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    n, p = X.shape
    k = np.asarray(D).shape[1]
    e, mag, _, unmodelled = pearson(X, D, H, log_shift)
    axis = 0 if side == "pixels" else 1
    dot = (lambda M, v: M @ v) if side == "pixels" else (lambda M, v: M @ v.T)
    m_dev, m_here = _roundings(n, p, side)
    r = entry_roundings(k)
    return dict(out=dot(V, e), chi2=(e * e).sum(axis=axis), unmodelled=unmodelled,
                out_bound=gamma(2 * r + m_dev + m_here) * dot(np.abs(V), mag),
                chi2_bound=gamma(2 * (2 * r + 1) + m_dev + m_here) * (np.abs(e) * mag).sum(axis=axis))


def in_kernel_order(X, V, D, H, side="pixels", log_shift=LOG_SHIFT, ft=np.longdouble):
    """(out, chi2) by the header's rule in the kernel's order - y component by component, the entry through its subtraction, square
    root and quotient, one walk index after the other, on the channel side in chunks of PCHUNK pixels added afterwards - in the
    floating-point type ``ft`` (without the fused multiply-adds: in extended precision that is beside the point)."""
    X = np.asarray(X)
    V = np.atleast_2d(np.asarray(V, dtype=np.float64)).astype(ft)
    n, p = X.shape
    x = X.astype(ft)
    Df, Hf = np.asarray(D, dtype=np.float64).astype(ft), np.asarray(H, dtype=np.float64).astype(ft)
    y = np.zeros((n, p), dtype=ft)
    for i in range(Df.shape[1]):
        y = y + Df[:, i][:, None] * Hf[i][None, :]
    floored = ~(y >= ft(log_shift))
    ys = np.where(floored, ft(1), y)
    e = np.where(floored, ft(0), (x - ys) / np.sqrt(ys))
    g = V.shape[0]
    if side == "pixels":
        out, chi2 = np.zeros((g, p), dtype=ft), np.zeros(p, dtype=ft)
        for c in range(n):
            out += V[:, c][:, None] * e[c][None, :]
            chi2 += e[c] * e[c]
        return out, chi2
    out, chi2 = np.zeros((g, n), dtype=ft), np.zeros(n, dtype=ft)
    for q0 in range(0, p, PCHUNK):
        po, pc = np.zeros((g, n), dtype=ft), np.zeros(n, dtype=ft)
        for j in range(q0, min(p, q0 + PCHUNK)):
            po += V[:, j][:, None] * e[:, j][None, :]
            pc += e[:, j] * e[:, j]
        out += po
        chi2 += pc
    return out, chi2


def make_products(X, D, H, log_shift=LOG_SHIFT):
    """The callable ``espm_amd.residuals._subspace_iteration`` takes, on numpy: E formed once."""
    e, _, _, unmodelled = pearson(X, D, H, log_shift)

    def run(side, vectors, chi2=False):
        V = np.atleast_2d(np.asarray(vectors, dtype=np.float64))
        axis = 0 if side == "pixels" else 1
        return dict(out=V @ e if side == "pixels" else V @ e.T, chi2=(e * e).sum(axis=axis) if chi2 else None, unmodelled=unmodelled)

    return run


# ---- the image ----------------------------------------------------------------------------------------------------------------------------
PEAKS = (20, 50, 75)
DISC = ((12, 20), 6.0, 0.25)   # centre (row, column), radius, the third phase's abundance inside


def three_phase(n=96, shape=(40, 33), seed=7, dose=150.0):
    """dict(X (n, p) uint8, D (n, 3), H (3, p), disc (p,) bool, shape): Poisson counts of three phases.  The spectra are a flat
    background (5 % of the counts) under a Gaussian peak (sigma 3 channels) at the channels PEAKS, each summing to ``dose`` counts per pixel; the first
    phase's abundance ramps from 0.2 to 0.8 along x, the second is the rest; the third holds DISC[2] on a disc of radius DISC[1] at
    DISC[0], where it takes its share from the other two in proportion.  D[:, :2] with ``two_phase_H`` is the true two-phase model:
    what a fit that knows nothing of the third phase should find."""
    ny, nx = shape
    p = ny * nx
    c = np.arange(n, dtype=np.float64)
    peaks = np.stack([np.exp(-0.5 * ((c - pk) / 3.0) ** 2) for pk in PEAKS], axis=1)
    S = 0.05 / n + 0.95 * peaks / peaks.sum(axis=0, keepdims=True)
    yy, xx = np.mgrid[0:ny, 0:nx]
    a1 = (0.2 + 0.6 * xx / (nx - 1.0)).reshape(p)
    (cy, cx), radius, a3 = DISC
    disc = (((yy - cy) ** 2 + (xx - cx) ** 2) <= radius ** 2).reshape(p)
    third = np.where(disc, a3, 0.0)
    H = np.stack([a1 * (1.0 - third), (1.0 - a1) * (1.0 - third), third])
    D = dose * S
    X = np.random.default_rng(seed).poisson(D @ H)
    assert X.max() <= 255
    X = X.astype(np.uint8)
    for A in (X, D, H, disc):
        A.setflags(write=False)
    return dict(X=X, D=D, H=H, disc=disc, shape=shape)


def two_phase_H(H):
    """The abundances of the first two phases as if the third were not there: they sum to 1 in every pixel."""
    return np.ascontiguousarray(H[:2] / H[:2].sum(axis=0, keepdims=True))


def independence(X):
    """(D (n, 1), H (1, p), T): r / T, c and the total of integer X, exact."""
    Xi = np.asarray(X).astype(np.int64)
    r, c = Xi.sum(axis=1).astype(np.float64), Xi.sum(axis=0).astype(np.float64)
    T = float(Xi.sum())
    return (r / T)[:, None], c[None, :], T


def planted_model(n, p, k, channel, pixel):
    """``attribution_reference.planted_model``: an all-zero row of D and all-zero columns of H (``pixel`` and the model's own 11), where
    the model is 0 under whatever counts are there."""
    import attribution_reference as ar
    D, H = ar.planted_model(n, p, k, channel=channel, pixel=pixel)
    D.setflags(write=False), H.setflags(write=False)
    return D, H


def corr(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.corrcoef(a, b)[0, 1])
