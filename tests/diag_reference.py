"""What pixel_diagnostics must compute, in numpy fp64, and the seeded images its tests run on (tests/test_pixel_diagnostics_cpu.py,
tests/test_gpu_pixel_diagnostics.py).

    Y = max(D H, log_shift);  dev_j = 2 sum_c (x ln(x / y) - x + y);  F_j = D^T diag(1 / y_j) D;  H_std = sqrt(diag(C_j)),
    C = F^-1, or F^-1 - F^-1 1 1^T F^-1 / (1^T F^-1 1) under the simplex.

The bounds are derived, not tuned (eps = 2^-52):

* deviance: t_c = x ln(x / y) - x + y is one term of the sum and ``abs_terms`` is sum_c |t_c| (every t_c >= 0, so this is half the
  deviance itself, up to the rounding of its terms).  The recursive sum of n terms is off by at most (n - 1) eps / 2 of that.  A
  term's own rounding (the product D h, the quotient, the logarithm, the two additions) is a few eps of x, y and |x ln(x / y)|, which
  near a good fit are ~sqrt(y) times larger than t_c ~ 1 / 2: at the doses used here (y up to ~500 per entry) that is a few tens of
  eps t_c per term, against the 8 n eps >= 512 eps that every term is allowed.  tests/test_pixel_diagnostics_cpu.py holds an
  evaluation in the kernel's own order (y - x + x ln(x (1 / y)), summed channel by channel) and, where the platform has one, an
  extended-precision evaluation against this bound.
* H_std: the entries of F carry a relative error of a few eps each, (F + dF)^-1 - F^-1 is bounded by cond(F) |dF| / |F| relative to
  F^-1, the factorisation and the k solves add k-fold that; the square root halves it.  64 k eps cond(F_j), relative to the
  reference's entry.
"""
import functools

import numpy as np

EPS = 2.0 ** -52
LOG_SHIFT = 1e-14


def reference(X, D, H, log_shift=LOG_SHIFT, simplex=False):
    """dict(deviance (p,), abs_terms (p,), H_std (k, p), cond (p,), C (p, k, k)) for X (n, p), D (n, k), H (k, p), all fp64."""
    X, D, H = (np.asarray(a, dtype=np.float64) for a in (X, D, H))
    k = D.shape[1]
    Y = np.maximum(D @ H, log_shift)
    pos = X > 0
    xl = np.zeros_like(X)
    xl[pos] = X[pos] * np.log(X[pos] / Y[pos])
    dev = 2.0 * (xl - X + Y).sum(axis=0)
    abs_terms = np.abs(xl - X + Y).sum(axis=0)
    F = np.einsum("ci,cj,cp->pij", D, D, 1.0 / Y)
    with np.errstate(all="ignore"):
        cond = np.linalg.cond(F)
    try:
        Finv = np.linalg.inv(F)
    except np.linalg.LinAlgError:
        Finv = np.full_like(F, np.nan)
    C = Finv
    if simplex:
        if k == 1:
            C = np.zeros_like(Finv)   # (1 / f - (1 / f)^2 / (1 / f): exactly 0)
        else:
            u = Finv.sum(axis=2)
            C = Finv - u[:, :, None] * u[:, None, :] / u.sum(axis=1)[:, None, None]
    with np.errstate(invalid="ignore"):
        std = np.sqrt(np.maximum(np.einsum("pii->ip", C), 0.0))
    return dict(deviance=dev, abs_terms=abs_terms, H_std=std, cond=cond, C=C, F=F)


def spectra(n, k, counts):
    """(n, k): k separated Gaussian peaks on a flat background, every column summing to ``counts`` - a well-conditioned F."""
    c = np.arange(n, dtype=np.float64)[:, None]
    centres = (np.arange(k, dtype=np.float64)[None, :] + 0.5) * n / k
    D = np.exp(-0.5 * ((c - centres) / max(1.5, n / (6.0 * k))) ** 2) + 0.05
    return D * (counts / D.sum(axis=0, keepdims=True))


@functools.lru_cache(maxsize=None)
def image(n, p, k, dtype, simplex, seed=0):
    """A seeded image for the parity tests: (X (n, p) in ``dtype``, D, H, facts).  H is positive (on the simplex with ``simplex``),
    X is Poisson of D H, and
      * pixel ``empty_pixel`` has no counts at all,
      * channel ``zero_channel`` is all zero,
      * row ``floor_channel`` of D is zero, so D H = 0 < log_shift there, and one entry of X in it holds a count (with the floor
        that entry adds x ln(x / log_shift) to its pixel's deviance; without it, infinity).
    u8: counts clipped at 255; u16: a dose high enough for counts above 255; f64: a fraction added (non-integer X)."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 3 * p + k)
    dtype = np.dtype(dtype)
    counts = 40000.0 if dtype == np.uint16 else 500.0
    D = spectra(n, k, counts)
    H = rng.random((k, p)) + 0.1
    H = H / H.sum(axis=0, keepdims=True) if simplex else H * rng.uniform(0.5, 2.0, size=(1, p)) / k
    facts = dict(empty_pixel=p // 3, zero_channel=n // 2, floor_channel=n // 5, floor_pixel=(2 * p) // 3)
    D[facts["floor_channel"]] = 0.0
    X = rng.poisson(D @ H).astype(np.float64)
    if dtype == np.uint8:
        X = np.minimum(X, 255.0)
    if dtype == np.float64:
        X = X + rng.random(X.shape)
    X[:, facts["empty_pixel"]] = 0
    X[facts["zero_channel"], :] = 0
    X[facts["floor_channel"], :] = 0
    X[facts["floor_channel"], facts["floor_pixel"]] = 3
    X = X.astype(dtype)
    for a in (X, D, H):
        a.setflags(write=False)
    return X, D, H, facts


def check(out, ref, n, k, label=""):
    """The two derived bounds, per pixel and per entry; the worst ratios are printed before they are asserted."""
    dev_err = np.abs(out["deviance"] - ref["deviance"])
    dev_bound = 8 * n * EPS * ref["abs_terms"]
    std_err = np.abs(out["H_std"] - ref["H_std"])
    std_bound = 64 * k * EPS * ref["cond"][None, :] * ref["H_std"]
    with np.errstate(all="ignore"):
        r_dev = np.nanmax(dev_err / dev_bound)
        r_std = np.nanmax(np.where(std_bound > 0, std_err / std_bound, np.where(std_err > 0, np.inf, 0.0)))
    print(f"{label}: deviance error / bound {r_dev:.3g}, H_std error / bound {r_std:.3g}, max cond(F) {ref['cond'].max():.3g}")
    assert np.isfinite(out["deviance"]).all() and np.isfinite(out["H_std"]).all()
    assert (dev_err <= dev_bound).all(), f"deviance off by {r_dev:.3g} of its bound"
    assert (std_err <= std_bound).all(), f"H_std off by {r_std:.3g} of its bound"
