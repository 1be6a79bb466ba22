"""What spectral_diagnostics must compute, in numpy fp64 straight from the definitions, and the seeded images its tests run on
(tests/test_spectral_diagnostics_cpu.py, tests/test_gpu_spectral_diagnostics.py).

    Y = max(D H, log_shift), D = W or G W;  per channel c:  dev_c = 2 sum_p (x ln(x / y) - x + y),  sum_p x,  sum_p y,
    M_c = sum_p h_p h_p^T / y_cp  (an einsum over the pixels).
    G = None:  S_c = M_c^-1 (np.linalg.inv),  W_std = D_std = sqrt(diag S_c); under the simplex over the rows R,
               T = sum_{c in R} S_c and the rows of R get diag(S_c - S_c T^-1 S_c).
    G (n, m):  F[(i,a),(j,b)] = sum_c G[c,i] G[c,j] M_c[a,b] (one einsum over (c, i, j, a, b)),  C = F^-1, under the simplex
               C - C A (A^T C A)^-1 A^T C;  W_std[i,a] = sqrt(C[(i,a),(i,a)]),  D_std[c,a] = sqrt(g_c^T C_aa g_c).

The bounds are derived, not tuned (eps = 2^-52; every image here has H > 0, G >= 0, D >= 0):

* deviance, C1 = 8:  |dev - ref| <= C1 p eps sum_p |t|, t = x ln(x / y) - x + y >= 0.  Any order of adding p non-negative terms
  is within (p - 1) eps of their sum; a term's own rounding is a few tens of eps t at these doses (tests/diag_reference.py has the
  argument, with the channels in place of the pixels), against the 8 p eps >= 512 eps every term is allowed.
* sum_spectrum: for integer dtypes every partial sum is an integer below 2^53, exact in any order: bit-equal.
* model_spectrum and every entry of M, C2 = 4:  relative error <= C2 (p + k) eps.  y = d . h is a sum of k non-negative
  products: k eps relative, the floor keeps it; 1 / y, h_i / y and its product with h_j are three more roundings; the sum over
  p non-negative terms adds (p - 1) eps in any order.  (p + k + 3) eps for either side, twice that between two evaluations,
  and 2 (p + k + 3) <= 4 (p + k).  Nothing cancels, so the bound is relative to the entry itself.
* W_std, D_std, C3 = 8:  relative to the reference's entry, <= C3 k (p + k) eps cond, cond = cond(M_c), or cond(F) with a
  dictionary.  With S = M^-1 and a perturbation dM of relative size delta entry-wise (M >= 0 entry-wise, so |dM|_2 <= delta |M|_2),
  d(v^T S v) = -(S v)^T dM (S v) to first order, |S v|^2 = v^T S^2 v <= |S|_2 v^T S v, hence |d(v^T S v)| <= delta cond(M) v^T S v:
  relative to the entry, for a diagonal entry (v = e_i) and for g_c^T C_aa g_c alike; the square root halves it.  delta is the
  C2 (p + k) eps above (for F, the n non-negative terms of its assembly on top: (n + 2) eps, inside the factor k and C3 at the
  shapes used), the factorisations and solves on either side add a few k eps cond.
  Under the simplex the variance is a difference, S_ii - (S T^-1 S)_ii, and the derivation above covers only its first term: were
  the constrained variance a small fraction of the free one, the error relative to it would grow by that fraction.  The bound is
  asserted in the same shape all the same, with the channel's own cond(M_c) (cond(F) with a dictionary) and no further factor: on
  these images the constrained variances are of the size of the free ones; the worst ratio to the bound is 3e-3 (k = 1, where
  cond = 1 leaves the bound at its smallest) and below 1e-4 for k >= 3.
  tests/test_spectral_diagnostics_cpu.py evaluates everything in the kernel's order (pixel chunks of ESPM_CDIAG_PCHUNK, added
  afterwards) and in extended precision against these bounds and prints the room.
"""
import functools

import numpy as np

import diag_reference as dr

EPS = dr.EPS
LOG_SHIFT = dr.LOG_SHIFT
C1, C2, C3 = 8, 4, 8
M_DICT = 6


def _rows(simplex_rows, rows):
    if simplex_rows is None:
        return None
    return np.arange(rows) if simplex_rows is True else np.asarray(simplex_rows, dtype=np.int64)


def _inv(A):
    try:
        with np.errstate(all="ignore"):
            return np.linalg.inv(A)
    except np.linalg.LinAlgError:
        return np.full_like(A, np.nan)


def bounds_from_M(M, G=None, simplex_rows=None):
    """dict(W_std, D_std, cond, cond_D, C, cond_max) from M (n, k, k) by np.linalg.inv: cond(M_c) of the entry's channel, or cond(F)
    with a dictionary, shaped like W_std (cond) and like D_std (cond_D)."""
    M = np.asarray(M, dtype=np.float64)
    n, k = M.shape[:2]
    with np.errstate(all="ignore"):
        if G is None:
            rows = _rows(simplex_rows, n)
            cond = np.linalg.cond(M)
            S = _inv(M)
            free = np.einsum("cii->ci", S).copy()
            var, cond_k = free.copy(), np.repeat(cond[:, None], k, axis=1)
            C = S
            if rows is not None:
                Tinv = _inv(S[rows].sum(axis=0))
                var[rows] = free[rows] - np.einsum("cij,jl,cli->ci", S[rows], Tinv, S[rows])
            std = np.sqrt(np.maximum(var, 0.0))
            return dict(W_std=std, D_std=std.copy(), cond=cond_k, cond_D=cond_k, C=C, cond_max=cond.max())
        G = np.asarray(G, dtype=np.float64)
        m = G.shape[1]
        rows = _rows(simplex_rows, m)
        F = np.einsum("ci,cj,cab->iajb", G, G, M).reshape(m * k, m * k)
        cond = np.linalg.cond(F)
        Cf = _inv(F)
        C = Cf
        if rows is not None:
            A = np.zeros((m, k, k))
            A[rows] = np.eye(k)
            A = A.reshape(m * k, k)
            C = Cf - Cf @ A @ _inv(A.T @ Cf @ A) @ A.T @ Cf
        C4 = C.reshape(m, k, m, k)
        var_W, var_D = np.einsum("iaia->ia", C4), np.einsum("ci,iaja,cj->ca", G, C4, G)
        return dict(W_std=np.sqrt(np.maximum(var_W, 0.0)), D_std=np.sqrt(np.maximum(var_D, 0.0)), cond=np.full((m, k), cond),
                    cond_D=np.full((G.shape[0], k), cond), C=C, F=F, cond_max=float(cond))


def reference(X, D_or_W, H, G=None, simplex_rows=None, log_shift=LOG_SHIFT):
    """Everything spectral_diagnostics returns, plus abs_terms (n,) and the cond arrays of ``bounds_from_M``; X is (n, p)."""
    X, W, H = (np.asarray(a, dtype=np.float64) for a in (X, D_or_W, H))
    D = W if G is None else np.asarray(G, dtype=np.float64) @ W
    Y = np.maximum(D @ H, log_shift)
    pos = X > 0
    xl = np.zeros_like(X)
    xl[pos] = X[pos] * np.log(X[pos] / Y[pos])
    t = xl - X + Y
    M = np.einsum("ip,jp,cp->cij", H, H, 1.0 / Y, optimize=True)
    out = dict(channel_deviance=2.0 * t.sum(axis=1), abs_terms=np.abs(t).sum(axis=1), sum_spectrum=X.sum(axis=1),
               model_spectrum=Y.sum(axis=1), M=M)
    out.update(bounds_from_M(M, G=G, simplex_rows=simplex_rows))
    return out


@functools.lru_cache(maxsize=None)
def dict_image(n, p, k, dtype, m=M_DICT, seed=0):
    """A seeded dictionary image: (X (n, p) in ``dtype``, G (n, m), W (m, k), H, facts) with the facts of ``diag_reference.image`` - a
    pixel without counts, an all-zero channel, and a row of G (so of D = G W) that is 0 with one counted entry of X in it."""
    rng = np.random.default_rng(2000 * seed + 7 * n + 3 * p + k)
    c = np.arange(n, dtype=np.float64)[:, None]
    G = np.exp(-0.5 * ((c - (np.arange(m)[None, :] + 0.5) * n / m) / max(2.5, n / (4.0 * m))) ** 2) + 0.05
    W = rng.random((m, k)) ** 2 + 0.05
    W *= 500.0 / (G @ W).sum(axis=0, keepdims=True)
    H = (rng.random((k, p)) + 0.1) * rng.uniform(0.5, 2.0, size=(1, p)) / k
    facts = dict(empty_pixel=p // 3, zero_channel=n // 2, floor_channel=n // 5, floor_pixel=(2 * p) // 3)
    G[facts["floor_channel"]] = 0.0
    X = rng.poisson(G @ W @ H).astype(np.float64)
    if np.dtype(dtype) == np.uint8:
        X = np.minimum(X, 255.0)
    X[:, facts["empty_pixel"]] = 0
    X[facts["zero_channel"], :] = 0
    X[facts["floor_channel"], :] = 0
    X[facts["floor_channel"], facts["floor_pixel"]] = 3
    X = X.astype(dtype)
    for a in (X, G, W, H):
        a.setflags(write=False)
    return X, G, W, H, facts


def _ratio(err, bound):
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))


def check(out, ref, p, k, label="", integer=True, stds=True):
    """The derived bounds, per channel and per entry; the worst ratios are printed before they are asserted.  ``stds=False``: the
    sums only (singular images, whose reference inverse means nothing)."""
    lim = C2 * (p + k) * EPS
    r_dev = _ratio(np.abs(out["channel_deviance"] - ref["channel_deviance"]), C1 * p * EPS * ref["abs_terms"])
    r_y = _ratio(np.abs(out["model_spectrum"] - ref["model_spectrum"]), lim * ref["model_spectrum"])
    r_m = _ratio(np.abs(out["M"] - ref["M"]), lim * np.abs(ref["M"]))
    msg = f"{label}: deviance {r_dev:.3g}, model_spectrum {r_y:.3g}, M {r_m:.3g}"
    r_w = r_d = 0.0
    if stds:
        fac = C3 * k * (p + k) * EPS
        r_w = _ratio(np.abs(out["W_std"] - ref["W_std"]), fac * ref["cond"] * ref["W_std"])
        r_d = _ratio(np.abs(out["D_std"] - ref["D_std"]), fac * ref["cond_D"] * ref["D_std"])
        msg += f", W_std {r_w:.3g}, D_std {r_d:.3g} of their bounds; max cond {ref['cond_max']:.3g}"
    print(msg)
    assert all(np.isfinite(out[a]).all() for a in ("channel_deviance", "sum_spectrum", "model_spectrum", "M"))
    assert r_dev <= 1, f"deviance off by {r_dev:.3g} of its bound"
    if integer:
        assert np.array_equal(out["sum_spectrum"], ref["sum_spectrum"]), "sums of counts are exact"
    else:
        assert _ratio(np.abs(out["sum_spectrum"] - ref["sum_spectrum"]), lim * ref["sum_spectrum"]) <= 1
    assert r_y <= 1, f"model_spectrum off by {r_y:.3g} of its bound"
    assert r_m <= 1, f"M off by {r_m:.3g} of its bound"
    if stds:
        assert np.isfinite(out["W_std"]).all() and np.isfinite(out["D_std"]).all()
        assert r_w <= 1, f"W_std off by {r_w:.3g} of its bound"
        assert r_d <= 1, f"D_std off by {r_d:.3g} of its bound"
