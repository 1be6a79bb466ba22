"""Objective pieces of the path (espm/measures.py:456-504, :524-548, :560-577; KLdiv :387-425) on the GPU, the majorisers the path's
tests check the updates against (KL_loss_surrogate, log_surrogate: host numpy) and the ground-truth comparison of a fit
(espm/measures.py:13-47, :99-119, :125-339, :579-626; k x k problems, host numpy)."""
import ctypes as C

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_image, check_log_shift, check_model
from espm_amd.conf import log_shift


def KLdiv_loss(X, W, H, log_shift=log_shift, average=False):
    """sum(WH) - sum(max(X, eps) log(WH)) with W, H clamped at eps (espm/measures.py:456-504).

    Evaluated by the H-step kernel in loss-only mode: it forms sum X log(X / Y) per pixel tile;
    sum X log X is added back here."""
    import torch

    from espm_amd.engine import MUEngine

    X = np.asarray(X)
    W = np.maximum(np.asarray(W), log_shift)
    H = np.maximum(np.asarray(H), log_shift)
    eng = MUEngine(X, H.shape[0], fix_zero_lines=False, max_iter=1, log_shift=log_shift, simplex_W=False)
    eng.load_state(W, H)
    eng.eval_current(advance_h=False)
    h = eng.history(average=False)
    kl_div = float(h["kl"][0])                      # sum X ln(X/Y) + sum Y - sum X
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64))
    xlogx = float(torch.xlogy(Xd, Xd.clamp_min(log_shift)).sum())
    val = kl_div + eng.sum_x - xlogx                # (eps * log Y on empty bins is below the sum's resolution)
    return val / X.size if average else val


def KLdiv(X, D, H, log_shift=log_shift, average=False):
    """Generalised KL divergence D_KL(X || D H) = sum X log(X / DH) + sum(DH - X), all three clamped at log_shift (espm/measures.py:387-425).

    The factorised form of the path's data term: the H-step kernel in loss-only mode forms exactly this sum per pixel tile (the state's
    record: KL part + sum of D H - sum of X), in fp32 element-wise with fp64 sums."""
    from espm_amd.engine import MUEngine

    X = np.asarray(X)
    D = np.maximum(np.asarray(D), log_shift)
    H = np.maximum(np.asarray(H), log_shift)
    eng = MUEngine(X, H.shape[0], fix_zero_lines=False, max_iter=1, log_shift=log_shift, simplex_W=False)
    eng.load_state(D, H)
    eng.eval_current(advance_h=False)
    val = float(eng.history(average=False)["kl"][0])   # (X = 0 contributes log_shift * log(log_shift / Y) in the reference: below the sum's resolution)
    return val / X.size if average else val


def KL(X, Y, log_shift=log_shift, average=False):
    """Generalised KL divergence of two matrices, sum X log(X / Y) + sum(Y - X) with both clamped at log_shift (espm/measures.py:427-454):
    a reporting measure of arbitrary arrays - element-wise in fp64 with torch where the arrays are, the host for numpy input."""
    import torch

    Xt = torch.as_tensor(np.asarray(X) if not isinstance(X, torch.Tensor) else X).to(torch.float64).clamp_min(log_shift)
    Yt = torch.as_tensor(np.asarray(Y) if not isinstance(Y, torch.Tensor) else Y).to(torch.float64).clamp_min(log_shift)
    red = torch.mean if average else torch.sum
    return float((red(Yt) - red(Xt)) + (red(Xt * torch.log(Xt)) - red(Xt * torch.log(Yt))))


def KL_loss_surrogate(X, W, H, Ht, log_shift=log_shift, average=False):
    """The majoriser of the KL data term at Ht that the multiplicative H update minimises (espm/measures.py:506-522):
    sum_ij X_ij sum_k U_ikj log(U_ikj / (W_ik H_kj)) + sum(W Ht), U_ikj = W_ik Ht_kj / (W Ht)_ij.

    The inner sum over k collapses - log(U / (W H)) = log(Ht / H)_kj - log(W Ht)_ij and sum_k U = 1 - to
    (W (Ht log(Ht / H)))_ij / (W Ht)_ij - log (W Ht)_ij: two small products instead of the reference's n x k x p arrays, the same value to rounding."""
    W = np.maximum(np.asarray(W, dtype=np.float64), log_shift)
    H = np.maximum(np.asarray(H, dtype=np.float64), log_shift)
    Ht = np.maximum(np.asarray(Ht, dtype=np.float64), log_shift)
    X = np.maximum(np.asarray(X, dtype=np.float64), log_shift)
    WHt = W @ Ht
    inner = (W @ (Ht * np.log(Ht / H))) / WHt - np.log(WHt)
    if average:   # (the reference averages X * inner + sum_k W Ht over the n x p entries)
        return float(np.mean(X * inner + WHt))
    return float(np.sum(X * inner) + np.sum(WHt))


def log_surrogate(H, Ht, mu, epsilon, average=False):
    """The tangent majoriser of the log sparsity term at Ht (espm/measures.py:550-558): sum_kj mu_k (log(Ht + eps) + (H - Ht) / (Ht + eps))."""
    H, Ht = np.asarray(H), np.asarray(Ht)
    weight = mu if np.isscalar(mu) else np.asarray(mu)[:, None]
    terms = weight * (np.log(Ht + epsilon) + (H - Ht) / (Ht + epsilon))
    return np.mean(terms) if average else np.sum(terms)


def log_reg(H, mu, epsilon=1, average=False):
    """sum_ij mu_i log(H_ij + eps) (espm/measures.py:524-548); a (k, p) elementwise reduction done with
    torch on the device (plumbing - the fit loop gets this term from the fused H-step)."""
    import torch

    from espm_amd.engine import require_gpu

    dev = require_gpu()
    Hd = torch.from_numpy(np.ascontiguousarray(H, dtype=np.float64)).to(dev)
    mud = torch.as_tensor(np.asarray(mu, dtype=np.float64), device=dev)
    if mud.dim() == 1:
        mud = mud[:, None]
    t = mud * torch.log(Hd + epsilon)
    return float(t.mean() if average else t.sum())


def trace_xtLx(L, x, average=False):
    """Tr(x^T L x) = sum(x * (L x)) (espm/measures.py:560-577) with the device stencil."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream, require_gpu
    from espm_amd.utils import classify_laplacian

    x = np.asarray(x)
    xm = x.reshape(x.shape[0], -1)                  # (p, k)
    p, k = xm.shape
    kind, shape = classify_laplacian(L, p)
    dev = require_gpu()
    h = torch.from_numpy(np.ascontiguousarray(xm.T, dtype=np.float32)).to(dev)  # (k, p)
    if kind == "identity":
        hl = h
    else:
        hl = torch.empty_like(h)
        _lib.check(_lib.lib.espm_mu_laplacian(_ptr(h), k, shape[0], shape[1], p, _ptr(hl), _stream()))
    t = (h.double() * hl.double())
    return float(t.mean() if average else t.sum())


# ---- ground-truth comparison (true_D / true_H tracking, espm/estimators/base.py:335-347) --------------------------
def spectral_angle(v1, v2):
    """Angle in degrees between two spectra, or between the rows of two (phases, channels) arrays (espm/measures.py:13-47)."""
    v1, v2 = np.asarray(v1, dtype=np.float64), np.asarray(v2, dtype=np.float64)
    if v1.ndim == 1:
        if v1.shape != v2.shape:
            raise ValueError("v1 and v2 should have the same shape.")
        return np.arccos(np.clip(np.dot(v1 / np.linalg.norm(v1), v2 / np.linalg.norm(v2)), -1.0, 1.0)) * 180 / np.pi
    if v1.shape[1] != v2.shape[1]:
        raise ValueError("The second dimensions of v1 and v2 should be the same.")
    a = v1 / np.sqrt(np.sum(v1 ** 2, axis=1, keepdims=True))
    b = v2 / np.sqrt(np.sum(v2 ** 2, axis=1, keepdims=True))
    return np.arccos(np.clip(a @ b.T, -1.0, 1.0)) * 180 / np.pi


def squared_distance(x, y=None):
    """Mean squared distance between the rows of x and the rows of y (espm/measures.py:579-626)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    y = x if y is None else np.atleast_2d(np.asarray(y, dtype=np.float64))
    if x.shape[1] != y.shape[1]:
        raise ValueError("The sizes of x and y do not fit")
    xx, yy = (x * x).sum(axis=1), (y * y).sum(axis=1)
    return np.abs(xx[:, None] + yy[None, :] - 2 * np.dot(x, y.T)) / x.shape[1]


def global_min(matr):
    """Row-wise minima and their columns (espm/measures.py:157-170)."""
    import warnings
    res = [float(np.min(row)) for row in matr]
    ind = [int(np.argmin(row)) for row in matr]
    if any(ind.count(x) > 1 for x in ind):
        warnings.warn("Several results share the same truth")
    return res, ind


def unique_min(matrix):
    """The one-row-per-column assignment of a square matrix with the smallest sum, by brute force over the permutations
    (espm/measures.py:172-207; not meant for more than ~10 phases): its entries in column order and the permutation."""
    from itertools import permutations
    matrix = np.asarray(matrix)
    k = matrix.shape[0]
    perms = list(permutations(range(k), k))
    sums = [sum(matrix[perm[i], i] for i in range(k)) for perm in perms]
    best = perms[sums.index(min(sums))]
    return [matrix[best[i], i] for i in range(k)], best


def find_min_angle(true_vectors, algo_vectors, get_ind=False, unique=False):
    """Best match of NMF spectra to true spectra by spectral angle (espm/measures.py:125-155)."""
    out = (unique_min if unique else global_min)(spectral_angle(true_vectors, algo_vectors))
    return out if get_ind else out[0]


def find_min_MSE(true_maps, algo_maps, get_ind=False, unique=False):
    """Best match of NMF maps to true maps by mean squared error (espm/measures.py:244-270)."""
    out = (unique_min if unique else global_min)(squared_distance(true_maps, algo_maps))
    return out if get_ind else out[0]


def mse(map1, map2):
    """Mean squared error between two maps (espm/measures.py:51-72)."""
    return np.mean((np.asarray(map1) - np.asarray(map2)) ** 2)


def mae(map1, map2):
    """Mean absolute error between two maps (espm/measures.py:75-96)."""
    return np.mean(np.abs(np.asarray(map1) - np.asarray(map2)))


def r2(map_true, map_pred):
    """Coefficient of determination between two maps, every leading index an output (espm/measures.py:99-119: scikit-learn's r2_score
    on the maps reshaped to (first axis, rest))."""
    from sklearn.metrics import r2_score
    a, b = np.asarray(map_true), np.asarray(map_pred)
    return r2_score(a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1))


def ordered_r2(true_maps, algo_maps, input_inds):
    """R^2 of every phase for a given correspondence (espm/measures.py:315-327)."""
    return [float(r2(true_maps[j], algo_maps[i])) for i, j in enumerate(input_inds)]


def ordered_mse(true_maps, algo_maps, input_inds):
    """MSE of every phase for a given correspondence (espm/measures.py:287-299)."""
    return [float(mse(true_maps[j], algo_maps[i])) for i, j in enumerate(input_inds)]


def ordered_mae(true_maps, algo_maps, input_inds):
    """MAE of every phase for a given correspondence (espm/measures.py:301-313)."""
    return [float(mae(true_maps[j], algo_maps[i])) for i, j in enumerate(input_inds)]


def ordered_angles(true_spectra, algo_spectra, input_inds):
    """Spectral angle of every phase for a given correspondence (espm/measures.py:330-339)."""
    return [spectral_angle(true_spectra[j], algo_spectra[i]) for i, j in enumerate(input_inds)]


def find_min_config(true_maps, true_spectra, algo_maps, algo_spectra, angles=True):
    """Best match of NMF phases to the truth by angles (or by map errors) and whether the two criteria agree
    (espm/measures.py:222-256)."""
    min_MSE_config = find_min_MSE(true_maps, algo_maps, get_ind=True, unique=True)[1]
    min_angle_config = find_min_angle(true_spectra, algo_spectra, get_ind=True, unique=True)[1]
    warning = False
    if min_MSE_config != min_angle_config:
        print("WARNING : angles and mse disagree there's probably an issue")
        warning = True
    if angles:
        return (find_min_angle(true_spectra, algo_spectra, unique=True), ordered_mse(true_maps, algo_maps, min_angle_config),
                min_angle_config, warning)
    return (ordered_angles(true_spectra, algo_spectra, min_MSE_config), find_min_MSE(true_maps, algo_maps, unique=True),
            min_MSE_config, warning)


def Frobenius_loss(X, W, H, average=False):
    """||X - W H||_F^2 (espm/measures.py:350-384): one GEMM and an element-wise reduction with torch on the device."""
    import torch

    from espm_amd.engine import require_gpu
    dev = require_gpu()
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)
    r = Xd - torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).to(dev) @ torch.from_numpy(np.ascontiguousarray(H, dtype=np.float64)).to(dev)
    t = r * r
    return float(t.mean() if average else t.sum())


# ---- per-pixel diagnostics of a fitted model (csrc/mu_diag.hip) ------------------------------------------------------------------
def pixel_diagnostics(X, D, H, *, simplex_H=False, log_shift=log_shift, layout="cm", device=None):
    """Where the model D H fails and how well every abundance is known: per pixel j, with Y = max(D H, log_shift),

    * ``deviance`` (p,): 2 sum_c (x ln(x / y) - x + y), the Poisson (KL) deviance of the pixel's spectrum - hyperspy's ``red_chisq``
      map for counts;
    * ``H_std`` (k, p): sqrt(diag(C_j)), the Cramer-Rao bound of H[:, j] given the spectra - hyperspy's parameter ``std``.
      C_j = F_j^-1 with the expected Fisher information F_j = D^T diag(1 / y[:, j]) D; under ``simplex_H`` the bound with
      sum_i h_i = 1, C = F^-1 - F^-1 1 1^T F^-1 / (1^T F^-1 1) (exactly 0 for one component);
    * ``n_singular``: the pixels whose F_j has a Cholesky pivot that is not above k eps max diag(F_j); their column of ``H_std`` is NaN.

    What the bound leaves out: the uncertainty of D itself, the regularisers of the fit (mu, lambda_L) and abundances held at the
    ``log_shift`` floor.  It is the error bar "given the spectra", as hyperspy's ``std`` is "given the model".

    X: the image as measured (no log_shift fill, no normalisation), non-negative, (channels, pixels) for ``layout="cm"`` or
    (pixels, channels) for "pm" - a host array (uploaded in row chunks in its own dtype) or a device tensor.  u8, u16, f32 and f64
    are read as they are; other integer dtypes and float16 are converted to f32 or f64, whichever holds them exactly.  D (n, k) is
    G W in counts, H (k, p); 1..8 components.  Everything is computed in fp64 by one HIP kernel; there is no CPU path.  Returns a
    dict of float64 numpy arrays and the int ``n_singular``."""
    from espm_amd import _lib
    X = check_image(X)
    n, p, k, D, H = check_model(D, H, "pixel_diagnostics", _lib.DIAG_MAX_K, tuple(X.shape), layout)
    check_log_shift(log_shift)
    import torch

    from espm_amd.engine import _ptr, _stream

    img = _image.Resident(X, layout, device).upload()
    dev = img.dev
    with img.scope():
        Dd, Hd = img.model(D, H)
        dv = torch.empty(p, dtype=torch.float64, device=dev)
        hs = torch.empty((k, p), dtype=torch.float64, device=dev)
        ns = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib.espm_pixel_diagnostics(*img.abi(), _ptr(Dd), _ptr(Hd), k, float(log_shift), int(bool(simplex_H)), _ptr(dv),
                                                   _ptr(hs), _ptr(ns), _stream()))
        return dict(deviance=dv.cpu().numpy(), H_std=hs.cpu().numpy(), n_singular=int(ns.item()))


# ---- per-channel diagnostics of a fitted model (csrc/mu_diag_chan.hip) -------------------------------------------------------------
_SPECTRAL_MAX_F = 2048   # rows of the dense information matrix of a dictionary fit (m k): above it, it is no small matrix any more


def _spd_inverse(A):
    """(A^-1, bad) of symmetric matrices (..., N, N) by LAPACK's Cholesky A = L L^T, whose squared diagonal holds the pivots of the
    root-free form the pixel kernel uses, with that kernel's rule: a pivot that is not above N eps max diag(A) marks the matrix
    singular.  A^-1 = L^-T L^-1.  Singular matrices (``bad``) come back as NaN."""
    A = np.array(A, dtype=np.float64, copy=True)
    N = A.shape[-1]
    eye = np.eye(N)
    thr = N * np.finfo(np.float64).eps * np.max(np.diagonal(A, axis1=-2, axis2=-1), axis=-1)
    bad = ~np.isfinite(A).all(axis=(-2, -1))
    A[bad] = eye
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:   # a pivot <= 0 somewhere in the stack: find which matrices, one by one
        flat, fbad = A.reshape(-1, N, N), bad.reshape(-1).copy()
        for c in range(flat.shape[0]):
            try:
                np.linalg.cholesky(flat[c])
            except np.linalg.LinAlgError:
                fbad[c] = True
        bad = fbad.reshape(bad.shape)
        A[bad] = eye
        L = np.linalg.cholesky(A)
    bad = bad | ~(np.diagonal(L, axis1=-2, axis2=-1) ** 2 > thr[..., None]).all(axis=-1)
    L[bad] = eye
    Z = np.linalg.inv(L)
    S = np.swapaxes(Z, -1, -2) @ Z
    S[bad] = np.nan
    return S, bad


def _simplex_rows(simplex_rows, rows):
    """None (no constraint), True (all ``rows`` rows of W) or an index array -> None or a sorted array of distinct row indices."""
    if simplex_rows is None or simplex_rows is False:
        return None
    if simplex_rows is True:
        return np.arange(rows)
    idx = np.unique(np.asarray(simplex_rows).astype(np.int64).ravel())
    if idx.size == 0:
        return None
    if idx[0] < 0 or idx[-1] >= rows:
        raise ValueError(f"simplex_rows must index the {rows} rows of W")
    return idx


def _sqrt_var(v):
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.where(v < 0, 0.0, v))   # (a rounding-negative variance is 0; a NaN stays)


def _constrained(free, sub, N):
    """free - sub, the variance left by a constraint; a difference at the rounding level of ``free`` (an entry the constraint
    leaves no freedom, such as the only row of its set) is 0."""
    with np.errstate(invalid="ignore"):
        return np.where(free - sub <= 8 * N * np.finfo(np.float64).eps * free, 0.0, free - sub)


def spectral_bounds(M, G=None, simplex_rows=None):
    """The host half of ``spectral_diagnostics``: from the per-channel information M (n, k, k) to the Cramer-Rao bounds
    dict(W_std, D_std (n, k), n_singular), in fp64 numpy - nothing here depends on the pixels.

    ``G=None``: W is D, the information is block diagonal, S_c = M_c^-1 by Cholesky (``_spd_inverse``); a channel whose M_c fails the
    pivot rule (a pivot not above k eps max diag(M_c)) is NaN.  Under the simplex sum_{c in rows} W[c, a] = 1 the rows of the set
    get diag(S_c - S_c T^-1 S_c) with T the sum of S_c over the regular rows of the set (NaN rows are left out of T: they are
    treated as held, not as free); rows outside the set keep S_c.
    ``G`` (n, m): F[(i, a), (j, b)] = sum_c G[c, i] G[c, j] M_c[a, b], dense (m k)^2, C = F^-1 (the pivot rule with m k in place of
    k; a singular F makes every entry NaN), under the simplex C - C A (A^T C A)^-1 A^T C with A[(i, a), b] = delta_ab for i in
    ``simplex_rows``; W_std[i, a] = sqrt(C[(i, a), (i, a)]), D_std[c, a] = sqrt(g_c^T C_aa g_c)."""
    M = np.asarray(M, dtype=np.float64)
    n, k = M.shape[0], M.shape[1]
    if G is None:
        rows = _simplex_rows(simplex_rows, n)
        S, bad = _spd_inverse(M)
        var = np.einsum("cii->ci", S).copy()
        if rows is not None:
            reg = rows[~bad[rows]]
            if reg.size:
                Tinv, tbad = _spd_inverse(S[reg].sum(axis=0))
                if tbad:
                    var[reg] = np.nan
                else:
                    var[reg] = _constrained(var[reg], np.einsum("cij,jl,cli->ci", S[reg], Tinv, S[reg]), k)
        W_std = _sqrt_var(var)
        return dict(W_std=W_std, D_std=W_std.copy(), n_singular=int(np.isnan(W_std).any(axis=1).sum()))
    G = np.asarray(G, dtype=np.float64)
    m = G.shape[1]
    rows = _simplex_rows(simplex_rows, m)
    F = np.empty((m, k, m, k), dtype=np.float64)
    for a in range(k):
        for b in range(a + 1):
            P = G.T @ (M[:, a, b][:, None] * G)
            P = 0.5 * (P + P.T)
            F[:, a, :, b] = P
            F[:, b, :, a] = P
    C, bad = _spd_inverse(F.reshape(m * k, m * k))

    def variances(C):   # diag(C) as (m, k) and g_c^T C_aa g_c as (n, k)
        C4 = C.reshape(m, k, m, k)
        return (np.einsum("iaia->ia", C4).copy(),
                np.stack([((G @ np.ascontiguousarray(C4[:, a, :, a])) * G).sum(axis=1) for a in range(k)], axis=1))

    var_W, var_D = variances(C)
    if not bad and rows is not None:
        A = np.zeros((m, k, k), dtype=np.float64)
        A[rows] = np.eye(k)
        A = A.reshape(m * k, k)
        CA = C @ A
        Tinv, tbad = _spd_inverse(A.T @ CA)
        if tbad:
            var_W[:], var_D[:] = np.nan, np.nan
        else:
            sub_W, sub_D = variances(CA @ Tinv @ CA.T)
            var_W, var_D = _constrained(var_W, sub_W, m * k), _constrained(var_D, sub_D, m * k)
    W_std, D_std = _sqrt_var(var_W), _sqrt_var(var_D)
    return dict(W_std=W_std, D_std=D_std, n_singular=int(np.isnan(W_std).any(axis=1).sum()))


def spectral_diagnostics(X, D_or_W, H, *, G=None, simplex_rows=None, log_shift=log_shift, layout="cm", device=None):
    """In which energy channels the model fails and how well every spectrum is known - the transpose side of ``pixel_diagnostics``.
    Per channel c, with Y = max(D H, log_shift) and D = ``D_or_W`` (or ``G @ D_or_W`` with a dictionary ``G`` (n, m) and W (m, k)):

    * ``channel_deviance`` (n,): 2 sum_p (x ln(x / y) - x + y), the residual spectrum - a missing line shows as a narrow band of
      channels the model does not fit;
    * ``sum_spectrum``, ``model_spectrum`` (n,): sum_p x and sum_p y, to plot it next to;
    * ``M`` (n, k, k): M_c = sum_p h_p h_p^T / y_cp, the expected Fisher information of row c of D with the abundances held;
    * ``W_std``, of W's shape: the Cramer-Rao bound of every entry of W given H, and ``D_std`` (n, k): the bound on the spectra
      D = G W (``spectral_bounds`` holds the algebra; without G both are sqrt(diag(M_c^-1)));
    * ``n_singular``: the rows of ``W_std`` that are NaN - channels whose M_c has a Cholesky pivot that is not above
      k eps max diag(M_c), or all m rows when the dictionary's information matrix fails the same rule.

    ``simplex_rows``: None for no constraint, True for sum_c W[c, a] = 1 over all rows of W, or the indices of the rows that sum
    to one (a physics model's ``NMF_simplex()``).  Singular rows are left out of the constraint's sum: they stay NaN and the
    regular rows are bounded as if the singular ones were held.

    What the bound leaves out: the uncertainty of H itself, the regularisers of the fit (mu, lambda_L) and entries of W held at the
    ``log_shift`` floor.  It is the error bar "given the abundances", as ``pixel_diagnostics`` gives the one "given the spectra".

    X, ``layout``, ``device`` and the dtype rules are those of ``pixel_diagnostics``; 1..8 components; a dictionary with m k above
    2048 raises NotImplementedError.  The pass over X is one fp64 HIP kernel that reduces over the pixels without atomics (two
    calls give the same bits; so do the two layouts); there is no CPU path.  The step from M to the bounds does not depend on the
    pixels and is fp64 numpy on the host.  Returns a dict of float64 numpy arrays and the int ``n_singular``."""
    from espm_amd import _lib
    W = np.asarray(D_or_W, dtype=np.float64)
    if W.ndim == 2 and W.shape[1] > _lib.DIAG_MAX_K:
        raise NotImplementedError(f"spectral_diagnostics: {W.shape[1]} components (the kernel is built for 1..{_lib.DIAG_MAX_K})")
    if G is not None:
        G = np.asarray(G, dtype=np.float64)
        if G.ndim != 2 or W.ndim != 2 or G.shape[1] != W.shape[0]:
            raise ValueError(f"G must be (channels, m) and W (m, k): got {G.shape} and {W.shape}")
        if G.shape[1] * W.shape[1] > _SPECTRAL_MAX_F:
            raise NotImplementedError(f"spectral_diagnostics: a dictionary of {G.shape[1]} entries x {W.shape[1]} components gives an "
                                      f"information matrix of {G.shape[1] * W.shape[1]} rows (at most {_SPECTRAL_MAX_F})")
        D = G @ W
    else:
        D = W
    X = check_image(X)
    n, p, k, D, H = check_model(D, H, "spectral_diagnostics", _lib.DIAG_MAX_K, tuple(X.shape), layout)
    check_log_shift(log_shift)
    _simplex_rows(simplex_rows, W.shape[0])   # (an index out of range: before the upload)
    import torch

    from espm_amd.engine import _ptr, _stream

    img = _image.Resident(X, layout, device).upload()
    dev = img.dev
    nt = k * (k + 1) // 2
    with img.scope():
        Dd, Hd = img.model(D, H)
        out = torch.empty((3 + nt) * n, dtype=torch.float64, device=dev)   # dev, xsum, ysum, then m_tri (n, nt)
        nbytes = int(_lib.lib.espm_channel_diagnostics_scratch(n, p, k))
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib.espm_channel_diagnostics(*img.abi(), _ptr(Dd), _ptr(Hd), k, float(log_shift), _ptr(out[:n]),
                                                     _ptr(out[n:2 * n]), _ptr(out[2 * n:3 * n]), _ptr(out[3 * n:]), _ptr(scratch),
                                                     nbytes, _stream()))
        host = out.cpu().numpy()
    tri = host[3 * n:].reshape(n, nt)
    M = np.empty((n, k, k), dtype=np.float64)
    il, jl = np.tril_indices(k)   # row by row: (0,0), (1,0), (1,1), (2,0), ...
    M[:, il, jl] = tri
    M[:, jl, il] = tri
    res = dict(channel_deviance=host[:n].copy(), sum_spectrum=host[n:2 * n].copy(), model_spectrum=host[2 * n:3 * n].copy(), M=M)
    res.update(spectral_bounds(M, G=G, simplex_rows=simplex_rows))
    return res
