"""Residual components on the device (csrc/mu_residual.hip): the leading singular triplets of the Pearson residual matrix

    E = (X - Y) / sqrt(Y),  Y = D H,

the two things every user of an NMF decomposition asks first.  AFTER a fit - is a phase missing, and what does it look like?  For a
correct Poisson model every entry of E has mean 0 and variance 1, E looks like noise and its top singular value sits near
``edge`` = sqrt(n) + sqrt(p); a missing phase is a singular value far above that, its left vector the residual spectrum and its right
vector the map of where the phase sits.  BEFORE a fit - how many components does the map hold?  Against the independence model
y_cj = r_c c_j / T (channel sums times pixel sums over the total, ``independence_model``) the same matrix is correspondence analysis,
and its singular values are sqrt(T) times the non-trivial ones of hyperspy's Poisson-normalised PCA: ``scree``.  The reference has
neither.

E is never stored: ``svd`` is a block subspace iteration (block of 8) whose every step is a pass over X (``products``, the entry
point espm_residual_products: E^T U or E V for 8 vectors at once, defined by a rule in fp64, in a fixed order, without atomics - two
calls, and the two layouts of one image, give the same bits).  An entry whose model is below ``log_shift`` leaves E (e = 0) and, where
it holds counts, is counted in ``unmodelled``: a single one at Y = log_shift would carry e ~ 1e7 and own the whole decomposition.

At EDS doses the Pearson residual is heavy-tailed (fourth moment 3 + 1 / Y), so the analytic edge is only a guide: the honest scale
is a sampled null, ``null_singular_values`` - the top singular value of replicates of the model drawn on the device
(``espm_amd.sampling``) against the model itself - and ``calibrate``.

The iteration is written around a ``products`` callable (``_subspace_iteration``), so it runs on any implementation of the two
products; ``calibrate`` is numpy; everything else needs the GPU (there is no CPU path)."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import (check_image, check_layout, check_log_shift, check_model, check_seed, image_dims, is_tensor,
                                  narrowed_image)

MAX_G = 8        # ESPM_RESID_MAX_G: vectors per launch (any number is accepted, in batches)
MAX_K = 8        # ESPM_RESID_MAX_K: components of the model
BLOCK = 8        # the block of the subspace iteration: the vectors asked for and the oversampling
MAX_VECTORS = 6  # singular triplets svd returns at most


def _side(side):
    if side not in ("pixels", "channels"):
        raise ValueError(f"side must be 'pixels' (E^T U, a value per pixel) or 'channels' (E V, a value per channel), not {side!r}")
    return side == "pixels"


def _host_vectors(V, m, axis, who):
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 1:
        V = V[None, :]
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] != m:
        raise ValueError(f"{who}: vectors of shape {V.shape} for {m} {axis} (one row of {m} per vector)")
    if not np.isfinite(V).all():
        raise ValueError(f"{who}: the vectors hold values that are not finite")
    return np.ascontiguousarray(V)


class _Pass:
    """X and a model, checked on the host and then uploaded ONCE (``image``, by the narrowing rule): every ``run`` is a pass over
    the resident image.  The vectors and the scratch are its own."""

    def __init__(self, X, D, H, log_shift, layout, who):
        check_layout(layout)
        X = check_image(X)
        if D is None or H is None:
            raise ValueError(f"{who}: a model D (channels, components), H (components, pixels) is required")
        self.n, self.p, self.k, D, H = check_model(D, H, who, MAX_K, tuple(X.shape), layout)
        self.who, self.log_shift = who, check_log_shift(log_shift)
        for name, A in (("D", D), ("H", H)):
            if not np.isfinite(A).all():
                raise ValueError(f"{who}: {name} holds values that are not finite")
        self.image, self._model, self.scratch = _image.Resident(narrowed_image(X, who), layout), (D, H), None

    def check_vectors(self, vectors, pixel_side):
        """The vectors as they go to the device: a checked host array, or a device tensor checked where it is."""
        m, axis = (self.n, "channels") if pixel_side else (self.p, "pixels")
        if not is_tensor(vectors):
            return _host_vectors(vectors, m, axis, self.who)
        import torch
        V = vectors if vectors.ndim == 2 else vectors[None, :]
        if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] != m:
            raise ValueError(f"{self.who}: vectors of shape {tuple(vectors.shape)} for {m} {axis} (one row of {m} per vector)")
        if V.dtype != torch.float64:
            raise ValueError(f"{self.who}: device vectors must be float64, not {V.dtype}")
        if not bool(torch.isfinite(V).all()):
            raise ValueError(f"{self.who}: the vectors hold values that are not finite")
        return V

    def upload(self):
        if self.scratch is not None:
            return
        import torch

        from espm_amd import _lib
        self.dev = self.image.upload().dev
        with self.image.scope():
            self.Dd, self.Hd = self.image.model(*self._model)
            self.need = int(_lib.lib.espm_residual_products_scratch(_lib.RESID_CHANNELS, self.n, self.p, MAX_G))
            self.scratch = torch.empty(max(self.need, 8), dtype=torch.uint8, device=self.dev)
        self._model = None

    def run(self, vectors, pixel_side, chi2=False, device=False):
        """dict(out (g, p) or (g, n), chi2 or None, unmodelled) for checked ``vectors``; ``device``: out and chi2 stay on the GPU."""
        import torch

        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        self.upload()
        side = _lib.RESID_PIXELS if pixel_side else _lib.RESID_CHANNELS
        m = self.p if pixel_side else self.n
        with self.image.scope():
            V = vectors.to(self.dev).contiguous() if is_tensor(vectors) else torch.from_numpy(vectors).to(self.dev)
            g = int(V.shape[0])
            out = torch.empty((g, m), dtype=torch.float64, device=self.dev)
            c2 = torch.empty(m, dtype=torch.float64, device=self.dev) if chi2 else None
            un = torch.zeros(1, dtype=torch.int64, device=self.dev)
            for b in range(0, g, MAX_G):   # (chi2 and the count belong to E, not to the vectors: the first batch forms them)
                gb = min(MAX_G, g - b)
                _lib.check(_lib.lib.espm_residual_products(*self.image.abi(), side, _ptr(V[b:b + gb]), gb, _ptr(self.Dd), _ptr(self.Hd), self.k,
                                                           self.log_shift, _ptr(out[b:b + gb]), _ptr(c2 if b == 0 else None),
                                                           _ptr(un if b == 0 else None), _ptr(self.scratch), self.need, _stream()))
            unmodelled = int(un.cpu().numpy()[0])
            if not device:
                out, c2 = out.cpu().numpy(), (None if c2 is None else c2.cpu().numpy())
        return dict(out=out, chi2=c2, unmodelled=unmodelled)

    def products(self, side, vectors, chi2=False):
        """The callable ``_subspace_iteration`` takes: the pixel side's block stays on the device, the channel side's comes to the host."""
        pixel_side = _side(side)
        return self.run(self.check_vectors(vectors, pixel_side), pixel_side, chi2=chi2, device=pixel_side)


def products(X, vectors, D, H, side="pixels", log_shift=1e-14, layout="cm", chi2=False, device=False):
    """The Pearson residual matrix E = (X - D H) / sqrt(D H) applied to a block of vectors, dict(

    * ``out``: ``side="pixels"`` - ``vectors`` (g, n), a value per channel - (g, p): sum_c vectors[q, c] e_cj, that is E^T U;
      ``side="channels"`` - ``vectors`` (g, p), a value per pixel - (g, n): sum_j vectors[q, j] e_cj, that is E V;
    * ``chi2``: with ``chi2=True`` the Pearson chi^2 sum e^2 of every pixel (p,) or channel (n,), else None;
    * ``unmodelled``: the entries with counts whose model is below ``log_shift``; they and every other entry below it have e = 0).

    X: the image as measured, (channels, pixels) for ``layout="cm"`` or (pixels, channels) for "pm", a host array or a device
    tensor, checked and uploaded once by the narrowing rule (``_image_args.narrowed_image``).  D (n, k), H (k, p): 1 .. 8 components
    (NotImplementedError beyond).  ``vectors``: a host array or a device float64 tensor, any number of them (8 per launch).  ``device=True`` leaves
    ``out`` and ``chi2`` on the GPU.  ValueError for shapes that do not match and for X, vectors or a model that are not finite -
    all before anything is uploaded.  Sums in fp64 in a fixed order without atomics: two calls and both layouts give the same bits."""
    pixel_side = _side(side)
    ps = _Pass(X, D, H, log_shift, layout, "products")
    return ps.run(ps.check_vectors(vectors, pixel_side), pixel_side, chi2=chi2, device=device)


# ---- the subspace iteration -----------------------------------------------------------------------------------------------------------
def start_block(n, seed, block=BLOCK):
    """U0 (n, min(block, n)): the Q of a Gaussian (n, block) drawn from ``np.random.default_rng(seed)`` - a function of (n, seed) alone."""
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((n, block)))[0]


def _orthonormal_rows(V):
    """The rows of V (b, p) orthonormalised, where V lives."""
    if is_tensor(V):
        from espm_amd.init_device import _qr_tall
        return _qr_tall(V.T.contiguous()).T.contiguous()
    return np.ascontiguousarray(np.linalg.qr(V.T)[0].T)


def _rotate(M, V):
    if is_tensor(V):
        import torch
        return torch.from_numpy(np.ascontiguousarray(M)).to(V.device) @ V
    return M @ V


def _check_iteration(n_vectors, tol, max_iter, n, p):
    if isinstance(n_vectors, bool) or int(n_vectors) != n_vectors or not 1 <= int(n_vectors) <= MAX_VECTORS:
        raise ValueError(f"n_vectors must be 1 .. {MAX_VECTORS} (the block of {BLOCK} is the oversampling), not {n_vectors!r}")
    if int(n_vectors) > min(n, p):
        raise ValueError(f"n_vectors = {n_vectors} of a {n} x {p} matrix")
    if not tol > 0:
        raise ValueError("tol must be positive")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"max_iter must be a positive integer, not {max_iter!r}")
    return int(n_vectors), float(tol), int(max_iter)


def _subspace_iteration(products, n, p, n_vectors=4, tol=1e-10, max_iter=60, seed=0):
    """Block subspace iteration for the leading singular triplets of the n x p matrix E behind ``products(side, vectors, chi2=False)``
    -> dict(out, chi2, unmodelled): ("pixels", (b, n)) gives E^T U as (b, p), in whatever array type the callable likes (a device
    tensor stays on the device); ("channels", that array type (b, p)) gives E V as a host (b, n).

    From U0 = ``start_block(n, seed)``; one iteration: V <- E^T U; V orthonormalised; Z <- E V; U, R <- qr(Z^T) - the Ritz values are
    the singular values of R.  Stops when the largest relative change of the leading ``n_vectors`` Ritz values is below ``tol``, or at
    ``max_iter``.  Then U and V are rotated to the Ritz vectors (E V^T = U R = (U A) S B^T: spectra U A, maps B^T V), one more
    pixel-side pass gives the Ritz residuals rho_i = ||E^T u_i - s_i v_i||_2 - a true singular value lies within rho_i of s_i - with
    chi2 and the unmodelled count, and every spectrum's largest-magnitude entry is made positive."""
    r, tol, max_iter = _check_iteration(n_vectors, tol, max_iter, n, p)
    U = start_block(n, seed, min(BLOCK, p))   # (n, b), b = min(BLOCK, n, p)
    ritz, n_iter, converged = None, 0, False
    while n_iter < max_iter and not converged:
        V = _orthonormal_rows(products("pixels", np.ascontiguousarray(U.T))["out"])
        Z = _image.to_host(products("channels", V)["out"])
        U, R = np.linalg.qr(Z.T)
        s = np.linalg.svd(R, compute_uv=False)
        n_iter += 1
        if ritz is not None:
            change = np.abs(s[:r] - ritz[:r]) / np.maximum(s[:r], np.finfo(np.float64).tiny)
            converged = bool(change.max() < tol)
        ritz = s
    A, s, Bt = np.linalg.svd(R)
    spectra = (U @ A)[:, :r]
    maps = _rotate(Bt[:r], V)
    last = products("pixels", np.ascontiguousarray(spectra.T), chi2=True)
    maps, back = _image.to_host(maps), _image.to_host(last["out"])
    sv = s[:r]
    rho = np.linalg.norm(back - sv[:, None] * maps, axis=1)
    sign = np.where(spectra[np.abs(spectra).argmax(axis=0), np.arange(r)] < 0, -1.0, 1.0)
    chi2_map = _image.to_host(last["chi2"])
    total = float(chi2_map.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        explained = sv * sv / total
    return dict(singular_values=sv, spectra=np.ascontiguousarray(spectra * sign[None, :]), maps=np.ascontiguousarray(maps * sign[:, None]),
                ritz_residuals=rho, chi2_total=total, chi2_map=chi2_map, explained=explained, edge=float(np.sqrt(n) + np.sqrt(p)),
                n_iter=n_iter, converged=converged, unmodelled=int(last["unmodelled"]))


def _svd_of(ps, n_vectors, tol, max_iter, seed):
    _check_iteration(n_vectors, tol, max_iter, ps.n, ps.p)
    return _subspace_iteration(ps.products, ps.n, ps.p, n_vectors=n_vectors, tol=tol, max_iter=max_iter, seed=seed)


def svd(X, D, H, n_vectors=4, tol=1e-10, max_iter=60, seed=0, log_shift=1e-14, layout="cm"):
    """The leading singular triplets of the Pearson residual matrix E = (X - D H) / sqrt(D H) of a model, dict(

    * ``singular_values`` (r,), descending; ``spectra`` (n, r): the left vectors, each with its largest-magnitude entry positive;
      ``maps`` (r, p): the right vectors;
    * ``ritz_residuals`` (r,): rho_i = ||E^T u_i - s_i v_i||_2 - a true singular value of E lies within rho_i of s_i;
    * ``chi2_total``: sum e^2 = ||E||_F^2; ``chi2_map`` (p,): per pixel; ``explained`` (r,) = s^2 / chi2_total;
    * ``edge`` = sqrt(n) + sqrt(p): where the top singular value of pure unit-variance noise sits - a guide only at EDS doses, where
      e is heavy-tailed: ``null_singular_values`` has the honest scale;
    * ``n_iter``, ``converged``, ``unmodelled`` (as for ``products``)).

    Block subspace iteration with a block of 8 (``_subspace_iteration``): two passes over X per iteration, X uploaded once, the
    p-long block kept and orthonormalised on the device.  ``n_vectors``: 1 .. 6 (ValueError beyond; the rest of the block is the
    oversampling); ``tol``: on the relative change of the Ritz values; ``seed``: of the Gaussian start.  X, D, H, ``layout`` and the
    refusals as for ``products``."""
    return _svd_of(_Pass(X, D, H, log_shift, layout, "svd"), n_vectors, tol, max_iter, seed)


# ---- the scree plot: E against the independence model ---------------------------------------------------------------------------------
def independence_model(X, layout="cm"):
    """(D (n, 1), H (1, p)) with D H = r c^T / T: the channel sums r times the pixel sums c over the total T - the model of an image
    whose every pixel has the same spectrum.  D = r / T, H = c.  The sums are ``marginals.channel_spectra`` / ``pixel_maps`` under
    all-ones weights without a model: exact for integer X.  ValueError for an image without a count."""
    from espm_amd import marginals
    check_layout(layout)
    X = check_image(X)
    n, p = image_dims(X.shape, layout)
    c = marginals.pixel_maps(X, np.ones((1, n)), layout=layout)["counts"][0]
    r = marginals.channel_spectra(X, np.ones((1, p)), layout=layout)["counts"][:, 0]
    T = float(c.sum())
    if not T > 0:
        raise ValueError("independence_model: the image holds no count")
    return np.ascontiguousarray((r / T)[:, None]), np.ascontiguousarray(c[None, :])


def scree(X, n_vectors=6, tol=1e-10, max_iter=60, seed=0, log_shift=1e-14, layout="cm"):
    """``svd`` of X against its own ``independence_model``: correspondence analysis, the scree plot that says how many components a
    map holds before anything is fitted - k phases show as k - 1 values above the bulk near ``edge``.  Returns ``svd``'s dict with
    ``normalised_pca`` (r,) = singular_values / sqrt(T), the values hyperspy's Poisson-normalised PCA reports beyond its trivial first
    one (which is 1), and ``total_counts`` = T.  X is uploaded once; arguments and refusals as for ``svd``."""
    check_layout(layout)
    X = check_image(X)
    _check_iteration(n_vectors, tol, max_iter, *image_dims(X.shape, layout))
    check_log_shift(log_shift)
    Xd = _image.Resident(narrowed_image(X, "scree"), layout).upload().Xd
    D, H = independence_model(Xd, layout=layout)
    out = _svd_of(_Pass(Xd, D, H, log_shift, layout, "scree"), n_vectors, tol, max_iter, seed)
    T = float(H.sum())
    out["normalised_pca"], out["total_counts"] = out["singular_values"] / np.sqrt(T), T
    return out


# ---- the sampled null -----------------------------------------------------------------------------------------------------------------
def null_singular_values(D, H, n_rep=10, seed=0, replicate0=0, log_shift=1e-14, tol=1e-8, max_iter=60):
    """(n_rep,) float64: the top singular value of the Pearson residual of the replicates ``replicate0 .. replicate0 + n_rep - 1`` of
    the model D (n, k) H (k, p) (``espm_amd.sampling``'s rule under ``seed``) against the model itself - the distribution the top
    singular value has when the model is right.  Each replicate is drawn on the device as 16-bit counts and stays there; ``svd`` with
    one vector follows (``tol``, ``max_iter``; its start is the same for every replicate).  D and H are checked as ``sampling.sample``
    checks them, 1 .. 8 components; ValueError if a replicate has saturated entries or entries without a valid rate, as ``simulate``
    raises."""
    from espm_amd import sampling
    seed, n_rep = check_seed(seed), sampling._check_n_rep(n_rep)
    replicate0 = sampling._check_replicate(replicate0, n_rep)
    check_log_shift(log_shift)
    n, p, _, D, H = check_model(D, H, "null_singular_values", MAX_K)
    _check_iteration(1, tol, max_iter, n, p)
    D, H = sampling._model(D, H)
    Dd, Hd, dev = sampling._upload(D, H)
    out = np.empty(n_rep)
    for r in range(n_rep):
        Xr, saturated, invalid = sampling._draw(Dd, Hd, dev, seed, replicate0 + r, np.dtype(np.uint16), "cm")
        if saturated or invalid:
            raise ValueError(f"null_singular_values: replicate {replicate0 + r} has {saturated} saturated entries and {invalid} "
                             "without a valid rate")
        out[r] = _svd_of(_Pass(Xr, D, H, log_shift, "cm", "null_singular_values"), 1, tol, max_iter, 0)["singular_values"][0]
    return out


def calibrate(singular_values, null):
    """The singular values on the scale of the sampled null of the top one: dict(``pvalue`` of singular_values[0] =
    (1 + #{r : null_r >= s_1}) / (n_rep + 1), the Monte-Carlo p-value (never 0), ``n_significant``: the number of leading values above
    the largest null value - for the second and later ones a conservative comparison, the null being that of the top value).  Host
    numpy."""
    s, null = np.asarray(singular_values, dtype=np.float64), np.asarray(null, dtype=np.float64)
    if s.ndim != 1 or s.size < 1 or null.ndim != 1 or null.size < 1:
        raise ValueError("singular_values must be (r,) and null (n_rep,), both non-empty")
    if not (np.isfinite(s).all() and np.isfinite(null).all()):
        raise ValueError("calibrate: values that are not finite")
    above = s > null.max()
    n_significant = int(s.size if above.all() else np.argmin(above))
    return dict(pvalue=float((1.0 + (null >= s[0]).sum()) / (null.size + 1.0)), n_significant=n_significant)
