"""Element presence on the device (csrc/mu_spectra_ml.hip): is element e in phase j at all?

With a dictionary or physics model G (channels x elements) the fitted ``W_`` (elements x phases) is the quantitative result, and a
trace element is an entry of it at or near zero - where the Wald bar of ``measures.spectral_diagnostics`` (``W_std``, from the
expected information, blind to active floors) means nothing.  The honest statistic at a boundary is a likelihood ratio between
nested models: the best Poisson fit of W >= 0 with the abundances H held against the best fit with entry (e, j) held at zero.

The estimation problem is the pixel problem of ``espm_amd.presence`` once more: ONE "pixel" whose observations are all n p entries
of X and whose design columns are g_e (x) h_j.  The certificate, the scale onto the ray and the safeguarded Newton rule carry over
(DESIGN.md section 4); tests/spectra_ml_reference.py restates the rule in numpy and is its definition.

* ``ml_spectra``: the ML W over a free set of entries, every pass one fp64 HIP pass over the resident image (the entry point
  espm_spectra_ml_pass: per-channel deviance, Q = (X / Y) H^T and the observed information A_c = sum_p (x / y^2) h h^T, reduced
  over the pixels without float atomics) followed by small dense algebra on m k <= 2048 unknowns in torch fp64 on the device, and
  ONE small read-back (deviance, gap, the decision);
* ``presence``: the full fit, then for every tested entry the fit without it, warm-started at the full solution; the
  likelihood-ratio statistic ``lr`` and its p-value under the boundary mixture 1/2 chi2_0 + 1/2 chi2_1.

Everything but the argument checks needs the GPU (there is no CPU path).  Out of scope: profile-likelihood intervals of entries of
W, the simplex over W, entries held at positive values, G = None, more than 8 components or m k above 2048, more than one GPU."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_image, check_layout, check_log_shift, image_dims, narrowed_image

MAX_K = 8          # ESPM_DIAG_MAX_K: components of the model
MAX_F = 2048       # unknowns m k of the dense information matrix (measures.spectral_diagnostics' limit)
MAX_PASS = 64      # the default cap of the passes of a fit
TAU0, TAU_MIN, TAU_MAX, TAU_STEP = 1e-2, 1e-8, 1.0, 10.0
THETA, START = 0.01, 1e-3


def _positive_int(v, name):
    if isinstance(v, bool) or int(v) != v or int(v) < 1:
        raise ValueError(f"{name} must be a positive integer, not {v!r}")
    return int(v)


def _check_entries(entries, m, k, who):
    """(E, 2) int64 of distinct (element, component) pairs inside (m, k)."""
    ent = np.asarray(entries)
    if ent.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if ent.ndim != 2 or ent.shape[1] != 2 or ent.dtype.kind not in "iu":
        raise ValueError(f"{who}: entries must be (E, 2) integer pairs (element, component), not {ent.shape} of {ent.dtype}")
    ent = ent.astype(np.int64)
    if (ent < 0).any() or (ent[:, 0] >= m).any() or (ent[:, 1] >= k).any():
        raise ValueError(f"{who}: entries must index W of shape ({m}, {k})")
    if len({(int(e), int(j)) for e, j in ent}) != len(ent):
        raise ValueError(f"{who}: entries must be distinct")
    return ent


class _Solver:
    """X, G and H, checked on the host and then uploaded ONCE: every ``run`` is a fit over a free set on the resident image."""

    def __init__(self, X, G, H, tol, max_pass, log_shift, layout, device, who):
        check_layout(layout)
        X = check_image(X)
        if G is None:
            raise NotImplementedError(f"{who}: G is required, a dictionary (channels, m) ndarray (without one the problem decouples "
                                      f"per channel: the pixel problem with the roles of the factors swapped)")
        G = np.ascontiguousarray(G, dtype=np.float64)
        H = np.ascontiguousarray(H, dtype=np.float64)
        if G.ndim != 2 or H.ndim != 2 or G.size == 0 or H.size == 0:
            raise ValueError("G must be (channels, m) and H (components, pixels), both non-empty")
        self.n, self.p = image_dims(X.shape, layout)
        self.m, self.k = int(G.shape[1]), int(H.shape[0])
        if G.shape[0] != self.n:
            raise ValueError(f"X has {self.n} channels, G has {G.shape[0]}")
        if H.shape[1] != self.p:
            raise ValueError(f"X has {self.p} pixels, H has {H.shape[1]}")
        if self.k > MAX_K:
            raise NotImplementedError(f"{who}: {self.k} components (the kernel is built for 1..{MAX_K})")
        if self.m * self.k > MAX_F:
            raise NotImplementedError(f"{who}: a dictionary of {self.m} entries x {self.k} components gives an information matrix of "
                                      f"{self.m * self.k} rows (at most {MAX_F})")
        check_log_shift(log_shift)
        if not tol > 0:
            raise ValueError("tol must be positive")
        self.max_pass = _positive_int(max_pass, "max_pass")
        for name, v in (("G", G), ("H", H)):
            if not np.isfinite(v).all() or (v < 0).any():
                raise ValueError(f"{who}: {name} must be finite and not negative")
        self.who, self.layout, self.log_shift, self.tol = who, layout, float(log_shift), float(tol)
        self.G, self.H = G, H
        self.a = np.outer(G.sum(axis=0), H.sum(axis=1))
        self.image, self.Gd = _image.Resident(narrowed_image(X, who), layout, device), None

    def check_start(self, W0):
        if W0 is None:
            return np.ones((self.m, self.k))
        W0 = np.array(W0, dtype=np.float64)
        if W0.shape != (self.m, self.k):
            raise ValueError(f"{self.who}: W0 of shape {W0.shape} for a dictionary of {self.m} entries and {self.k} components")
        if not np.isfinite(W0).all():
            raise ValueError(f"{self.who}: W0 holds values that are not finite")
        return W0

    def check_free(self, free):
        """(F, inert): the free entries the model can see, and those it cannot (a_ej = 0)."""
        if free is None:
            free = np.ones((self.m, self.k), dtype=bool)
        else:
            free = np.asarray(free)
            if free.shape != (self.m, self.k) or free.dtype != bool:
                raise ValueError(f"{self.who}: free must be a boolean array of shape ({self.m}, {self.k})")
        F = free & (self.a > 0)
        return F, free & ~(self.a > 0)

    def upload(self):
        if self.Gd is None:
            import torch

            from espm_amd import _lib, marginals
            self.dev = self.image.upload().dev
            self.Gd, self.Hd, self.ad = self.image.model(self.G, self.H, self.a)
            # N: the marginals' pass under all-ones weights (exact for integers)
            self.N = float(marginals.pixel_maps(self.image.Xd, np.ones((1, self.n)), layout=self.layout)["counts"][0].sum())
            n, p, k = self.n, self.p, self.k
            nt = k * (k + 1) // 2
            with self.image.scope():
                self.out = torch.empty((3 + k + nt) * n, dtype=torch.float64, device=self.dev)   # dev, xsum, ysum, q (n, k), a_tri (n, nt)
                self.nbytes = int(_lib.lib.espm_spectra_ml_pass_scratch(n, p, k))
                self.scratch = torch.empty(self.nbytes // 8, dtype=torch.float64, device=self.dev)
                self.un = torch.zeros(1, dtype=torch.int64, device=self.dev)
                il, jl = np.tril_indices(k)   # row by row: (0,0), (1,0), (1,1), (2,0), ...
                self.il, self.jl = torch.from_numpy(il).to(self.dev), torch.from_numpy(jl).to(self.dev)

    def device_pass(self, Wd):
        """The pass at D = G W: (dev (n,), Q (n, k), A (n, k, k)) on the device; the unmodelled count stays in ``self.un``."""
        import torch

        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        n, k = self.n, self.k
        nt = k * (k + 1) // 2
        Dd = (self.Gd @ Wd).contiguous()
        o = self.out
        _lib.check(_lib.lib.espm_spectra_ml_pass(*self.image.abi(), _ptr(Dd), _ptr(self.Hd), k, self.log_shift, _ptr(o[:n]),
                                                 _ptr(o[n:2 * n]), _ptr(o[2 * n:3 * n]), _ptr(o[3 * n:(3 + k) * n]),
                                                 _ptr(o[(3 + k) * n:]), _ptr(self.un), _ptr(self.scratch), self.nbytes, _stream()))
        tri = o[(3 + k) * n:].view(n, nt)
        A = torch.empty((n, k, k), dtype=torch.float64, device=self.dev)
        A[:, self.il, self.jl] = tri
        A[:, self.jl, self.il] = tri
        return o[:n], o[3 * n:(3 + k) * n].view(n, k), A

    def run(self, W0, F):
        """One fit over the free set F (a host bool (m, k) with an entry at least) from the host start W0: the dict of ``ml_spectra``
        without ``inert``, W and channel_deviance as host arrays."""
        import torch
        self.upload()
        m, k, N = self.m, self.k, self.N
        res = dict(W=np.zeros((m, k)), deviance=0.0, channel_deviance=np.zeros(self.n), gap=0.0, n_pass=0, n_rejected=0, n_fallback=0,
                   converged=True, unmodelled=0)
        if N == 0:
            return res
        W0 = np.where(F, W0, 0.0)
        bad = F & ~(W0 > 0)
        W0[bad] = N / (F.sum() * self.a[bad]) * START
        res["converged"] = False
        with self.image.scope():
            Fd = torch.from_numpy(F).to(self.dev)
            idx = torch.from_numpy(np.flatnonzero(F.ravel())).to(self.dev)
            aF = self.ad[Fd]
            W = torch.from_numpy(W0).to(self.dev)
            tau, dev_acc, trial, e = TAU0, float("inf"), False, None
            kept, pending = None, False
            solved = torch.zeros((), dtype=torch.float64, device=self.dev)   # whether the step before came out of a finite factorisation
            for _ in range(self.max_pass):
                W = W * (N / (aF @ W[Fd]))
                dev_c, Q, A = self.device_pass(W)
                q = self.Gd.T @ Q
                rF = q[Fd] / aF
                # the one read-back of a pass: the deviance, the certificate, the count, and what kind of step led here
                dev, rmax, un, was_trial = (float(v) for v in torch.stack((dev_c.sum(), rF.max(), self.un[0].to(torch.float64), solved)).cpu())
                res["n_pass"] += 1
                if pending:
                    trial = was_trial == 1.0
                    res["n_fallback"] += not trial
                pending = False
                if trial and not dev <= dev_acc:
                    W, trial, tau = e, False, min(tau * TAU_STEP, TAU_MAX)
                    res["n_rejected"] += 1
                    continue
                gap = 2.0 * N * (rmax - 1.0)
                dev_acc = dev
                kept = (W, dev_c.clone())
                res.update(deviance=dev, gap=gap, unmodelled=int(un))
                if gap <= self.tol:
                    res["converged"] = True
                    break
                if trial:
                    tau = max(tau / TAU_STEP, TAU_MIN)
                r = torch.zeros_like(W)
                r[Fd] = rF
                e = W * r
                B = torch.einsum("ce,cf,cij->eifj", self.Gd, self.Gd, A).reshape(m * k, m * k)[idx][:, idx]
                B.diagonal().add_(tau * (aF / W[Fd]))
                L, info = torch.linalg.cholesky_ex(B)
                delta = torch.cholesky_solve((q[Fd] - aF)[:, None], L)[:, 0]
                step = W.clone()
                step[Fd] = torch.maximum(W[Fd] + delta, THETA * W[Fd])
                ok = (info == 0) & torch.isfinite(delta).all()   # a factorisation that is not finite: the EM successor instead
                W, solved, pending = torch.where(ok, step, e), ok.to(torch.float64), True
            if kept is not None:
                res["W"], res["channel_deviance"] = _image.to_host(kept[0]), _image.to_host(kept[1])
        return res


def ml_spectra(X, G, H, W0=None, free=None, tol=1e-3, max_pass=MAX_PASS, log_shift=1e-14, layout="cm", device=None):
    """The Poisson maximum-likelihood W (m, k) >= 0 of D = G W given the dictionary G (n, m) and the abundances H (k, p), over the
    entries of the boolean ``free`` (m, k) (None: all), by the safeguarded Newton rule of tests/spectra_ml_reference.py with its
    optimality certificate as the stop.  Returns dict(

    * ``W`` (m, k) float64: entries outside ``free`` exactly 0, scaled so that sum a W = N (a_ej = (G^T 1)_e (H 1)_j, N: the counts);
    * ``deviance``: 2 sum (x ln(x / y) - x + y) at ``W``, y = max(G W H, log_shift), and ``channel_deviance`` (n,), its terms;
    * ``gap``: the certificate 2 N (max_free (G^T (X / Y) H^T) / a - 1): ``deviance`` is above its minimum over {W >= 0, support in
      ``free``} by at most ``gap`` (convexity) - wherever no entry with counts sits under the floor: ``unmodelled`` counts those, and
      with counts U in them the bound is 2 U + max(gap, 0);
    * ``n_pass``: the passes over the image (the certifying one included), ``n_rejected``: the trials whose deviance rose (the EM
      successor of the last accepted point follows), ``n_fallback``: the factorisations that were not finite (EM step instead);
    * ``converged``: gap <= tol.  At the cap ``W``, ``deviance`` and ``gap`` are those of the last accepted point;
    * ``inert`` (m, k) bool: the free entries with a_ej = 0, which no observation sees; they are held at 0).

    The ML is over W >= 0 with H held: no regulariser (mu), no simplex and no floor of a fit is imposed.  X, ``layout``: as for
    ``presence.ml_unmix`` (uploaded ONCE through ``_image.Resident``); ``W0``: the start (None: 1; an entry that is not > 0 becomes
    N / (|free| a_ej) * 1e-3).  1..8 components and m k <= 2048 (NotImplementedError beyond, and for ``G=None``); ValueError for
    shapes that do not match, values that are not finite, G or H negative, ``tol`` or ``log_shift`` not positive and a ``free``
    without an entry the model sees - all before anything is uploaded.  One GPU per call."""
    sv = _Solver(X, G, H, tol, max_pass, log_shift, layout, device, "ml_spectra")
    W0 = sv.check_start(W0)
    F, inert = sv.check_free(free)
    if not F.any():
        raise ValueError("ml_spectra: no free entry of W that the model can see")
    return dict(sv.run(W0, F), inert=inert)


def presence(X, G, H, W0=None, free=None, entries=None, tol=1e-3, max_pass=MAX_PASS, log_shift=1e-14, layout="cm", device=None):
    """Is element e present in phase j?  The likelihood ratio between the ML W over ``free`` (``ml_spectra``) and the ML W with
    entry (e, j) held at zero, warm-started at the full solution - on the resident image, one fit per tested entry.  Returns dict(

    * ``W_ml`` (m, k), ``deviance_ml``: the full fit;
    * ``lr`` (m, k) = max(deviance without (e, j) - deviance_ml, 0); NaN for the entries not tested and for an entry whose removal
      leaves no free entry; each of the two deviances is within ``gap`` <= tol of its minimum (``ml_spectra``'s caveat applies);
    * ``pvalue`` (m, k) = ``espm_amd.presence.pvalue(lr)``: the tail of 1/2 chi2_0 + 1/2 chi2_1, the law of the statistic when the
      true entry sits ON the boundary; asymptotic, and NaN where ``lr`` is;
    * ``entries`` (E, 2): the tested (element, component) pairs - ``entries`` as given, by default every free entry the model sees;
    * ``converged``, ``gap``, ``n_pass`` (1 + E,): the full fit, then the fit without each tested entry, in the order of ``entries``
      (an entry outside the free set, or the only free one, is no fit: converged, 0, 0);
    * ``inert``, ``unmodelled``: of the full fit).

    A nested fit whose first pass already certifies costs that one pass.  Arguments and refusals as for ``ml_spectra``; ValueError
    also for ``entries`` that are no distinct (E, 2) index pairs into W."""
    from espm_amd.presence import pvalue
    sv = _Solver(X, G, H, tol, max_pass, log_shift, layout, device, "presence")
    W0 = sv.check_start(W0)
    F, inert = sv.check_free(free)
    if not F.any():
        raise ValueError("presence: no free entry of W that the model can see")
    ent = np.argwhere(F) if entries is None else _check_entries(entries, sv.m, sv.k, "presence")
    full = sv.run(W0, F)
    lr = np.full((sv.m, sv.k), np.nan)
    rows = [full]
    for e, j in ent:
        sub = F.copy()
        sub[e, j] = False
        if not F[e, j] or not sub.any():
            rows.append(dict(converged=True, gap=0.0, n_pass=0))
            continue
        red = sv.run(full["W"], sub)
        lr[e, j] = max(red["deviance"] - full["deviance"], 0.0)
        rows.append(red)
    pv = np.full(lr.shape, np.nan)
    ok = ~np.isnan(lr)
    pv[ok] = pvalue(lr[ok])
    return dict(W_ml=full["W"], deviance_ml=full["deviance"], lr=lr, pvalue=pv, entries=ent,
                converged=np.array([r["converged"] for r in rows], dtype=bool), gap=np.array([r["gap"] for r in rows], dtype=np.float64),
                n_pass=np.array([r["n_pass"] for r in rows], dtype=np.int64), inert=inert, unmodelled=full["unmodelled"])
