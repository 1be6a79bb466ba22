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
  likelihood-ratio statistic ``lr`` and its p-value under the boundary mixture 1/2 chi2_0 + 1/2 chi2_1;
* ``ml_spectra_pinned``: the best fit with ONE entry held at a value t >= 0 - a point of that entry's profile - by the pinned rule
  (tests/spectra_ml_pinned_reference.py: no scale onto the ray, a certificate of its own, the slope of the profile);
* ``intervals``: how much of element e could be in phase j - the profile-likelihood interval of every tested entry, an upper limit
  where the entry sits at the boundary.  The 2 E ends (two per tested entry) are 2 E pinned problems of ONE image: they run in
  LOCKSTEP on espm_spectra_ml_pass_batch, which serves B models in one pass launch and skips the ones that have retired, with the
  dense algebra, the decisions and the bracketed root finder as batched, masked tensor updates and one small read-back per pass.

Everything but the argument checks needs the GPU (there is no CPU path).  Out of scope: intervals of normalised concentrations
W_ej / sum_e W_ej, the simplex over W, the uncertainty of H, ``mu`` and the floors of a fit, entries that the caller fixes at
positive values (``fixed_W``), G = None, more than 8 components or m k above 2048, more than one GPU."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_image, check_layout, check_log_shift, image_dims, narrowed_image

MAX_K = 8          # ESPM_DIAG_MAX_K: components of the model
MAX_F = 2048       # unknowns m k of the dense information matrix (measures.spectral_diagnostics' limit)
MAX_PASS = 64      # the default cap of the passes of a fit
TAU0, TAU_MIN, TAU_MAX, TAU_STEP = 1e-2, 1e-8, 1.0, 10.0
THETA, START = 0.01, 1e-3
H_FLOOR = 1e-30    # the pinned rule's floor of a step, H_FLOOR N / a: it has no scale onto the ray to keep an entry from underflowing
MAX_PASS_PINNED = 128   # the default cap of the passes of one pinned fit, and of the full fit of ``intervals``
# ``intervals(batch=None)`` takes the largest batch within two budgets - design choices, not measurements:
BATCH_SCRATCH_BYTES = 1 << 30   # the scratch of espm_spectra_ml_pass_batch (the partial sums of every model's pass)
BATCH_INFO_BYTES = 256 << 20    # the stacked information matrices, B (m k)^2 doubles


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

    # ---- the pinned rule, many problems in lockstep (tests/spectra_ml_pinned_reference.py) -----------------------------------------------
    def batch_buffers(self, B):
        """The outputs, the counters and the scratch of espm_spectra_ml_pass_batch for B models (kept for the next call at the same B)."""
        import torch

        from espm_amd import _lib
        if getattr(self, "_batch", (0, None))[0] != B:
            n, k = self.n, self.k
            nt = k * (k + 1) // 2
            nbytes = int(_lib.lib.espm_spectra_ml_pass_batch_scratch(n, self.p, k, B))
            z = dict(dtype=torch.float64, device=self.dev)
            self._batch = None   # (the buffers of another B go before these come)
            self._batch = (B, dict(dev=torch.zeros((B, n), **z), ysum=torch.zeros((B, n), **z), q=torch.zeros((B, n, k), **z),
                                   tri=torch.zeros((B, n, nt), **z), un=torch.zeros(B, dtype=torch.int64, device=self.dev),
                                   scratch=torch.empty(nbytes // 8, **z), nbytes=nbytes))
        return self._batch[1]

    def device_pass_batch(self, Wd, active, buf):
        """The pass at D_b = G W_b for the models with ``active`` (B,) uint8 set: (dev (B, n), Q (B, n, k), A (B, n, k, k)) on the
        device, the unmodelled counts in ``buf["un"]``.  The rows of a model that is not active are those of its last active pass."""
        import torch

        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        B, k = Wd.shape[0], self.k
        Dd = (self.Gd @ Wd).contiguous()
        _lib.check(_lib.lib.espm_spectra_ml_pass_batch(*self.image.abi(), _ptr(Dd), _ptr(self.Hd), k, B, _ptr(active), self.log_shift,
                                                       _ptr(buf["dev"]), _ptr(buf["ysum"]), _ptr(buf["q"]), _ptr(buf["tri"]), _ptr(buf["un"]),
                                                       _ptr(buf["scratch"]), buf["nbytes"], _stream()))
        A = torch.empty((B, self.n, k, k), dtype=torch.float64, device=self.dev)
        A[:, :, self.il, self.jl] = buf["tri"]
        A[:, :, self.jl, self.il] = buf["tri"]
        return buf["dev"], buf["q"], A

    def lockstep(self, F, pins, t, W0, root=None):
        """B pinned problems of the free set F (host bool (m, k)) at once, every pass ONE batched device pass and ONE small read-back:
        problem b holds entry ``pins[b]`` (an entry of F) at ``t[b]`` and fits the others from ``W0[b]`` (host, (B, m, k), positive on
        F).  Without ``root`` a problem is that one fit.  With ``root`` = dict(up (B,) bool, w_ml, w0 (B,), dev_ml, q_level, lr_tol,
        max_eval, lift (m, k)) it is one END of a profile interval: the bracketed root finder of the reference moves t from fit to
        fit, each fit warm-started at the one before.  A problem retires on its own (its flag in ``active`` goes to 0: the device
        pass skips it); nothing is re-packed.  Returns host arrays: W (B, m, k), deviance, gap, slope, channel_deviance (B, n) of the
        last accepted point, n_pass, n_rejected, n_fallback, converged (of the last fit), unmodelled, n_lockstep (the batched passes
        this call took: its loop's own count), and with ``root`` also end (NaN where the end was not found), found, n_eval.

        ONE SHAPE FOR ALL: every lockstep pass forms the whole (B, m k, m k) stack of information matrices and factors B systems of
        |F| unknowns, also for the problems that have retired or that only evaluate this pass - those solve the identity, and their
        results are never selected.  The device pass skips a retired problem; the dense algebra does not, so on a small image, where
        that algebra is the cost of a pass, the retired problems of a batch are paid for until its last problem ends.  (Re-packing
        the batch would save that at the price of new shapes, and new roundings, from pass to pass.)"""
        import torch
        self.upload()
        m, k, n, N = self.m, self.k, self.n, self.N
        B, mk = len(pins), self.m * self.k
        inf = float("inf")
        with self.image.scope():
            f64, i64 = dict(dtype=torch.float64, device=self.dev), dict(dtype=torch.int64, device=self.dev)
            buf = self.batch_buffers(B)
            idx = torch.from_numpy(np.flatnonzero(F.ravel())).to(self.dev)
            flat = pins[:, 0] * k + pins[:, 1]
            Mh = np.repeat(F.ravel()[None], B, axis=0)
            Mh[np.arange(B), flat] = False
            M = torch.from_numpy(Mh).to(self.dev)
            MF = M[:, idx]
            pin, ar = torch.from_numpy(flat).to(self.dev), torch.arange(B, device=self.dev)
            a = self.ad.reshape(mk)
            a1 = torch.where(a > 0, a, torch.ones_like(a))   # (outside F, where a may be 0, nothing of this is used)
            floor = H_FLOOR * N / a1
            tt = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(self.dev)
            W = torch.from_numpy(np.ascontiguousarray(W0, dtype=np.float64).reshape(B, mk)).to(self.dev)
            W[ar, pin] = tt
            alive = torch.ones(B, dtype=torch.bool, device=self.dev)
            tau, dev_acc = torch.full((B,), TAU0, **f64), torch.full((B,), inf, **f64)
            trial, conv = torch.zeros_like(alive), torch.zeros_like(alive)
            e = W.clone()
            fit_pass, n_pass, n_rej, n_fb, kept_un = (torch.zeros(B, **i64) for _ in range(5))
            kept_W, kept_devc = W.clone(), torch.zeros((B, n), **f64)
            kept_dev, kept_gap, kept_slope = (torch.zeros(B, **f64) for _ in range(3))
            eye = torch.eye(idx.numel(), **f64)
            if root is not None:
                up = torch.from_numpy(np.ascontiguousarray(root["up"], dtype=bool)).to(self.dev)
                w_ml, w0 = (torch.from_numpy(np.ascontiguousarray(root[key], dtype=np.float64)).to(self.dev) for key in ("w_ml", "w0"))
                lift = torch.from_numpy(np.ascontiguousarray(root["lift"], dtype=np.float64).reshape(mk)).to(self.dev)
                lo, hi = torch.where(up, w_ml, torch.zeros_like(w_ml)), torch.where(up, torch.full_like(w_ml, inf), w_ml)
                n_eval, end, found = torch.zeros(B, **i64), torch.full((B,), float("nan"), **f64), torch.zeros_like(alive)
            un_max = n_lockstep = 0
            while True:
                n_lockstep += 1
                active = alive.to(torch.uint8)
                dev_c, Q, A = self.device_pass_batch(W.view(B, m, k), active, buf)
                q = (self.Gd.T @ Q).reshape(B, mk)
                dv = dev_c.sum(dim=1)
                n_pass += alive
                fit_pass += alive
                rej = alive & trial & ~(dv <= dev_acc)
                acc = alive & ~rej
                r = torch.where(M, q / a1, torch.zeros_like(q))
                rmax = torch.where(M, r, torch.full_like(r, -inf)).max(dim=1).values   # (M empty: -inf, and a gap of 0)
                gap = 2.0 * torch.where(M, (a - q) * W, torch.zeros_like(q)).sum(dim=1) + 2.0 * N * torch.clamp(rmax - 1.0, min=0.0)
                slope = 2.0 * (a[pin] - q[ar, pin])
                stop = acc & (gap <= self.tol)
                go = acc & ~stop
                # ACCEPT: the point is the one reported
                dev_acc = torch.where(acc, dv, dev_acc)
                kept_W, kept_devc = torch.where(acc[:, None], W, kept_W), torch.where(acc[:, None], dev_c, kept_devc)
                kept_dev, kept_gap, kept_slope = torch.where(acc, dv, kept_dev), torch.where(acc, gap, kept_gap), torch.where(acc, slope, kept_slope)
                kept_un = torch.where(acc, buf["un"], kept_un)
                conv = torch.where(alive, stop, conv)
                tau = torch.where(go & trial, torch.clamp(tau / TAU_STEP, min=TAU_MIN), tau)
                # ... its EM successor and the blended Newton step over M (a problem that does not step solves the identity)
                e_new = W * r
                e_new[ar, pin] = tt
                WF, aF = W[:, idx], a[idx]
                step_at = MF & go[:, None]
                Bm = torch.einsum("ce,cf,bcij->beifj", self.Gd, self.Gd, A).reshape(B, mk, mk)[:, idx][:, :, idx]
                Bm = torch.where(step_at[:, :, None] & step_at[:, None, :], Bm, torch.zeros_like(Bm))
                Bm.diagonal(dim1=1, dim2=2).add_(torch.where(step_at, tau[:, None] * (aF / WF), torch.ones_like(WF)))
                Bm = torch.where(go[:, None, None], Bm, eye)
                rhs = torch.where(step_at, (q - a)[:, idx], torch.zeros_like(WF))
                L, info = torch.linalg.cholesky_ex(Bm)
                delta = torch.cholesky_solve(rhs[:, :, None], L)[:, :, 0]
                ok = (info == 0) & torch.isfinite(delta).all(dim=1)
                step = W.clone()
                step[:, idx] = torch.where(MF, torch.maximum(torch.maximum(WF + delta, THETA * WF), floor[idx]), WF)
                n_fb += go & ~ok
                n_rej += rej
                # REJECT: the EM successor of the last accepted point
                W = torch.where(go[:, None], torch.where(ok[:, None], step, e_new), torch.where(rej[:, None], e, W))
                e = torch.where(go[:, None], e_new, e)
                trial = torch.where(go, ok, trial & ~rej)
                tau = torch.where(rej, torch.clamp(tau * TAU_STEP, max=TAU_MAX), tau)
                capped = alive & ~stop & (fit_pass >= self.max_pass)
                if root is None:
                    alive = alive & ~stop & ~capped
                else:
                    # a fit that certified is one evaluation of phi: the end, or the bracket and the next t (the reference's _advance)
                    phi = dv - root["dev_ml"] - root["q_level"]
                    n_eval += stop
                    first_low = ~up & (n_eval == 1)
                    fin = stop & ((phi.abs() <= root["lr_tol"]) | (first_low & (phi <= 0)))
                    end, found = torch.where(fin, tt, end), found | fin
                    more = stop & ~fin & (n_eval < root["max_eval"])
                    inner = torch.where(up, phi < 0, phi > 0)
                    lo2, hi2 = torch.where(inner, tt, lo), torch.where(inner, hi, tt)
                    tn = tt - phi / slope
                    open_ = torch.isinf(hi2)
                    good = torch.isfinite(tn) & (tn > lo2) & (tn < hi2)
                    tn = torch.where(open_, torch.minimum(tn, w_ml + 8.0 * (tt - w_ml)), tn)
                    mid = torch.where(open_, w_ml + 2.0 * (tt - w_ml), 0.5 * (lo2 + hi2))
                    tn = torch.where(good, tn, mid)
                    tn = torch.where(first_low, torch.maximum(w_ml - w0, 0.5 * w_ml), tn)
                    tt, lo, hi = torch.where(more, tn, tt), torch.where(more, lo2, lo), torch.where(more, hi2, hi)
                    Wr = torch.where(M, torch.maximum(W, lift), W)
                    Wr[ar, pin] = tt
                    W = torch.where(more[:, None], Wr, W)
                    tau, dev_acc = torch.where(more, torch.full_like(tau, TAU0), tau), torch.where(more, torch.full_like(tau, inf), dev_acc)
                    trial, fit_pass = trial & ~more, torch.where(more, torch.zeros_like(fit_pass), fit_pass)
                    alive = alive & ~capped & ~(stop & ~more)
                # the one read-back of a lockstep pass: how many problems go on, and the counters (the most entries under the floor)
                live, un = (int(v) for v in torch.stack((alive.sum(), torch.where(active.bool(), buf["un"], torch.zeros_like(kept_un)).max())).cpu())
                un_max = max(un_max, un)
                if live == 0:
                    break
            h = _image.to_host
            out = dict(W=h(kept_W).reshape(B, m, k), deviance=h(kept_dev), gap=h(kept_gap), slope=h(kept_slope), channel_deviance=h(kept_devc),
                       n_pass=h(n_pass), n_rejected=h(n_rej), n_fallback=h(n_fb), converged=h(conv), unmodelled=h(kept_un), unmodelled_max=un_max, n_lockstep=n_lockstep)
            if root is not None:
                out.update(end=h(end), found=h(found), n_eval=h(n_eval))
        return out


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


def _check_pin(pin, F, who):
    try:
        e, j = (int(v) for v in pin)
        ok = len(pin) == 2 and all(int(v) == v and not isinstance(v, bool) for v in pin)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (0 <= e < F.shape[0] and 0 <= j < F.shape[1]) or not F[e, j]:
        raise ValueError(f"{who}: pin must be an (element, component) pair inside the free set the model sees, not {pin!r}")
    return e, j


def ml_spectra_pinned(X, G, H, pin, t, W0=None, free=None, tol=1e-3, max_pass=MAX_PASS_PINNED, log_shift=1e-14, layout="cm", device=None):
    """ONE POINT OF THE PROFILE: the Poisson maximum-likelihood W >= 0 over ``free`` with the entry ``pin`` = (element, component)
    HELD AT ``t`` >= 0, by the pinned rule of tests/spectra_ml_pinned_reference.py - ``ml_spectra``'s rule without the scale onto
    the ray, with a certificate of its own.  Returns ``ml_spectra``'s dict, where

    * ``W`` has ``W[pin] == t`` bit for bit and is NOT scaled onto the ray;
    * ``gap`` = 2 sum_M (a - q) W + 2 N max(max_M q / a - 1, 0) over M = the free set less the pin: ``deviance`` is above its minimum
      over {W >= 0, W[pin] = t} by at most ``gap`` (convexity, and sum_M a W* <= N at the pinned optimum; ``ml_spectra``'s caveat for
      counted entries under the floor applies);

    plus ``slope`` = 2 (a_pin - q_pin): the derivative of the profile deviance in t at this point (by the envelope theorem, exact at
    the pinned optimum).  A free set of the pin alone is one evaluating pass with gap 0.  Arguments and refusals as for
    ``ml_spectra``; ValueError also for a ``pin`` outside the free set the model sees and for a ``t`` that is negative or not finite
    - before anything is uploaded.  ``W0``: the start of the other entries (None: 1; an entry that is not > 0 becomes
    N / (|M| a_ej) * 1e-3)."""
    sv = _Solver(X, G, H, tol, max_pass, log_shift, layout, device, "ml_spectra_pinned")
    W0 = sv.check_start(W0)
    F, inert = sv.check_free(free)
    pin = _check_pin(pin, F, "ml_spectra_pinned")
    if isinstance(t, bool) or not np.isfinite(float(t)) or float(t) < 0:
        raise ValueError(f"ml_spectra_pinned: t must be finite and not negative, not {t!r}")
    sv.upload()
    M = F.copy()
    M[pin] = False
    W0 = np.where(M, W0, 0.0)
    if sv.N == 0:
        W0[:] = 0.0
    elif M.any():
        bad = M & ~(W0 > 0)
        W0[bad] = sv.N / (M.sum() * sv.a[bad]) * START
    out = sv.lockstep(F, np.array([pin], dtype=np.int64), np.array([float(t)]), W0[None])
    return dict(W=out["W"][0], deviance=float(out["deviance"][0]), channel_deviance=out["channel_deviance"][0], gap=float(out["gap"][0]),
                slope=float(out["slope"][0]), n_pass=int(out["n_pass"][0]), n_rejected=int(out["n_rejected"][0]),
                n_fallback=int(out["n_fallback"][0]), converged=bool(out["converged"][0]), unmodelled=int(out["unmodelled"][0]), inert=inert)


def _auto_batch(sv, n_problems):
    """The largest batch within BATCH_SCRATCH_BYTES and BATCH_INFO_BYTES (at least 1, at most the problems there are)."""
    from espm_amd import _lib
    per_model = int(_lib.lib.espm_spectra_ml_pass_batch_scratch(sv.n, sv.p, sv.k, 1))
    return int(max(1, min(n_problems, BATCH_SCRATCH_BYTES // per_model, BATCH_INFO_BYTES // ((sv.m * sv.k) ** 2 * 8))))


def intervals(X, G, H, W0=None, free=None, entries=None, level=0.95, tol=1e-3, lr_tol=1e-2, max_eval=64, max_pass=MAX_PASS_PINNED,
              batch=None, log_shift=1e-14, layout="cm", device=None):
    """How much of element e could be in phase j?  The PROFILE-LIKELIHOOD interval of entries of W with the abundances H held: the
    values t whose best fit with W_ej held at t (``ml_spectra_pinned``) lies within the chi2_1 quantile ``threshold`` =
    2 erfinv(level)^2 of the best fit (``ml_spectra``).  Where the entry sits at the boundary - a trace element - the interval starts
    at exactly 0 and its upper end is an UPPER LIMIT ("< 0.05 at 95 %"); away from it the two ends are an asymmetric error bar
    ("0.8 (0.5 - 1.2)").  ``presence``'s statistic is this profile at the single point t = 0.  The intervals are two-sided: a one-sided
    95 % upper limit is the upper end at ``level=0.90``.  Returns dict(

    * ``W_ml`` (m, k), ``deviance_ml``: the full fit;
    * ``lower``, ``upper`` (m, k): the ends, with |g(t) - deviance_ml - threshold| <= ``lr_tol`` for the certified pinned deviance g
      (each of the two deviances within ``tol`` of its minimum); ``lower`` is EXACTLY 0 where ``W_ml`` is 0 and where
      g(0) - deviance_ml <= threshold (``presence``'s lr <= threshold: the boundary); NaN for the entries not tested, for an entry
      outside the free set, and for an end that was not found;
    * ``level``, ``threshold``, ``entries`` (E, 2): the tested (element, component) pairs - ``entries`` as given, by default every
      free entry the model sees;
    * ``converged`` (bool), ``n_eval``, ``n_pass``, each (E, 2): [:, 0] the lower end, [:, 1] the upper - whether the end was found,
      the pinned fits it took and their passes over the image (an entry outside the free set is no fit: converged, 0, 0);
    * ``n_full_pass``: the passes of the full fit; ``inert``, ``unmodelled``: of the full fit;
    * ``batch``: the problems that ran in lockstep; ``n_lockstep``: the batched device passes (and read-backs) the ends took).

    The full fit is ``ml_spectra``'s; then all 2 E ends advance TOGETHER, ``batch`` problems at a time (None: the largest batch for
    which the scratch of the batched pass stays within BATCH_SCRATCH_BYTES and the stacked information matrices within
    BATCH_INFO_BYTES).  A lockstep pass is one batched G W, one espm_spectra_ml_pass_batch over the resident image for the problems
    still running, batched G^T Q, information matrices and Cholesky in torch fp64 on the device, the accept / reject / stop of
    every problem and the root finder's bracket and next t as masked tensor updates, and ONE small read-back.  Every evaluation is a
    pinned fit warm-started at the one before with the fitted entries lifted to the rule's own start fill.  A pinned fit that does
    not converge within ``max_pass``, or an end that takes more than ``max_eval`` fits, ends as not converged (NaN), without an
    exception.  Two calls with the same arguments give the same bits; another ``batch`` meets the same bound, not the same bits.

    What the interval is NOT: it holds H fixed (its uncertainty is not in it); it is the interval of W_ej itself, not of a normalised
    concentration W_ej / sum_e W_ej; no simplex over W, no ``mu`` and no floor of a fit is imposed; and it is ASYMPTOTIC.  One GPU per
    call.  Arguments and refusals as for ``presence``; ValueError also for ``level`` outside (0, 1), ``lr_tol`` not positive, and
    ``max_eval`` or ``batch`` that are no positive integers - all before anything is uploaded."""
    from espm_amd.presence import threshold
    sv = _Solver(X, G, H, tol, max_pass, log_shift, layout, device, "intervals")
    W0 = sv.check_start(W0)
    F, inert = sv.check_free(free)
    if not F.any():
        raise ValueError("intervals: no free entry of W that the model can see")
    ql = threshold(level)
    if not lr_tol > 0:
        raise ValueError("lr_tol must be positive")
    max_eval = _positive_int(max_eval, "max_eval")
    if batch is not None:
        batch = _positive_int(batch, "batch")
    ent = np.argwhere(F) if entries is None else _check_entries(entries, sv.m, sv.k, "intervals")
    E = len(ent)
    full = sv.run(W0, F)
    W_ml, N = full["W"], sv.N
    lower, upper = np.full((sv.m, sv.k), np.nan), np.full((sv.m, sv.k), np.nan)
    conv, n_eval, n_pass = np.zeros((E, 2), dtype=bool), np.zeros((E, 2), dtype=np.int64), np.zeros((E, 2), dtype=np.int64)
    # the ends that need no fit are settled here; the others are the problems of the lockstep, in the order (entry, side)
    prob = []
    for i, (e, j) in enumerate(ent):
        if not F[e, j]:
            conv[i] = True
        elif full["converged"]:
            if W_ml[e, j] == 0:
                lower[e, j], conv[i, 0] = 0.0, True
            else:
                prob.append((i, 0))
            prob.append((i, 1))
    nF = int(F.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        lift = np.where(F, N / ((nF - 1) * sv.a) * START, 0.0) if nF > 1 else np.zeros(F.shape)
    B = 0 if not prob else (_auto_batch(sv, len(prob)) if batch is None else min(batch, len(prob)))
    n_lockstep = 0
    for at in range(0, len(prob), max(B, 1)):
        part = np.array(prob[at:at + B])
        pins, up = ent[part[:, 0]], part[:, 1] == 1
        w_ml, ae = W_ml[pins[:, 0], pins[:, 1]], sv.a[pins[:, 0], pins[:, 1]]
        w0 = np.sqrt(ql) * np.sqrt(ae * w_ml + ql) / ae
        start = np.repeat(np.where(F, np.maximum(W_ml, lift), 0.0)[None], len(part), axis=0)
        out = sv.lockstep(F, pins, np.where(up, w_ml + w0, 0.0), start,
                          root=dict(up=up, w_ml=w_ml, w0=w0, dev_ml=full["deviance"], q_level=ql, lr_tol=float(lr_tol), max_eval=max_eval,
                                    lift=lift))
        for b, (i, side) in enumerate(part):
            e, j = ent[i]
            conv[i, side], n_eval[i, side], n_pass[i, side] = out["found"][b], out["n_eval"][b], out["n_pass"][b]
            (upper if side else lower)[e, j] = out["end"][b]
        n_lockstep += out["n_lockstep"]
    return dict(W_ml=W_ml, deviance_ml=full["deviance"], lower=lower, upper=upper, level=float(level), threshold=ql, entries=ent,
                converged=conv, n_eval=n_eval, n_pass=n_pass, n_full_pass=full["n_pass"], inert=inert, unmodelled=full["unmodelled"],
                batch=B, n_lockstep=n_lockstep)
