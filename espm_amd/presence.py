"""Presence maps on the device (csrc/mu_pixel_ml.hip): is phase j in this pixel at all?

At EDS doses of a few tens of counts per pixel most abundances of most phases sit at or near zero, where a Cramer-Rao bar around
h ~ 0 (``measures.pixel_diagnostics``' ``H_std``, which ignores active floors) means nothing.  The honest statistic at a boundary is
a likelihood ratio between nested models: the pixel's best Poisson fit with all k spectra against its best fit with spectrum j left
out.  Both are per-pixel maximum-likelihood problems given the spectra D:

* ``ml_unmix``: the ML abundances of every pixel over a set of components, by EM (the entry point espm_pixel_ml; the rule is in
  include/espm_mu.h, "pixel ML") or by a safeguarded Newton step (``method="newton"``: espm_pixel_ml_newton, csrc/mu_pixel_ml_newton.hip,
  "pixel ML, Newton") - every pixel with a stop of its own and an optimality CERTIFICATE: ``gap`` bounds how far the
  pixel's deviance is above the minimum over {h >= 0, support in the set}, wherever no entry with counts sits under the floor;
* ``presence``: the k + 1 nested fits, the likelihood-ratio statistic ``lr`` of every (component, pixel) - certified to within
  ``tol`` on either side - and its asymptotic p-value under the boundary mixture 1/2 chi2_0 + 1/2 chi2_1;
* ``ml_unmix_pinned`` and ``intervals``: how much of component j COULD be in this pixel - the best fit with h_j held at a per-pixel
  value (the entry point espm_pixel_ml_pinned, csrc/mu_pixel_ml_pinned.hip, "pixel ML, pinned"), and the profile-likelihood interval
  a root finder on the device builds from such fits: an upper limit where the abundance sits at the boundary, an asymmetric error
  bar away from it.  ``presence``'s statistic is that profile at the single point 0.

The ML abundances are also what ``H_std`` is formally a bound for, and with a ``simplex_H`` fit their column sums map the per-pixel
dose or thickness that the simplex model cannot express.  ``method="simplex"`` / ``simplex=True`` solve the pixel problem OF that
model instead - sum h = 1, the spectra carry the intensity (espm_pixel_ml_simplex, csrc/mu_pixel_ml_simplex.hip, "pixel ML,
simplex") - so that the tests and the intervals are about phase fractions, with no scale per pixel that the fit did not have.
EM is slow (hundreds of passes, tails of thousands) and cannot fail, and it is the default; the Newton rule reaches the same certified points in tens of passes.  The
kernel runs a bounded number of passes per launch and the loop here reads one integer, the pixels not yet done, between launches.
fp64 throughout, no float atomics: two calls, both layouts, every dtype that holds the counts and every ``chunk`` give the same bits.
Everything but the argument checks needs the GPU (there is no CPU path)."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_image, check_layout, check_log_shift, image_dims, narrowed_image

MAX_K = 8            # ESPM_PML_MAX_K: components of the model
MAX_PASS = 20000     # the default cap of the passes of a pixel
CHUNK = 64           # passes per launch
METHODS = ("em", "newton")   # espm_pixel_ml, espm_pixel_ml_newton: the two rules of the SAME problem, h >= 0 with a free scale
ALL_METHODS = METHODS + ("simplex",)   # ... and espm_pixel_ml_simplex: another problem, the fit under sum h = 1


def _check_method(method):
    if method not in ALL_METHODS:
        raise ValueError(f"method must be one of {ALL_METHODS}, not {method!r}")
    return method


def _positive_int(v, name):
    if isinstance(v, bool) or int(v) != v or int(v) < 1:
        raise ValueError(f"{name} must be a positive integer, not {v!r}")
    return int(v)


def _components(components, k):
    """The sorted component set and its bitmask."""
    if components is None:
        comp = list(range(k))
    else:
        comp = sorted({int(j) for j in components})
        if len(comp) != len(list(components)) or any(isinstance(j, bool) or int(j) != j for j in components):
            raise ValueError(f"components must be distinct integers, not {components!r}")
        if not comp or comp[0] < 0 or comp[-1] >= k:
            raise ValueError(f"components must be a non-empty subset of 0 .. {k - 1}, not {components!r}")
    return comp, sum(1 << j for j in comp)


class _Solver:
    """X and the spectra, checked on the host and then uploaded ONCE (``image``, by the narrowing rule): every ``run`` is a nested
    fit on the resident image.  The component sets, the start and the solver's state are its own."""

    def __init__(self, X, D, tol, max_pass, chunk, log_shift, layout, who, method="em"):
        check_layout(layout)
        self.method = _check_method(method)
        self.simplex = method == "simplex"   # the flag ``run`` and ``run_pinned`` go by: espm_pixel_ml_simplex, sum_M h = 1 - h_pin
        X = check_image(X)
        D = np.ascontiguousarray(D, dtype=np.float64)
        if D.ndim != 2 or D.size == 0:
            raise ValueError("D must be (channels, components), not empty")
        self.n, self.p = image_dims(X.shape, layout)
        self.k = int(D.shape[1])
        if D.shape[0] != self.n:
            raise ValueError(f"X has {self.n} channels, D has {D.shape[0]}")
        if self.k > MAX_K:
            raise NotImplementedError(f"{who}: {self.k} components (the kernels are built for 1..{MAX_K})")
        check_log_shift(log_shift)
        if not tol > 0:
            raise ValueError("tol must be positive")
        self.max_pass, self.chunk = _positive_int(max_pass, "max_pass"), _positive_int(chunk, "chunk")
        if not np.isfinite(D).all() or (D < 0).any():
            raise ValueError(f"{who}: D must be finite and not negative")
        self.who, self.layout, self.log_shift, self.tol = who, layout, float(log_shift), float(tol)
        self.D, self.s = D, np.ascontiguousarray(D.sum(axis=0))
        self.image, self.Dd = _image.Resident(narrowed_image(X, who), layout), None

    def check_start(self, H0):
        if H0 is None:
            return None
        H0 = np.ascontiguousarray(H0, dtype=np.float64)
        if H0.shape != (self.k, self.p):
            raise ValueError(f"{self.who}: H0 of shape {H0.shape} for {self.k} components and {self.p} pixels")
        if not np.isfinite(H0).all():
            raise ValueError(f"{self.who}: H0 holds values that are not finite")
        return H0

    def check_components(self, components):
        comp, mask = _components(components, self.k)
        empty = [j for j in comp if not self.s[j] > 0]
        if empty:
            raise ValueError(f"{self.who}: the spectrum of component {empty[0]} is all zero: leave it out of `components`")
        return comp, mask

    def upload(self):
        if self.Dd is None:
            self.dev = self.image.upload().dev
            self.Dd, = self.image.model(self.D)

    def counts(self):
        """N (p,) on the device: the counts of every pixel (the marginals' pass under all-ones weights: exact for integers)."""
        import torch

        from espm_amd import marginals
        N = marginals.pixel_maps(self.image.Xd, np.ones((1, self.n)), layout=self.layout)["counts"][0]
        return torch.from_numpy(np.ascontiguousarray(N)).to(self.dev)

    def run(self, start, comp, mask):
        """One fit over the component set: dict of DEVICE tensors H (k, p), deviance, gap (p,), n_pass (p,) int32, done (p,) uint8 and the
        ints unmodelled, nonfinite.  ``start``: a device (k, p) float64 tensor (consumed), a checked host array, or None: N / sum_M s
        (under the simplex: 1 / |M|)."""
        import ctypes as C

        import torch

        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        self.upload()
        k, p = self.k, self.p
        with self.image.scope():
            if start is None:
                Hd = torch.zeros((k, p), dtype=torch.float64, device=self.dev)
                Hd[comp] = 1.0 / len(comp) if self.simplex else (self.counts() / float(self.s[comp].sum()))[None, :]
            elif isinstance(start, torch.Tensor):
                Hd = start.contiguous()
            else:
                Hd = torch.from_numpy(start).to(self.dev)
            dv, gp = torch.zeros(p, dtype=torch.float64, device=self.dev), torch.zeros(p, dtype=torch.float64, device=self.dev)
            passes = torch.zeros(p, dtype=torch.int32, device=self.dev)
            done = torch.zeros(p, dtype=torch.uint8, device=self.dev)
            counters = torch.zeros(3, dtype=torch.int64, device=self.dev)
            s_ptr = self.s.ctypes.data_as(C.c_void_p)
            args = (*self.image.abi(), _ptr(self.Dd), s_ptr, k, mask, self.log_shift, self.tol)
            state = (_ptr(Hd), _ptr(dv), _ptr(gp), _ptr(passes), _ptr(done), _ptr(counters))
            if self.method != "em":   # the rule's own scratch (e, dev_acc, tau, trial per pixel): the kernel initialises it
                extra = torch.empty((k + _lib.PMLN_STATE_EXTRA, p), dtype=torch.float64, device=self.dev)
                entry, state = _lib.lib.espm_pixel_ml_newton, state + (_ptr(extra), extra.numel() * extra.element_size())
                if self.simplex:   # nothing pinned: pin = -1, and neither t nor slope
                    entry = _lib.lib.espm_pixel_ml_simplex
                    args, state = (*args[:-2], -1, None, *args[-2:]), (*state[:3], None, *state[3:])
            else:
                entry = _lib.lib.espm_pixel_ml
            issued = 0
            while issued < self.max_pass:   # bounded launches: no launch's duration depends on the slowest pixel of the image
                step = min(self.chunk, self.max_pass - issued)
                _lib.check(entry(*args, step, *state, _stream()))
                issued += step
                if int(counters[_lib.PML_NOT_DONE].item()) == 0:   # the one integer read between the chunks
                    break
            cnt = counters.cpu().numpy()
        return dict(H=Hd, deviance=dv, gap=gp, n_pass=passes, done=done, unmodelled=int(cnt[_lib.PML_UNMODELLED]),
                    nonfinite=int(cnt[_lib.PML_NONFINITE]))

    def check_pin(self, pin, components):
        """(pin, the fitted set, its bitmask): ``components`` None is every component but ``pin``; the set may be empty (k = 1)."""
        if isinstance(pin, bool) or int(pin) != pin or not 0 <= int(pin) < self.k:
            raise ValueError(f"{self.who}: pin must be one of the components 0 .. {self.k - 1}, not {pin!r}")
        pin = int(pin)
        if not self.s[pin] > 0:
            raise ValueError(f"{self.who}: the spectrum of the pinned component {pin} is all zero")
        if components is None:
            components = [j for j in range(self.k) if j != pin]
        if len(list(components)) == 0:
            return pin, [], 0
        comp, mask = self.check_components(components)
        if pin in comp:
            raise ValueError(f"{self.who}: the pinned component {pin} is in `components`: it is held, not fitted")
        return pin, comp, mask

    def run_pinned(self, start, comp, mask, pin, t, done=None, searching=None):
        """One fit over the component set with component ``pin`` held at ``t`` (espm_pixel_ml_pinned; under the simplex
        espm_pixel_ml_simplex, where the set sums to 1 - t and a start of None is 1 / |M|), on the resident image: ``run``'s
        dict plus ``slope`` (p,) and ``searching``.  ``t``: a device (p,) float64 tensor.  ``start`` as for ``run``; a device tensor is
        updated IN PLACE (the next evaluation's warm start).  ``done``: None, or a device (p,) uint8 tensor (consumed) - a pixel
        with done != 0 is not touched, and its deviance, gap, slope and n_pass read 0.  ``searching``: None, or a device integer the
        caller counts its unfinished pixels in: it rides in the same transfer as the one counter read between the launches, comes
        back as an int, and where it is 0 nothing more is launched."""
        import ctypes as C

        import torch

        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        self.upload()
        k, p = self.k, self.p
        with self.image.scope():
            if start is None:
                Hd = torch.zeros((k, p), dtype=torch.float64, device=self.dev)
                if comp:
                    Hd[comp] = 1.0 / len(comp) if self.simplex else (self.counts() / float(self.s[comp].sum()))[None, :]
            elif isinstance(start, torch.Tensor):
                Hd = start
                assert Hd.is_contiguous()
            else:
                Hd = torch.from_numpy(start).to(self.dev)
            dv, gp, sl = (torch.zeros(p, dtype=torch.float64, device=self.dev) for _ in range(3))
            passes = torch.zeros(p, dtype=torch.int32, device=self.dev)
            done = torch.zeros(p, dtype=torch.uint8, device=self.dev) if done is None else done
            counters = torch.zeros(_lib.PML_COUNTERS + 1, dtype=torch.int64, device=self.dev)   # the kernel's three, and `searching`
            if searching is not None:
                counters[_lib.PML_COUNTERS] = searching
            extra = torch.empty((k + _lib.PMLN_STATE_EXTRA, p), dtype=torch.float64, device=self.dev)   # the kernel initialises it
            s_ptr = self.s.ctypes.data_as(C.c_void_p)
            args = (*self.image.abi(), _ptr(self.Dd), s_ptr, k, mask, pin, _ptr(t), self.log_shift, self.tol)
            state = (_ptr(Hd), _ptr(dv), _ptr(gp), _ptr(sl), _ptr(passes), _ptr(done), _ptr(counters), _ptr(extra),
                     extra.numel() * extra.element_size())
            entry = _lib.lib.espm_pixel_ml_simplex if self.simplex else _lib.lib.espm_pixel_ml_pinned
            issued = 0
            while issued < self.max_pass:
                step = min(self.chunk, self.max_pass - issued)
                _lib.check(entry(*args, step, *state, _stream()))
                issued += step
                cnt = counters.cpu().numpy()   # the one read-back between the chunks
                if cnt[_lib.PML_NOT_DONE] == 0:
                    break
            cnt = counters.cpu().numpy()
        return dict(H=Hd, deviance=dv, gap=gp, slope=sl, n_pass=passes, done=done, unmodelled=int(cnt[_lib.PML_UNMODELLED]),
                    nonfinite=int(cnt[_lib.PML_NONFINITE]), searching=int(cnt[_lib.PML_COUNTERS]))


def _result(r):
    """A ``run``'s dict on the host, as ``ml_unmix`` returns it."""
    t = _image.to_host
    return dict(H=t(r["H"]), deviance=t(r["deviance"]), gap=t(r["gap"]), n_pass=t(r["n_pass"]).astype(np.int64),
                converged=t(r["done"]) == 1, unmodelled=r["unmodelled"], nonfinite=r["nonfinite"])


def ml_unmix(X, D, H0=None, components=None, tol=1e-3, max_pass=MAX_PASS, chunk=CHUNK, log_shift=1e-14, layout="cm", method="em"):
    """The Poisson maximum-likelihood abundances of every pixel given the spectra D, over the component set ``components`` (None: all),
    by EM (``method="em"``, the default and the rule that is defined bit for bit) or by the safeguarded Newton step of
    include/espm_mu.h, "pixel ML, Newton" (``method="newton"``: the same certificate and stop, tens of passes where EM takes hundreds
    to thousands), with a per-pixel stop.  Returns dict(

    * ``H`` (k, p) float64: the ML abundances, rows outside the set exactly 0, scaled so that sum_j s_j h_j = N (s: the column sums of
      D, N: the pixel's counts); a pixel without a count has h = 0;
    * ``deviance`` (p,): 2 sum_c (x ln(x / y) - x + y) at ``H``, y = max(D h, log_shift) - ``pixel_diagnostics``' expression;
    * ``gap`` (p,): the certificate 2 N (max_j (D^T (x / y))_j / s_j - 1): ``deviance`` is above its minimum over {h >= 0, support in
      the set} by at most ``gap`` (convexity; it needs no entry with counts under the floor - see ``unmodelled``);
    * ``n_pass`` (p,) int: the steps the pixel took (under "newton": trials, rejected ones included); ``converged`` (p,) bool:
      gap <= tol.  A pixel that is not converged after ``max_pass`` passes reports the deviance and gap of its last pass (under
      "newton": of its last accepted point) and the h the next pass would start from;
    * ``unmodelled``: the entries with counts whose model is below ``log_shift`` (over the converged pixels); ``nonfinite``: the pixels
      stopped at a value that is not finite (they are not converged)).

    X: the image as measured, (channels, pixels) for ``layout="cm"`` or (pixels, channels) for "pm", a host array or a device tensor,
    checked and uploaded ONCE by the narrowing rule (``_image_args.narrowed_image``).  D (n, k): 1 .. 8 components
    (NotImplementedError beyond), finite, not negative; a component of the set needs a spectrum that is not all zero.  ``H0`` (k, p): the start; an entry of the set that is not > 0 is
    replaced by N / (|set| s_j) * 1e-3; None: N / sum_set s.  ``chunk``: the passes per launch (the results do not depend on it).
    ValueError for shapes that do not match, ``tol`` or ``log_shift`` not positive, X, D or H0 not finite and a ``method`` that does
    not exist - before anything is uploaded.

    ``method="simplex"``: the CONSTRAINED ML of a ``simplex_H`` model - abundances are phase fractions, sum_set h = 1 in every pixel,
    and the spectra carry the intensity - by the rule of include/espm_mu.h, "pixel ML, simplex" (the Newton step with the multiplier
    of the sum, an EM successor with a per-pixel root).  The same dict: the columns of ``H`` sum to 1 over the set (to within k ulps)
    and are NOT scaled onto sum_j s_j h_j = N; ``gap`` is the Frank-Wolfe certificate 2 (sum_j g_j h_j - min_j g_j), g = s - D^T (x / y):
    ``deviance`` is above its minimum over the simplex by at most that.  A pixel without a count puts h = 1 on the component of the
    least s_j.  ``H0``: lifted to at least 1e-3 / |set| and scaled to sum 1; None: 1 / |set|."""
    sv = _Solver(X, D, tol, max_pass, chunk, log_shift, layout, "ml_unmix", method)
    start = sv.check_start(H0)
    comp, mask = sv.check_components(components)
    return _result(sv.run(start, comp, mask))


def _empty_model_deviance(X, layout, log_shift):
    """The deviance of the model with no component at all, by the floor rule: y = log_shift in every channel; 0 for a pixel without a
    count.  Host numpy, one pass."""
    try:
        import torch
        if isinstance(X, torch.Tensor):
            X = X.cpu().numpy()
    except ImportError:
        pass
    x = np.asarray(X, dtype=np.float64)
    x = x if layout == "cm" else x.T
    t = log_shift - x
    pos = x > 0
    t[pos] += x[pos] * np.log(x[pos] * (1.0 / log_shift))
    return np.where(x.sum(axis=0) == 0, 0.0, 2.0 * t.sum(axis=0))


def pvalue(lr):
    """1/2 erfc(sqrt(lr / 2)): the tail of the boundary mixture 1/2 chi2_0 + 1/2 chi2_1 at ``lr``; 1 where lr == 0."""
    from scipy.special import erfc
    lr = np.asarray(lr, dtype=np.float64)
    return np.where(lr > 0, 0.5 * erfc(np.sqrt(lr / 2.0)), 1.0)


def presence(X, D, H0=None, tol=1e-3, max_pass=MAX_PASS, chunk=CHUNK, log_shift=1e-14, layout="cm", method="em"):
    """Is component j present in pixel q?  The likelihood ratio between the pixel's ML fit with all k spectra and its ML fit with
    spectrum j left out (``ml_unmix`` k + 1 times on the resident image, each reduced fit started at the full solution with row j
    zeroed).  ``method``: as for ``ml_unmix``, the one method for all k + 1 fits.  Returns dict(

    * ``H_ml`` (k, p), ``deviance_ml`` (p,): the full fit;
    * ``lr`` (k, p) = max(deviance without j - deviance_ml, 0): each of the two deviances is within ``gap`` <= tol of its minimum, so
      every entry is certified to within ``tol`` on either side;
    * ``pvalue`` (k, p) = 1/2 erfc(sqrt(lr / 2)), 1 where lr = 0: the tail of 1/2 chi2_0 + 1/2 chi2_1, the law of the statistic when
      the true abundance sits ON the boundary h_j = 0.  It is ASYMPTOTIC: at a few tens of counts per pixel, and where other abundances
      sit on their boundaries too, it is a guide and no calibration (``sampling`` draws the replicates a calibration needs);
    * ``converged``, ``gap``, ``n_pass`` (k + 1, p): row 0 the full fit, row 1 + j the fit without j;
    * ``unmodelled``, ``nonfinite``: of the full fit).

    With one component the reduced model is empty: its deviance is the floor rule's, y = log_shift in every channel, formed on the
    host without a launch.  Arguments and refusals as for ``ml_unmix``; every component needs a spectrum that is not all zero.

    ``method="simplex"``: the test a ``simplex_H`` fit calls for - the full fit under sum h = 1 against the fit over the other
    components, which sum to 1 again (each started at the full solution with row j zeroed and rescaled): no free scale per pixel on
    either side.  ``lr`` is exactly 0 wherever the full fit has h_j = 0 (there the full solution is a point of the reduced problem).
    One component: ValueError, nothing is fitted under the simplex."""
    sv = _Solver(X, D, tol, max_pass, chunk, log_shift, layout, "presence", method)
    start = sv.check_start(H0)
    comp, mask = sv.check_components(None)
    k, p = sv.k, sv.p
    if sv.simplex and k == 1:
        raise ValueError("presence: one component under the simplex (h = 1 in every pixel: nothing is fitted, nothing to test)")
    held = sv.image.host if k == 1 else None
    full = sv.run(start, comp, mask)
    without = np.empty((k, p))
    rows = [_result(full)]
    for j in range(k):
        if k == 1:
            without[j] = _empty_model_deviance(held, layout, sv.log_shift)
            rows.append(dict(converged=np.ones(p, dtype=bool), gap=np.zeros(p), n_pass=np.zeros(p, dtype=np.int64)))
            continue
        Hs = full["H"].clone()
        Hs[j] = 0.0
        rest = [i for i in comp if i != j]
        red = _result(sv.run(Hs, rest, mask & ~(1 << j)))
        without[j] = red["deviance"]
        rows.append(red)
    lr = np.maximum(without - rows[0]["deviance"][None, :], 0.0)
    if sv.simplex:   # h_j == 0 in the full fit: its point is a point of the reduced problem, whose minimum is therefore not above it
        lr = np.where(rows[0]["H"] == 0, 0.0, lr)   # (the rule's start lifts such zeros: the reduced fit may certify within tol above)
    return dict(H_ml=rows[0]["H"], deviance_ml=rows[0]["deviance"], lr=lr, pvalue=pvalue(lr),
                converged=np.stack([r["converged"] for r in rows]), gap=np.stack([r["gap"] for r in rows]),
                n_pass=np.stack([r["n_pass"] for r in rows]), unmodelled=rows[0]["unmodelled"], nonfinite=rows[0]["nonfinite"])


# ---- how much of phase j could be in this pixel: profile-likelihood intervals of the abundances ----------------------------------------
def _check_pinned_value(t, p, who, simplex=False):
    t = np.asarray(t, dtype=np.float64)
    if t.ndim == 0:
        t = np.full(p, float(t))
    if t.shape != (p,):
        raise ValueError(f"{who}: t must be a scalar or of shape ({p},), not {t.shape}")
    if not np.isfinite(t).all() or (t < 0).any():
        raise ValueError(f"{who}: t must be finite and not negative")
    if simplex and (t > 1).any():
        raise ValueError(f"{who}: t must not exceed 1 under the simplex (the others sum to 1 - t)")
    return np.ascontiguousarray(t)


def ml_unmix_pinned(X, D, pin, t, H0=None, components=None, tol=1e-3, max_pass=MAX_PASS, chunk=CHUNK, log_shift=1e-14, layout="cm",
                    simplex=False):
    """``ml_unmix`` with the abundance of component ``pin`` HELD at ``t`` (a scalar, or (p,): a value per pixel) while the components
    of ``components`` (None: all but ``pin``; may be empty) are fitted: one point of the profile likelihood of h_pin, by the rule of
    include/espm_mu.h, "pixel ML, pinned" (the Newton step of ``method="newton"`` without its scale onto the ray, which a pinned term
    leaves without a closed form).  Returns ``ml_unmix``'s dict - ``H`` with row ``pin`` equal to ``t`` bit for bit, and NOT scaled
    onto sum_j s_j h_j = N - plus ``slope`` (p,) = 2 (s_pin - (D^T (x / y))_pin), the derivative of the profile deviance in t
    (exact at the inner optimum, approximate at a certified point).  ``gap`` is this rule's own certificate,
    2 sum_M (s_j - q_j) h_j + 2 N max(max_M q_j / s_j - 1, 0): ``deviance`` is above its minimum over the set, at this t, by at most that.
    Arguments and refusals as for ``ml_unmix``; ValueError also for a ``pin`` that is no component or is in ``components``, a pinned
    spectrum that is all zero and a ``t`` that is negative, not finite or of another shape - all before anything is uploaded.

    ``simplex=True``: the same point of the profile under sum h = 1 (include/espm_mu.h, "pixel ML, simplex": espm_pixel_ml_simplex) -
    the fitted abundances sum to 1 - t, ``gap`` is the Frank-Wolfe certificate 2 (sum_M g_j h_j - (1 - t) min_M g_j), g = s - q, and
    ``slope`` = 2 (g_pin - sum_M g_j h_j / (1 - t)) carries the multiplier of the sum.  A ``t`` above 1 is a ValueError too."""
    sv = _Solver(X, D, tol, max_pass, chunk, log_shift, layout, "ml_unmix_pinned", "simplex" if simplex else "newton")
    start = sv.check_start(H0)
    pin, comp, mask = sv.check_pin(pin, components)
    t = _check_pinned_value(t, sv.p, sv.who, sv.simplex)
    sv.upload()
    td, = sv.image.model(t)
    r = sv.run_pinned(start, comp, mask, pin, td)
    return dict(_result(r), slope=_image.to_host(r["slope"]))


def threshold(level):
    """2 erfinv(level)^2: the chi2_1 quantile of a two-sided interval at ``level`` (0.95: 3.8415)."""
    from scipy.special import erfinv
    if isinstance(level, bool) or not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must lie strictly between 0 and 1, not {level!r}")
    return float(2.0 * erfinv(float(level)) ** 2)


def intervals(X, D, H0=None, level=0.95, components=None, tol=1e-3, lr_tol=1e-2, max_eval=64, max_pass=MAX_PASS, chunk=CHUNK,
              log_shift=1e-14, layout="cm", simplex=False):
    """How much of component j could be in pixel q?  The PROFILE-LIKELIHOOD interval of every abundance: the values t whose best fit
    with h_j held at t (``ml_unmix_pinned``) lies within the chi2_1 quantile ``threshold`` = 2 erfinv(level)^2 of the pixel's best fit
    (``ml_unmix(method="newton")``).  Where the abundance sits at the boundary the interval starts at 0 and its upper end is an UPPER
    LIMIT, the detection limit of the map; away from it the two ends are an asymmetric error bar.  ``presence``'s statistic is this
    profile at the single point t = 0.  The intervals are two-sided: a one-sided 95 % upper limit is the upper end at ``level=0.90``.
    Returns dict(

    * ``H_ml`` (k, p), ``deviance_ml`` (p,): the full fit;
    * ``lower``, ``upper`` (k, p): the ends, with |g(t) - deviance_ml - threshold| <= ``lr_tol`` for the certified pinned deviance g
      (each of the two deviances within ``tol`` of its minimum); ``lower`` is EXACTLY 0 where ``H_ml`` is 0 and where
      g(0) - deviance_ml <= threshold (``presence``'s lr <= threshold: the boundary); NaN in the rows that were not requested and
      for the pixels that did not finish; a pixel without a count has lower = 0 and upper = threshold / (2 s_j);
    * ``level``, ``threshold``;
    * ``converged`` (k, 2, p) bool, ``n_eval`` (k, 2, p): the pinned fits an end took, ``n_pass`` (k, 2, p): their passes in all
      ([:, 0] the lower end, [:, 1] the upper);
    * ``unmodelled``, ``nonfinite``: of the full fit).

    The root finder runs on the device in fp64, elementwise over the pixels, every pixel with a bracket of its own: the upper end
    starts at h_ml + sqrt(threshold) sqrt(s_j h_ml + threshold) / s_j and the open bracket grows geometrically; the next point is the
    Newton step on the convex profile with ``ml_unmix_pinned``'s ``slope`` where it falls inside the bracket and the midpoint where it
    does not.  Every evaluation is one pinned fit of the pixels still searching, warm-started at the evaluation before (its fitted
    abundances lifted to at least N / ((k - 1) s_i) * 1e-3, the fill of a start that is not positive); finished
    pixels are retired through the kernel's ``done``, and between launches the counters are read back and nothing else.  At most
    ``max_eval`` evaluations per end.

    What the interval is NOT: it holds the spectra D fixed, imposes no regulariser and no simplex, and is asymptotic (``sampling``
    draws the replicates a calibration of its coverage needs).  ``components``: the rows to compute (None: all); the fits are always
    over all k components, each of which needs a spectrum that is not all zero.  Other arguments and refusals as for ``ml_unmix``;
    ValueError also for ``level`` outside (0, 1), ``lr_tol`` not positive and ``max_eval`` below 1 - before anything is uploaded.

    ``simplex=True``: the interval of a phase FRACTION, for spectra of a ``simplex_H`` fit (they carry the intensity): the full fit is
    ``ml_unmix(method="simplex")``, every evaluation a pinned fit under sum h = 1 (``ml_unmix_pinned(simplex=True)``), and the same
    root finder runs with its bracket capped at 1 - every candidate t is min(t, 1), a point at t = 1 that is still inside the level
    finishes with ``upper`` EXACTLY 1, and ``H_ml`` = 1 gives ``upper`` = 1 without an evaluation - so that
    0 <= lower <= H_ml <= upper <= 1.  The warm starts are lifted to 1e-3 (1 - t) / (k - 1) and rescaled onto 1 - t by the rule's own
    start.  A pixel without a count has no closed form here: its profile is linear in t and one Newton step lands on the end (or the
    cap).  Still fixed spectra, no regulariser, asymptotic, one component at a time."""
    import torch
    q = threshold(level)
    if not lr_tol > 0:
        raise ValueError("lr_tol must be positive")
    max_eval = _positive_int(max_eval, "max_eval")
    sv = _Solver(X, D, tol, max_pass, chunk, log_shift, layout, "intervals", "simplex" if simplex else "newton")
    start = sv.check_start(H0)
    every, mask = sv.check_components(None)
    k, p = sv.k, sv.p
    rows = _components(components, k)[0]
    full = sv.run(start, every, mask)
    with sv.image.scope():
        dev = sv.dev
        H_ml, dev_ml, ok = full["H"], full["deviance"], full["done"] == 1
        nan = float("nan")
        lower, upper = (torch.full((k, p), nan, dtype=torch.float64, device=dev) for _ in range(2))
        conv = torch.zeros((k, 2, p), dtype=torch.bool, device=dev)
        n_eval, n_pass = (torch.zeros((k, 2, p), dtype=torch.int64, device=dev) for _ in range(2))
        # what a warm start is lifted to: the kernel's own fill N / (|M| s_i) * 1e-3 of a start that is not positive
        lift = None if k == 1 or sv.simplex else (sv.counts()[None, :] / ((k - 1) * torch.from_numpy(sv.s).to(dev))[:, None]) * 1e-3
        for j in rows:
            rest = [i for i in every if i != j]
            rmask = mask & ~(1 << j)
            h_ml = H_ml[j]
            w0 = (q ** 0.5) * torch.sqrt(float(sv.s[j]) * h_ml + q) / float(sv.s[j])
            for side in (0, 1):
                up = side == 1
                out = torch.full((p,), nan, dtype=torch.float64, device=dev)
                active = ok.clone()
                if up:
                    lo, hi, t = h_ml.clone(), torch.full_like(h_ml, float("inf")), h_ml + w0
                    if sv.simplex:   # the cap: no fraction above 1; a pixel that is all j has its upper end there
                        t = torch.clamp(t, max=1.0)
                        one = active & (h_ml >= 1)
                        out = torch.where(one, torch.ones_like(out), out)
                        conv[j, side] |= one
                        active &= ~one
                else:
                    lo, hi, t = torch.zeros_like(h_ml), h_ml.clone(), torch.zeros_like(h_ml)
                    zero = active & (h_ml == 0)
                    out = torch.where(zero, torch.zeros_like(out), out)
                    conv[j, side] |= zero
                    active &= ~zero
                Hc = H_ml.clone()
                for ev in range(max_eval):
                    if rest and lift is not None:   # (an abundance the evaluation before drove to 1e-13 may have to come back: from
                        # there it grows slowly; under the simplex the rule's own start lifts and rescales)
                        Hc[rest] = torch.maximum(Hc[rest], lift[rest])
                    r = sv.run_pinned(Hc, rest, rmask, j, t.contiguous(), done=(~active).to(torch.uint8), searching=active.sum())
                    if r["searching"] == 0:   # (that launch found every pixel retired: its workgroups returned at once)
                        break
                    fitted = active & (r["done"] == 1)
                    phi = r["deviance"] - dev_ml - q
                    fin = fitted & (phi.abs() <= lr_tol)
                    if not up and ev == 0:
                        fin |= fitted & (phi <= 0)   # the boundary: the interval reaches 0
                    if up and sv.simplex:
                        fin |= fitted & (t == 1) & (phi <= 0)   # the cap: the interval reaches 1
                    out = torch.where(fin, t, out)
                    conv[j, side] |= fin
                    n_eval[j, side] += active
                    n_pass[j, side] += torch.where(active, r["n_pass"].to(torch.int64), torch.zeros_like(n_pass[j, side]))
                    go = fitted & ~fin
                    inner = (phi < 0) if up else (phi > 0)   # the evaluated point replaces the lower end of the bracket
                    lo, hi = torch.where(go & inner, t, lo), torch.where(go & ~inner, t, hi)
                    tn = t - phi / r["slope"]
                    open_ = torch.isinf(hi)
                    good = torch.isfinite(tn) & (tn > lo) & (tn < hi)
                    tn = torch.where(open_, torch.minimum(tn, h_ml + 8.0 * (t - h_ml)), tn)
                    mid = torch.where(open_, h_ml + 2.0 * (t - h_ml), 0.5 * (lo + hi))
                    nxt = torch.where(good, tn, mid)
                    if not up and ev == 0:   # (the slope at t = 0 belongs to the floor where nothing else is fitted)
                        nxt = torch.maximum(h_ml - w0, 0.5 * h_ml)
                    if up and sv.simplex:
                        nxt = torch.clamp(nxt, max=1.0)
                    t = torch.where(go, nxt, t)
                    active = go
                (upper if up else lower)[j] = out
        host = _image.to_host
        res = _result(full)
        return dict(H_ml=res["H"], deviance_ml=res["deviance"], lower=host(lower), upper=host(upper), level=float(level), threshold=q,
                    converged=host(conv), n_eval=host(n_eval), n_pass=host(n_pass), unmodelled=res["unmodelled"], nonfinite=res["nonfinite"])
