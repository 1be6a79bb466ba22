"""Channel ML on the device (csrc/mu_channel_ml.hip): free spectra given the abundances, line tests and confidence bands.

Without a dictionary (``SmoothNMF(G=None)``, the reference's default) the spectra ARE ``W_`` (channels x phases), and with the
abundances H held the maximum-likelihood problem decouples per channel: channel c is ONE pixel problem of ``espm_amd.presence`` with
the roles of the factors swapped - its observations are the p pixels of row c of X, its design is H^T, its column sums
s_j = sum_p h_jp are the same for every channel and its count total is N_c = sum_p x_cp.  The rules are the pixel rules line for
line (tests/pixel_ml_newton_reference.py: the free-scale rule; tests/pixel_ml_pinned_reference.py: the pinned rule and the root
finder), run on (X^T, H^T); tests/channel_ml_reference.py does exactly that and is the definition.

On the device a fit is a LOCKSTEP of two entry points over the resident image: espm_spectra_ml_pass_batch evaluates the stacked
models d (B, n, k) - per channel the deviance, q and the observed information, reduced over the pixels - and espm_channel_ml_step
applies the rule's between-walk part to all B n problems at once, one thread each: certificate, accept / reject, the blended
root-free Cholesky step, the clamps, the scale onto the ray, and the next point written into d.  The loop enqueues ``chunk``
(pass, step) pairs and then reads back one small vector, the live problems per model; a model with none left is skipped by the pass
at workgroup entry.  No torch arithmetic runs inside the loop.

* ``ml_channels``: the ML spectra D (n, k) >= 0 over a component set, with the certificate of every channel;
* ``presence``: the full fit, then the k fits without component j as ONE batch of k models (the pinned rule at t = 0), the
  likelihood ratio ``lr`` (n, k) and its p-value under the boundary mixture 1/2 chi2_0 + 1/2 chi2_1 - "is this line of phase j real?";
* ``line_presence``: the same test for a whole window of channels - given H the channels are independent, so the ratios add;
* ``ml_channels_pinned``: the best fit with d_cj held at t_c: one point of every channel's profile;
* ``intervals``: the profile-likelihood band of every entry of D - "how much could be under this peak at most?" - all 2 |components|
  ends of all channels as one batch of pinned models, the bracketed root finder of ``presence.intervals`` between the evaluations.

Everything but the argument checks needs the GPU (there is no CPU path).  NOT covered: ``simplex_W``, ``mu`` and the floors of a fit
(the ML is over D >= 0 alone); the uncertainty of H (it is held); more than 8 components; more than one GPU per call; and a
channel's own ``unmodelled`` count - the pass counts the entries with counts under the ``log_shift`` floor per MODEL, over all of its
channels."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_image, check_layout, check_log_shift, image_dims, narrowed_image

MAX_K = 8          # ESPM_DIAG_MAX_K: components of the model
MAX_PASS = 128     # the default cap of the passes of one fit
CHUNK = 4          # (pass, step) pairs between two read-backs
START = 1e-3       # the rule's fill of a start that is not positive: N / (|M| s_j) * START


def _positive_int(v, name):
    if isinstance(v, bool) or int(v) != v or int(v) < 1:
        raise ValueError(f"{name} must be a positive integer, not {v!r}")
    return int(v)


class _Solver:
    """X and H, checked on the host and then uploaded ONCE: every ``fit`` is a lockstep of B models on the resident image."""

    def __init__(self, X, H, tol, max_pass, chunk, log_shift, layout, device, who):
        check_layout(layout)
        X = check_image(X)
        H = np.ascontiguousarray(H, dtype=np.float64)
        if H.ndim != 2 or H.size == 0:
            raise ValueError("H must be (components, pixels), not empty")
        self.n, self.p = image_dims(X.shape, layout)
        self.k = int(H.shape[0])
        if H.shape[1] != self.p:
            raise ValueError(f"X has {self.p} pixels, H has {H.shape[1]}")
        if self.k > MAX_K:
            raise NotImplementedError(f"{who}: {self.k} components (the kernels are built for 1..{MAX_K})")
        check_log_shift(log_shift)
        if not tol > 0:
            raise ValueError("tol must be positive")
        self.max_pass, self.chunk = _positive_int(max_pass, "max_pass"), _positive_int(chunk, "chunk")
        if not np.isfinite(H).all() or (H < 0).any():
            raise ValueError(f"{who}: H must be finite and not negative")
        self.who, self.layout, self.log_shift, self.tol = who, layout, float(log_shift), float(tol)
        self.H, self.s = H, np.ascontiguousarray(H.sum(axis=1))
        self.image, self.Hd, self.N = _image.Resident(narrowed_image(X, who), layout, device), None, None
        self._batch = (0, None)

    def check_start(self, D0):
        if D0 is None:
            return None
        D0 = np.ascontiguousarray(D0, dtype=np.float64)
        if D0.shape != (self.n, self.k):
            raise ValueError(f"{self.who}: D0 of shape {D0.shape} for {self.n} channels and {self.k} components")
        if not np.isfinite(D0).all():
            raise ValueError(f"{self.who}: D0 holds values that are not finite")
        return D0

    def check_components(self, components):
        from espm_amd.presence import _components
        comp, mask = _components(components, self.k)
        empty = [j for j in comp if not self.s[j] > 0]
        if empty:
            raise ValueError(f"{self.who}: the abundance map of component {empty[0]} is all zero: leave it out of `components`")
        return comp, mask

    def check_pin(self, pin, components):
        """(pin, the fitted set, the mask of the set AND the pin): ``components`` None is every component but ``pin``; may be empty."""
        if isinstance(pin, bool) or int(pin) != pin or not 0 <= int(pin) < self.k:
            raise ValueError(f"{self.who}: pin must be one of the components 0 .. {self.k - 1}, not {pin!r}")
        pin = int(pin)
        if not self.s[pin] > 0:
            raise ValueError(f"{self.who}: the abundance map of the pinned component {pin} is all zero")
        if components is None:
            components = [j for j in range(self.k) if j != pin]
        comp, mask = ([], 0) if len(list(components)) == 0 else self.check_components(components)
        if pin in comp:
            raise ValueError(f"{self.who}: the pinned component {pin} is in `components`: it is held, not fitted")
        return pin, comp, mask | (1 << pin)

    # ---- the device ------------------------------------------------------------------------------------------------------------------
    def upload(self):
        if self.Hd is None:
            self.dev = self.image.upload().dev
            self.Hd, = self.image.model(self.H)

    def evaluate(self, Dd):
        """One espm_spectra_ml_pass at Dd (n, k) on the device: (xsum (n,), dev (n,)), device tensors of this call's own."""
        import torch

        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        n, p, k = self.n, self.p, self.k
        nt = k * (k + 1) // 2
        with self.image.scope():
            z = dict(dtype=torch.float64, device=self.dev)
            dev, xsum, ysum, q, tri = (torch.zeros(sz, **z) for sz in (n, n, n, n * k, n * nt))
            un = torch.zeros(1, dtype=torch.int64, device=self.dev)
            nbytes = int(_lib.lib.espm_spectra_ml_pass_scratch(n, p, k))
            scratch = torch.empty(nbytes // 8, **z)
            _lib.check(_lib.lib.espm_spectra_ml_pass(*self.image.abi(), _ptr(Dd), _ptr(self.Hd), k, self.log_shift, _ptr(dev), _ptr(xsum),
                                                     _ptr(ysum), _ptr(q), _ptr(tri), _ptr(un), _ptr(scratch), nbytes, _stream()))
        return xsum, dev

    def counts(self):
        """N (n,) on the device: the counts of every channel (the pass's own sum: exact for integers), kept."""
        import torch
        if self.N is None:
            with self.image.scope():
                self.N, _ = self.evaluate(torch.ones((self.n, self.k), dtype=torch.float64, device=self.dev))
        return self.N

    def default_start(self, comp):
        """N_c / sum_M s_j on the fitted set, 0 elsewhere: (n, k) on the device."""
        import torch
        with self.image.scope():
            d = torch.zeros((self.n, self.k), dtype=torch.float64, device=self.dev)
            if comp:
                d[:, comp] = (self.counts() / float(self.s[comp].sum()))[:, None]
        return d

    def buffers(self, B):
        """The sums of the batched pass, the state and the outputs of the step for B models (kept for the next fit at the same B)."""
        import torch

        from espm_amd import _lib
        if self._batch[0] != B:
            n, k = self.n, self.k
            nt = k * (k + 1) // 2
            nbytes = int(_lib.lib.espm_spectra_ml_pass_batch_scratch(n, self.p, k, B))
            z = dict(dtype=torch.float64, device=self.dev)
            self._batch = (0, None)   # (the buffers of another B go before these come)
            self._batch = (B, dict(dev_in=torch.zeros((B, n), **z), ysum=torch.zeros((B, n), **z), q=torch.zeros((B, n, k), **z),
                                   tri=torch.zeros((B, n, nt), **z), un=torch.zeros(B, dtype=torch.int64, device=self.dev),
                                   scratch=torch.empty(nbytes // 8, **z), nbytes=nbytes,
                                   state=torch.zeros((B, 2 * k + _lib.CML_STATE_EXTRA, n), **z),
                                   dev=torch.zeros((B, n), **z), gap=torch.zeros((B, n), **z), slope=torch.zeros((B, n), **z),
                                   passes=torch.zeros((B, n), dtype=torch.int32, device=self.dev),
                                   active=torch.zeros(B, dtype=torch.uint8, device=self.dev),
                                   live=torch.zeros(B, dtype=torch.int64, device=self.dev)))
        return self._batch[1]

    def fit(self, d, pins, mask, t=None, done=None):
        """The lockstep of B = len(pins) models: model b fits ``mask`` by the free-scale rule (pins[b] == -1) or holds component
        pins[b] of ``mask`` at ``t[b]`` and fits the rest.  ``d``: a device (B, n, k) float64 tensor, contiguous - the starts, updated
        IN PLACE (a problem that is done keeps its final point there).  ``t``: a device (B, n) tensor (pinned models).  ``done``:
        None, or a device (B, n) uint8 tensor (updated in place): a problem with done != 0 is not touched.  Returns a dict of device
        tensors of the LAST ACCEPTED points - D (B, n, k), deviance, gap, slope (B, n), n_pass (B, n) int32, done (B, n) uint8,
        unmodelled (B,) - that stay valid until the next fit at the same B, and the ints ``started`` (the problems that entered) and
        ``n_lockstep`` (the (pass, step) pairs enqueued)."""
        import ctypes as C

        import torch

        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        self.upload()
        n, k, B = self.n, self.k, len(pins)
        with self.image.scope():
            buf = self.buffers(B)
            xsum = self.counts()
            if done is None:
                done = torch.zeros((B, n), dtype=torch.uint8, device=self.dev)
            assert d.is_contiguous() and d.shape == (B, n, k) and done.is_contiguous()
            pin_h = np.ascontiguousarray(pins, dtype=np.int32)
            state_bytes = buf["state"].numel() * buf["state"].element_size()
            lib = _lib.lib

            def step(start):
                _lib.check(lib.espm_channel_ml_step(n, k, B, start, _ptr(buf["dev_in"]), _ptr(buf["q"]), _ptr(buf["tri"]), _ptr(xsum),
                                                    self.s.ctypes.data_as(C.c_void_p), mask, pin_h.ctypes.data_as(C.c_void_p),
                                                    None if t is None else _ptr(t), self.tol, _ptr(d), _ptr(buf["state"]), state_bytes,
                                                    _ptr(buf["dev"]), _ptr(buf["gap"]), _ptr(buf["slope"]), _ptr(buf["passes"]), _ptr(done),
                                                    _ptr(buf["active"]), _ptr(buf["live"]), _stream()))

            image = self.image.abi()
            step(1)
            started = int(buf["live"].sum().item())
            issued, live = 0, started
            while live and issued < self.max_pass:
                for _ in range(min(self.chunk, self.max_pass - issued)):
                    _lib.check(lib.espm_spectra_ml_pass_batch(*image, _ptr(d), _ptr(self.Hd), k, B, _ptr(buf["active"]), self.log_shift,
                                                              _ptr(buf["dev_in"]), _ptr(buf["ysum"]), _ptr(buf["q"]), _ptr(buf["tri"]),
                                                              _ptr(buf["un"]), _ptr(buf["scratch"]), buf["nbytes"], _stream()))
                    step(0)
                    issued += 1
                live = int(buf["live"].cpu().sum())   # the one read-back between the chunks: the live problems of every model
            D = buf["state"][:, :k, :].permute(0, 2, 1)
        return dict(D=D, deviance=buf["dev"], gap=buf["gap"], slope=buf["slope"], n_pass=buf["passes"], done=done, unmodelled=buf["un"],
                    started=started, n_lockstep=issued)


def _host(r, b=0):
    """Model b of a ``fit``'s dict on the host, as ``ml_channels`` returns it."""
    h = _image.to_host
    done = h(r["done"][b])
    return dict(D=np.ascontiguousarray(h(r["D"][b])), deviance=h(r["deviance"][b]), gap=h(r["gap"][b]),
                n_pass=h(r["n_pass"][b]).astype(np.int64), converged=done == 1, unmodelled=int(r["unmodelled"][b].item()),
                nonfinite=int((done == 2).sum()))


def _full_fit(sv, D0, comp, mask):
    """The free-scale fit over ``comp`` from the checked host start D0 (None: the default): (the fit's dict, deviance_start)."""
    sv.upload()
    dev0 = None
    with sv.image.scope():
        if D0 is None:
            d = sv.default_start(comp)
        else:
            d, = sv.image.model(D0)
            sv.N, dev0 = sv.evaluate(d)
            d = d.clone()
    return sv.fit(d[None].contiguous(), [-1], mask), dev0


def ml_channels(X, H, D0=None, components=None, tol=1e-3, max_pass=MAX_PASS, chunk=CHUNK, log_shift=1e-14, layout="cm", device=None):
    """The Poisson maximum-likelihood spectra D (n, k) >= 0 of X ~ D H given the abundances H (k, p), over the components of
    ``components`` (None: all), every channel a problem of its own, by the free-scale Newton rule of
    tests/pixel_ml_newton_reference.py on (X^T, H^T) with its optimality certificate as the stop.  Returns dict(

    * ``D`` (n, k) float64: columns outside ``components`` exactly 0; row c scaled so that sum_j s_j d_cj = N_c (s_j = sum_p h_jp);
      a channel without a count has the row of zeros;
    * ``deviance`` (n,): 2 sum_p (x ln(x / y) - x + y) of every channel at ``D``, y = max(D H, log_shift);
    * ``deviance_start`` (n,): the same at ``D0`` as given (None without a ``D0``) - ``deviance_start - deviance`` is, per channel,
      what the spectra ``D0`` lose against free spectra;
    * ``gap`` (n,): the certificate 2 N_c (max_M q_j / s_j - 1), q = (X / Y) H^T: ``deviance`` is above its minimum over
      {d_c >= 0, support in ``components``} by at most ``gap`` (convexity), wherever no entry with counts sits under the floor;
    * ``n_pass`` (n,): the passes a channel took (the certifying one not counted, as in ``presence.ml_unmix``); ``converged`` (n,):
      gap <= tol within ``max_pass``; a channel still running at the cap holds its last ACCEPTED point, deviance and gap;
    * ``N`` (n,): the counts of every channel; ``unmodelled``: the entries with counts under the floor, over all channels, at the
      model's last pass; ``nonfinite``: the channels stopped at a value that is not finite).

    The loop enqueues ``chunk`` x (batched pass, step) launches and then reads back the live counts; ``chunk`` changes no bit of
    the result.  X, ``layout``: as for ``presence.ml_unmix`` (uploaded ONCE through ``_image.Resident``); ``D0``: the start (None:
    N_c / sum_M s_j; an entry that is not > 0 becomes N_c / (|M| s_j) * 1e-3).  1..8 components (NotImplementedError beyond);
    ValueError for shapes that do not match, values that are not finite, a negative H, ``tol`` or ``log_shift`` not positive,
    ``max_pass`` or ``chunk`` that are no positive integers and a component of the set whose abundance map is all zero - all before
    anything is uploaded.  One GPU per call."""
    sv = _Solver(X, H, tol, max_pass, chunk, log_shift, layout, device, "ml_channels")
    D0 = sv.check_start(D0)
    comp, mask = sv.check_components(components)
    r, dev0 = _full_fit(sv, D0, comp, mask)
    return dict(_host(r), deviance_start=None if dev0 is None else _image.to_host(dev0), N=_image.to_host(sv.counts()))


def pvalue(lr):
    """1/2 erfc(sqrt(lr / 2)), 1 where lr == 0: ``espm_amd.presence.pvalue``."""
    from espm_amd.presence import pvalue as pv
    return pv(lr)


def presence(X, H, D0=None, tol=1e-3, max_pass=MAX_PASS, chunk=CHUNK, log_shift=1e-14, layout="cm", device=None):
    """Is component j present in channel c - is this line of phase j real?  The likelihood ratio between the channel's ML fit with
    all k abundance maps (``ml_channels``) and its ML fit WITHOUT component j.  The k reduced fits run as ONE batch of k models in
    lockstep - model j holds d_cj at 0 by the pinned rule and fits the others, warm-started at the full solution with column j
    zeroed.  Returns dict(

    * ``D_ml`` (n, k), ``deviance_ml`` (n,): the full fit;
    * ``lr`` (n, k) = max(deviance without j - deviance_ml, 0): each of the two deviances is within ``gap`` <= tol of its minimum;
      EXACTLY 0 where ``D_ml[c, j] == 0`` (there the full solution is a point of the reduced problem);
    * ``pvalue`` (n, k) = 1/2 erfc(sqrt(lr / 2)), 1 where lr == 0: the tail of 1/2 chi2_0 + 1/2 chi2_1, the law of the statistic when
      the true d_cj sits ON the boundary; asymptotic in the counts of the channel;
    * ``converged``, ``gap``, ``n_pass`` (k + 1, n): row 0 the full fit, row 1 + j the fit without j;
    * ``deviance_start`` (as ``ml_channels``), ``N``, ``unmodelled``, ``nonfinite``: of the full fit).

    At least two components (ValueError: with one the reduced model is empty), each with an abundance map that is not all zero.
    Other arguments and refusals as for ``ml_channels``."""
    sv = _Solver(X, H, tol, max_pass, chunk, log_shift, layout, device, "presence")
    D0 = sv.check_start(D0)
    comp, mask = sv.check_components(None)
    k = sv.k
    if k < 2:
        raise ValueError("presence: one component (without it the model is empty: nothing to fit, nothing to test)")
    r, dev0 = _full_fit(sv, D0, comp, mask)
    full = _host(r)
    import torch
    with sv.image.scope():
        d = r["D"][0].contiguous()[None].repeat(k, 1, 1)
        for j in range(k):
            d[j, :, j] = 0.0
        t = torch.zeros((k, sv.n), dtype=torch.float64, device=sv.dev)
        red = sv.fit(d.contiguous(), list(range(k)), mask, t=t)
        rows = [full] + [_host(red, j) for j in range(k)]
    without = np.stack([row["deviance"] for row in rows[1:]], axis=1)
    lr = np.maximum(without - full["deviance"][:, None], 0.0)
    lr = np.where(full["D"] == 0, 0.0, lr)   # (the rule's start lifts such zeros: the reduced fit may certify within tol above)
    return dict(D_ml=full["D"], deviance_ml=full["deviance"], lr=lr, pvalue=pvalue(lr),
                converged=np.stack([row["converged"] for row in rows]), gap=np.stack([row["gap"] for row in rows]),
                n_pass=np.stack([row["n_pass"] for row in rows]), deviance_start=None if dev0 is None else _image.to_host(dev0),
                N=_image.to_host(sv.counts()), unmodelled=full["unmodelled"], nonfinite=full["nonfinite"])


def line_presence(lr, windows):
    """Is component j present ANYWHERE in a window of channels - is the line real?  ``lr`` (n, k): ``presence``'s statistic;
    ``windows``: half-open ranges (lo, hi) of channel indices, as for ``marginals.window_weights`` (they may overlap).  Given H the
    channel problems are independent, so the likelihood ratio of "component j has nothing in the whole window" is the sum of the
    channels' ratios.  Returns dict(

    * ``lr`` (windows, k) = sum_{c in window} lr[c, j];
    * ``pvalue`` (windows, k): under the null every channel's statistic is 1/2 chi2_0 + 1/2 chi2_1, so the sum over w channels is
      chi2_i with probability C(w, i) 2^-w: P = sum_{i=1..w} C(w, i) 2^-w P(chi2_i >= lr), and 1 where lr == 0.  For w = 1 it is
      the single channel's p-value.  Asymptotic, as that one is;
    * ``width`` (windows,): the channels w of every window).

    Host only (scipy.special.gammaincc).  ValueError for an ``lr`` that is not 2-D, holds negative values or values that are not
    finite, and for windows that are no ranges inside 0 .. n."""
    from scipy.special import comb, erfc, gammaincc, gammaln

    from espm_amd.marginals import window_weights
    lr = np.asarray(lr, dtype=np.float64)
    if lr.ndim != 2 or lr.size == 0:
        raise ValueError(f"line_presence: lr must be (channels, components), not {lr.shape}")
    if not np.isfinite(lr).all() or (lr < 0).any():
        raise ValueError("line_presence: lr must be finite and not negative")
    U = window_weights(lr.shape[0], windows)
    total = U @ lr
    width = U.sum(axis=1).astype(np.int64)
    pv = np.ones_like(total)
    for g, w in enumerate(width):
        i = np.arange(1, w + 1, dtype=np.float64)
        # C(w, i) 2^-w: exact products while the binomials are finite, through the logarithms beyond
        weight = comb(w, i) * 2.0 ** -float(w) if w <= 512 else np.exp(gammaln(w + 1.0) - gammaln(i + 1.0) - gammaln(w - i + 1.0) - w * np.log(2.0))
        tail = gammaincc(0.5 * i[:, None], 0.5 * total[g][None, :])   # P(chi2_i >= lr)
        tail[0] = erfc(np.sqrt(total[g] / 2.0))                       # (i = 1 as ``pvalue`` writes it: one channel gives its bits)
        pv[g] = np.where(total[g] > 0, weight @ tail, 1.0)
    return dict(lr=total, pvalue=pv, width=width)


def _pinned_value(t, n, who):
    t = np.asarray(t, dtype=np.float64)
    if t.ndim == 0:
        t = np.full(n, float(t))
    if t.shape != (n,):
        raise ValueError(f"{who}: t must be a scalar or of shape ({n},), not {t.shape}")
    return np.ascontiguousarray(t)


def ml_channels_pinned(X, H, pin, t, D0=None, components=None, tol=1e-3, max_pass=MAX_PASS, chunk=CHUNK, log_shift=1e-14, layout="cm",
                       device=None):
    """``ml_channels`` with the spectrum of component ``pin`` HELD at ``t`` (a scalar, or (n,): a value per channel) while the
    components of ``components`` (None: all but ``pin``; may be empty) are fitted: one point of the profile likelihood of d_c,pin,
    by the pinned rule of tests/pixel_ml_pinned_reference.py on (X^T, H^T) - the Newton rule without its scale onto the ray.
    Returns ``ml_channels``'s dict - ``D`` with column ``pin`` equal to ``t`` bit for bit, NOT scaled onto the ray, and ``gap`` =
    2 sum_M (s_j - q_j) d_cj + 2 N_c max(max_M q_j / s_j - 1, 0), this rule's own certificate - plus ``slope`` (n,) =
    2 (s_pin - q_pin), the derivative of the profile deviance in t (exact at the inner optimum).  A ``t`` that is negative or not
    finite stops that channel at once: not converged, counted in ``nonfinite``.  ``deviance_start`` is None.  Arguments and refusals
    as for ``ml_channels``; ValueError also for a ``pin`` that is no component or is in ``components``, a pinned abundance map that is
    all zero and a ``t`` of another shape - before anything is uploaded."""
    sv = _Solver(X, H, tol, max_pass, chunk, log_shift, layout, device, "ml_channels_pinned")
    D0 = sv.check_start(D0)
    pin, comp, mask = sv.check_pin(pin, components)
    t = _pinned_value(t, sv.n, sv.who)
    sv.upload()
    with sv.image.scope():
        d = sv.default_start(comp) if D0 is None else sv.image.model(D0)[0].clone()
        td, = sv.image.model(t)
        r = sv.fit(d[None].contiguous(), [pin], mask, t=td[None].contiguous())
    return dict(_host(r), slope=_image.to_host(r["slope"][0]), deviance_start=None, N=_image.to_host(sv.counts()))


def intervals(X, H, D0=None, level=0.95, components=None, tol=1e-3, lr_tol=1e-2, max_eval=64, max_pass=MAX_PASS, chunk=CHUNK,
              log_shift=1e-14, layout="cm", device=None):
    """How much of component j could be in channel c - how much could be under this peak at most?  The PROFILE-LIKELIHOOD band of
    the spectra with the abundances held: the values t whose best fit with d_cj held at t (``ml_channels_pinned``) lies within the
    chi2_1 quantile ``threshold`` = 2 erfinv(level)^2 of the channel's best fit (``ml_channels``).  Where d_cj sits at the boundary -
    most channels of a phase spectrum - the band starts at exactly 0 and its upper end is an UPPER LIMIT; on a peak the two ends are
    an asymmetric error bar.  ``presence``'s statistic is this profile at the single point t = 0.  Two-sided: a one-sided 95 %
    upper limit is the upper end at ``level=0.90``.  Returns dict(

    * ``D_ml`` (n, k), ``deviance_ml`` (n,): the full fit;
    * ``lower``, ``upper`` (n, k): the ends, with |g(t) - deviance_ml - threshold| <= ``lr_tol`` for the certified pinned deviance g;
      ``lower`` is EXACTLY 0 where ``D_ml`` is 0 and where g(0) - deviance_ml <= threshold; NaN in the columns not asked for and
      for the channels that did not finish;
    * ``level``, ``threshold``;
    * ``converged`` (k, 2, n) bool, ``n_eval`` (k, 2, n): the pinned fits an end took, ``n_pass`` (k, 2, n): their passes in all
      ([:, 0] the lower end, [:, 1] the upper);
    * ``deviance_start``, ``N``, ``unmodelled``, ``nonfinite``: of the full fit).

    All 2 |components| ends of all channels run as ONE batch of pinned models.  Every evaluation is a pinned fit of the channels
    still searching, warm-started at the evaluation before (its fitted entries lifted to at least N_c / ((k - 1) s_i) * 1e-3, the
    fill of a start that is not positive); between two evaluations the bracket and the next t of every (end, channel) are updated
    elementwise on the device - the rule of tests/pixel_ml_pinned_reference.py (``intervals``, ``_advance``): the upper end starts at
    d + sqrt(q) sqrt(s_j d + q) / s_j and its open bracket grows geometrically, the lower end at 0 and then max(d - w0, d / 2); the
    next point is the Newton step on the convex profile where it falls inside the bracket, else the midpoint.  At most ``max_eval``
    evaluations per end.

    What the band is NOT: it holds H fixed (its uncertainty is not in it), imposes no ``simplex_W``, ``mu`` or floor of a fit, and is
    ASYMPTOTIC in the counts of a channel.  ``components``: the columns to compute (None: all); the fits are always over all k
    components, each of which needs an abundance map that is not all zero.  Other arguments and refusals as for ``ml_channels``;
    ValueError also for ``level`` outside (0, 1), ``lr_tol`` not positive and ``max_eval`` below 1 - before anything is uploaded."""
    import torch

    from espm_amd.presence import _components, threshold
    q = threshold(level)
    if not lr_tol > 0:
        raise ValueError("lr_tol must be positive")
    max_eval = _positive_int(max_eval, "max_eval")
    sv = _Solver(X, H, tol, max_pass, chunk, log_shift, layout, device, "intervals")
    D0 = sv.check_start(D0)
    every, mask = sv.check_components(None)
    n, k = sv.n, sv.k
    cols = _components(components, k)[0]
    r, dev0 = _full_fit(sv, D0, every, mask)
    full = _host(r)
    pins = [j for j in cols for _ in (0, 1)]   # model 2 i: the lower end of column cols[i]; 2 i + 1: its upper end
    B = len(pins)
    with sv.image.scope():
        dev = sv.dev
        z = dict(dtype=torch.float64, device=dev)
        D_ml, dev_ml, ok = r["D"][0].contiguous().clone(), r["deviance"][0].clone(), r["done"][0] == 1
        pin_t = torch.tensor(pins, dtype=torch.int64, device=dev)
        up = (torch.arange(B, device=dev) % 2 == 1)[:, None]
        s = torch.from_numpy(sv.s).to(dev)
        sj = s[pin_t][:, None]
        h_ml = D_ml[:, pin_t].T.contiguous()                                    # (B, n)
        w0 = (q ** 0.5) * torch.sqrt(sj * h_ml + q) / sj
        inf, nan = float("inf"), float("nan")
        lo = torch.where(up, h_ml, torch.zeros_like(h_ml))
        hi = torch.where(up, torch.full_like(h_ml, inf), h_ml)
        t = torch.where(up, h_ml + w0, torch.zeros_like(h_ml)).contiguous()
        out = torch.full((B, n), nan, **z)
        conv = torch.zeros((B, n), dtype=torch.bool, device=dev)
        n_eval, n_pass = (torch.zeros((B, n), dtype=torch.int64, device=dev) for _ in range(2))
        active = ok[None, :].expand(B, n).clone()
        zero = active & ~up & (h_ml == 0)          # the lower end of an entry at the boundary: 0, without an evaluation
        out = torch.where(zero, torch.zeros_like(out), out)
        conv |= zero
        active &= ~zero
        # what a warm start is lifted to: the kernel's own fill N / (|M| s_i) * 1e-3 of a start that is not positive
        lift = None if k == 1 else (sv.counts()[:, None] / ((k - 1) * s)[None, :]) * START
        Dc = D_ml[None].repeat(B, 1, 1).contiguous()
        for ev in range(max_eval):
            if lift is not None:   # (the pinned column too: the step's start writes t over it)
                torch.maximum(Dc, lift[None], out=Dc)
            fit = sv.fit(Dc, pins, mask, t=t, done=(~active).to(torch.uint8).contiguous())
            if fit["started"] == 0:   # (every problem retired: the step's workgroups returned at entry)
                break
            fitted = active & (fit["done"] == 1)
            phi = fit["deviance"] - dev_ml[None, :] - q
            fin = fitted & (phi.abs() <= lr_tol)
            if ev == 0:
                fin |= fitted & ~up & (phi <= 0)   # the boundary: the band reaches 0
            out = torch.where(fin, t, out)
            conv |= fin
            n_eval += active
            n_pass += torch.where(active, fit["n_pass"].to(torch.int64), torch.zeros_like(n_pass))
            go = fitted & ~fin
            inner = torch.where(up, phi < 0, phi > 0)   # the evaluated point replaces the lower end of the bracket
            lo, hi = torch.where(go & inner, t, lo), torch.where(go & ~inner, t, hi)
            tn = t - phi / fit["slope"]
            open_ = torch.isinf(hi)
            good = torch.isfinite(tn) & (tn > lo) & (tn < hi)
            tn = torch.where(open_, torch.minimum(tn, h_ml + 8.0 * (t - h_ml)), tn)
            mid = torch.where(open_, h_ml + 2.0 * (t - h_ml), 0.5 * (lo + hi))
            nxt = torch.where(good, tn, mid)
            if ev == 0:   # (the slope at t = 0 belongs to the floor where nothing else is fitted)
                nxt = torch.where(up, nxt, torch.maximum(h_ml - w0, 0.5 * h_ml))
            t = torch.where(go, nxt, t).contiguous()
            active = go
        host = _image.to_host
        lower, upper = np.full((n, k), np.nan), np.full((n, k), np.nan)
        res = {key: np.zeros((k, 2, n), dtype=dt) for key, dt in (("converged", bool), ("n_eval", np.int64), ("n_pass", np.int64))}
        out_h, parts = host(out), dict(converged=host(conv), n_eval=host(n_eval), n_pass=host(n_pass))
        for i, j in enumerate(cols):
            lower[:, j], upper[:, j] = out_h[2 * i], out_h[2 * i + 1]
            for key in res:
                res[key][j] = parts[key][2 * i:2 * i + 2]
    return dict(D_ml=full["D"], deviance_ml=full["deviance"], lower=lower, upper=upper, level=float(level), threshold=q, **res,
                deviance_start=None if dev0 is None else host(dev0), N=host(sv.counts()), unmodelled=full["unmodelled"],
                nonfinite=full["nonfinite"])
