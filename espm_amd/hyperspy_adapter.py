"""The hyperspy side of the drop-in (reference: espm/datasets/eds_spim.py:113-139, :484-604,
:606-688, espm/hyperspy_extension.yaml, pyproject.toml:52-53).

The reference is a hyperspy extension: its signal class ``EDSespm`` exposes ``.X`` (the spectrum image as an (n, p)
matrix), ``.shape_2d`` and a ``decomposition(algorithm=est)`` that hands the unfolded data - (pixels, channels), hyperspy's
layout - to ``est.fit_transform`` (an estimator built with ``hspy_comp=True``), takes the loadings it returns and the
factors from ``est.components_``, and keeps the estimator as ``learning_results.decomposition_algorithm`` (from which the
reporting methods read ``W_``, ``G_``, ``H_`` after checking ``isinstance(..., NMFEstimator)``).

What is here:

* ``SpectrumImage`` - that contract without hyperspy: a light signal class over a (ny, nx, n) data cube with ``X``,
  ``shape_2d``, ``decomposition``, ``learning_results``, ``get_decomposition_loadings / _factors``.  It is what the tests
  drive (hyperspy is not installable in the build image), and it is usable on its own for a cube that did not come from
  hyperspy.  The (pixels, channels) view it hands over is the cube's own memory: with ``hspy_comp=True`` the estimator
  uploads it as it is (pixel-major is the engine's native ingest layout) - no host transpose, no device transpose.
* ``register()`` - where espm itself is installed, registers this package's ``NMFEstimator`` as a virtual subclass of the
  reference's abstract base (``abc.ABC.register``), so that ``EDSespm.plot_1D_results`` / ``concentration_report``
  (eds_spim.py:607, :639) accept a decomposition made with it.  Called by ``decompose`` below and harmless elsewhere.
* ``decompose(signal, est)`` - ``signal.decomposition(algorithm=est)`` on a real hyperspy signal (or a ``SpectrumImage``)
  with the checks the reference leaves to the user: ``hspy_comp`` must be on, ``shape_2d`` is taken from the signal when the
  estimator has none (the Laplacian needs the image grid, base.py:286-291).
* ``SpectrumImage.rebin`` / ``.estimate_best_binning`` (eds_spim.py:746-798 on integer factors, ``espm_amd.binning``) and
  ``decompose(signal, est, bin=(by, bx))``: the spectra fitted on the binned map, loadings at full resolution
  (``NMFEstimator.fit_binned``).
* ``SpectrumImage.thin(q, seed)`` (``espm_amd.splitting``: two independent count images from one) and
  ``decompose(signal, est, split=(q, seed))``: the fit of the thinned image, scored on the held-out counts
  (``NMFEstimator.fit_split``).
* ``SpectrumImage.simulate(est, seed, replicate)`` (``espm_amd.sampling``: a count image drawn from the fitted model),
  ``calibrated_deviance_maps(est)`` and ``bootstrap_maps(est)``: the maps of ``NMFEstimator.calibrate_deviance`` / ``bootstrap``.
* ``SpectrumImage.line_maps(lines)`` / ``.region_spectra(labels)`` (``espm_amd.marginals``: background-corrected line maps with their
  Poisson error bars and the sum spectrum of every region of a label map, from the raw cube; windows in channel indices) and
  ``line_maps(est)`` / ``region_spectra(est)``: the results of ``NMFEstimator.line_maps`` / ``region_spectra`` in the navigation
  and the signal shape.
* ``hyperspy_extension.yaml`` (next to this file) and the ``hyperspy.extensions`` entry point in ``pyproject.toml`` declare
  the signal type ``EDS_espm_amd`` -> ``EDSespmAMD`` below, defined only when hyperspy imports.
"""
from __future__ import annotations

import numpy as np


class LearningResults:
    """The attributes of hyperspy's ``LearningResults`` the reference reads (eds_spim.py:607-612, :639-644)."""

    def __init__(self):
        self.decomposition_algorithm = None
        self.factors = None          # (n, k)
        self.loadings = None         # (p, k)
        self.output_dimension = None
        self.navigation_mask = None
        self.signal_mask = None


class SpectrumImage:
    """A spectrum image (ny, nx, n) with the decomposition contract of hyperspy's ``Signal1D`` / the reference's ``EDSespm``.

    ``data`` is kept as given (no copy); ``X`` and the matrix handed to the estimator are views of it when it is
    C-contiguous."""

    def __init__(self, data):
        data = np.asarray(data)
        if data.ndim != 3:
            raise ValueError("a spectrum image is (rows, columns, channels)")
        self.data = data
        self.learning_results = LearningResults()

    @property
    def shape_2d(self):
        """(rows, columns) of the image, eds_spim.py:113-120."""
        return self.data.shape[0], self.data.shape[1]

    @property
    def X(self):
        """The data as (channels, pixels), eds_spim.py:122-131 (a view for a C-contiguous cube)."""
        ny, nx, n = self.data.shape
        return self.data.reshape((ny * nx, n)).T

    def unfolded(self):
        """(pixels, channels): what hyperspy's decomposition hands to a custom algorithm."""
        ny, nx, n = self.data.shape
        return self.data.reshape((ny * nx, n))

    def rebin(self, bin):
        """A new ``SpectrumImage`` of the sums over (by, bx) blocks of pixels (``espm_amd.binning.rebin`` on the device; the last
        bin row and column are smaller when the factors do not divide the image)."""
        from espm_amd import binning
        gny, gnx = binning.binned_shape(self.shape_2d, bin)
        return SpectrumImage(binning.rebin(self.unfolded(), self.shape_2d, bin, layout="pm").reshape((gny, gnx, self.data.shape[2])))

    def estimate_best_binning(self, bins=None, inspect=False):
        """The (by, bx) of least estimated risk among ``bins`` (by default the square bins up to half the image), or with
        ``inspect=True`` (risk of every candidate, best): eds_spim.py:746-798 on integer factors (``espm_amd.binning``)."""
        from espm_amd import binning
        return binning.estimate_best_binning(self.unfolded(), self.shape_2d, bins=bins, inspect=inspect, layout="pm")

    def thin(self, q=0.5, seed=0):
        """Two ``SpectrumImage``s of this one's shape and dtype: a Poisson-thinned part holding a fraction q of the counts and the rest,
        independent of each other for Poisson counts (``espm_amd.splitting.thin`` on the device; integer counts 0 .. 65535)."""
        from espm_amd import splitting
        Xa, Xb = splitting.thin(self.unfolded(), q=q, seed=seed, layout="pm")
        return SpectrumImage(Xa.reshape(self.data.shape)), SpectrumImage(Xb.reshape(self.data.shape))

    @staticmethod
    def simulate(est, seed=0, replicate=0, shape_2d=None):
        """A ``SpectrumImage`` (ny, nx, n) of 16-bit counts drawn from the fitted model of ``est`` (``NMFEstimator.simulate``: replicate
        ``replicate`` of ``G_ @ W_``, ``H_`` by the rule of ``espm_amd.sampling``).  ``shape_2d``: the image grid, by default the
        estimator's."""
        X = est.simulate(seed=seed, replicate=replicate)
        if not est.hspy_comp:
            X = np.ascontiguousarray(X.T)
        ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
        return SpectrumImage(X.reshape((ny, nx, X.shape[1])))

    def assign_counts(self, est, seed=0):
        """A list of k ``SpectrumImage``s of this one's shape and dtype, one per component of the fitted ``est``: every count of this
        image handed to one component by ``NMFEstimator.assign_counts`` (the rule of ``espm_amd.attribution``; integer counts
        0 .. 65535).  They add up to this image exactly, and for Poisson counts each is an independent noisy acquisition of its phase
        alone."""
        X = self.unfolded() if est.hspy_comp else self.X
        parts = est.assign_counts(X, seed=seed)
        if not est.hspy_comp:
            parts = np.ascontiguousarray(parts.transpose(0, 2, 1))
        return [SpectrumImage(part.reshape(self.data.shape)) for part in parts]

    def line_maps(self, lines):
        """(net (g, ny, nx), net_std (g, ny, nx)) of the raw cube, no estimator needed: the counts in every line's integration window
        less the background interpolated between its two side windows, and their Poisson standard deviation sqrt(sum u^2 x)
        (``espm_amd.marginals.line_maps`` on the device).  ``lines``: a list of ``(integration, background)`` in half-open ranges
        of CHANNEL INDICES, ``background`` None or ``((l0, l1), (r0, r1))`` - ``marginals.line_weights`` has the rule."""
        from espm_amd import marginals
        out = marginals.line_maps(self.unfolded(), lines, layout="pm")
        ny, nx = self.shape_2d
        return out["net"].reshape((-1, ny, nx)), out["net_std"].reshape((-1, ny, nx))

    def region_spectra(self, labels):
        """(L, n): the raw sum spectrum of every region of an integer label map (ny, nx) - negative labels belong to no region
        (``espm_amd.marginals.channel_spectra`` on the device)."""
        from espm_amd import marginals
        labels = np.asarray(labels)
        if labels.shape != self.shape_2d:
            raise ValueError(f"labels of shape {labels.shape} for an image of {self.shape_2d}")
        return marginals.channel_spectra(self.unfolded(), marginals.label_weights(labels), layout="pm")["counts"].T

    def scree(self, n_vectors=6):
        """The scree plot of the raw cube, no estimator needed: ``espm_amd.residuals.scree`` on the device - the singular values of the
        Pearson residual against the independence model, whose ``normalised_pca`` are the values hyperspy's Poisson-normalised PCA
        reports after its trivial first one; k phases show as k - 1 values above the bulk.  Returns that function's dict with the
        ``maps`` as (r, ny, nx) and the ``chi2_map`` as (ny, nx); the ``spectra`` stay (n, r)."""
        from espm_amd import residuals
        out = residuals.scree(self.unfolded(), n_vectors=n_vectors, layout="pm")
        ny, nx = self.shape_2d
        return dict(out, maps=out["maps"].reshape((-1, ny, nx)), chi2_map=out["chi2_map"].reshape((ny, nx)))

    def decomposition(self, algorithm, output_dimension=None, return_info=False, bin=None, split=None, **kwargs):
        """hyperspy's ``decomposition(algorithm=<object>)`` for a custom estimator: ``fit_transform(data (p, n))`` ->
        loadings (p, k), ``components_`` (k, n) -> factors (n, k); the estimator stays in ``learning_results``.  ``bin=(by, bx)``:
        ``algorithm.fit_binned`` instead - the spectra fitted on the binned image, the loadings at full resolution.
        ``split=(q, seed)``: ``algorithm.fit_split`` - the fit of the thinned image, with its held-out deviance on the estimator."""
        if not hasattr(algorithm, "fit_transform"):
            raise ValueError("algorithm must implement fit_transform() (scikit-learn style)")
        if kwargs:
            raise TypeError(f"unsupported decomposition arguments for a custom algorithm: {sorted(kwargs)}")
        if split is not None:
            q, seed = _check_split(split, bin)
            loadings = algorithm.fit_split(self.unfolded(), q=q, seed=seed)
        else:
            loadings = algorithm.fit_transform(self.unfolded()) if bin is None else algorithm.fit_binned(self.unfolded(), bin)
        factors = np.asarray(algorithm.components_).T
        lr = self.learning_results
        lr.decomposition_algorithm = algorithm
        lr.loadings, lr.factors = np.asarray(loadings), factors
        lr.output_dimension = factors.shape[1] if output_dimension is None else output_dimension
        if return_info:
            return algorithm

    def get_decomposition_loadings(self):
        """(k, ny, nx) maps."""
        ny, nx = self.shape_2d
        return self.learning_results.loadings.T.reshape((-1, ny, nx))

    def get_decomposition_factors(self):
        """(k, n) spectra."""
        return self.learning_results.factors.T

    def get_decomposition_diagnostics(self):
        """(deviance (ny, nx), H_std (k, ny, nx)) of the kept estimator, after its ``pixel_diagnostics()``."""
        return diagnostic_maps(self.learning_results.decomposition_algorithm, self.shape_2d)

    def get_decomposition_diagnostic_spectra(self):
        """(channel_deviance (n,), sum_spectrum (n,), model_spectrum (n,), D_std (k, n)) of the kept estimator, after its
        ``spectral_diagnostics()``."""
        return diagnostic_spectra(self.learning_results.decomposition_algorithm)


def diagnostic_maps(est, shape_2d=None):
    """``est.deviance_`` and ``est.H_std_`` (set by ``est.pixel_diagnostics()``) in the navigation shape, like the loadings:
    (ny, nx) and (k, ny, nx).  ``shape_2d``: the image grid, by default the estimator's."""
    if not hasattr(est, "deviance_"):
        raise AttributeError("call est.pixel_diagnostics() first: it sets deviance_ and H_std_")
    ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
    return np.asarray(est.deviance_).reshape((ny, nx)), np.asarray(est.H_std_).reshape((-1, ny, nx))


def presence_maps(est, shape_2d=None, method=None):
    """``est.H_ml_``, ``est.presence_lr_`` and ``est.presence_pvalue_`` (set by ``est.presence_maps()``) in the navigation shape, like
    the loadings: (k, ny, nx) each - the per-pixel ML abundances, the likelihood-ratio statistic of every phase's presence and its
    asymptotic p-value.  ``method``: None takes the maps as the last ``est.presence_maps()`` left them; "em", "newton" or
    "simplex" (the test under sum h = 1, for an estimator with ``simplex_H=True``) runs ``est.presence_maps(method=method)`` on the
    fit's own image first."""
    if method is not None:
        est.presence_maps(method=method)
    if not hasattr(est, "presence_lr_"):
        raise AttributeError("call est.presence_maps() first: it sets H_ml_, presence_lr_ and presence_pvalue_")
    ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
    return tuple(np.asarray(a).reshape((-1, ny, nx)) for a in (est.H_ml_, est.presence_lr_, est.presence_pvalue_))


def element_presence(est):
    """What ``est.element_presence()`` set, as a dict of (elements, phases) tables beside ``W_``: ``W_ml`` (the maximum-likelihood
    concentrations given the abundances), ``lr`` (the likelihood-ratio statistic of every entry's presence), ``pvalue`` (its
    asymptotic p-value; NaN where the entry was not tested), and ``entries``, ``converged``, ``gap``, ``n_pass`` of the fits."""
    if not hasattr(est, "W_presence_lr_"):
        raise AttributeError("call est.element_presence() first: it sets W_ml_, W_presence_lr_ and W_presence_pvalue_")
    return dict(W_ml=est.W_ml_, deviance_ml=est.W_deviance_ml_, lr=est.W_presence_lr_, pvalue=est.W_presence_pvalue_,
                entries=est.W_presence_entries_, converged=est.W_ml_converged_, gap=est.W_ml_gap_, n_pass=est.W_ml_n_pass_)


def concentration_intervals(est):
    """What ``est.concentration_intervals()`` set, as a dict of (elements, phases) tables beside ``W_``: ``W_ml`` (the
    maximum-likelihood concentrations given the abundances), ``lower`` and ``upper`` (the ends of every tested entry's
    profile-likelihood interval; ``upper`` is an upper limit where ``lower`` is 0; NaN where the entry was not tested), and ``level``,
    ``entries``, ``converged``, ``n_eval`` of the ends."""
    if not hasattr(est, "W_upper_"):
        raise AttributeError("call est.concentration_intervals() first: it sets W_ml_, W_lower_ and W_upper_")
    return dict(W_ml=est.W_ml_, deviance_ml=est.W_deviance_ml_, lower=est.W_lower_, upper=est.W_upper_, level=est.W_interval_level_,
                entries=est.W_interval_entries_, converged=est.W_interval_converged_, n_eval=est.W_interval_n_eval_)


def spectrum_bands(est):
    """What ``est.spectrum_intervals()`` and ``est.spectrum_presence()`` set, on the signal axis like the factors - a dict of (k, n)
    tables: ``D_ml`` (the maximum-likelihood spectra given the abundances, no dictionary behind them), and after
    ``spectrum_intervals()`` ``lower`` and ``upper`` (the profile-likelihood band of every spectrum; ``upper`` is an upper limit where
    ``lower`` is 0; NaN where a component was not asked for) with ``level``; after ``spectrum_presence()`` ``lr`` and ``pvalue`` (is
    component j in this channel at all) and ``excess_deviance`` (n,): what the fitted spectra lose against free ones, per channel."""
    if not hasattr(est, "D_ml_"):
        raise AttributeError("call est.spectrum_intervals() or est.spectrum_presence() first: they set D_ml_ and the tables beside it")
    out = dict(D_ml=np.asarray(est.D_ml_).T)
    if hasattr(est, "D_upper_"):
        out.update(lower=np.asarray(est.D_lower_).T, upper=np.asarray(est.D_upper_).T, level=est.D_interval_level_)
    if hasattr(est, "D_presence_lr_"):
        out.update(lr=np.asarray(est.D_presence_lr_).T, pvalue=np.asarray(est.D_presence_pvalue_).T,
                   excess_deviance=np.asarray(est.D_excess_deviance_))
    return out


def abundance_interval_maps(est, shape_2d=None):
    """``est.H_lower_`` and ``est.H_upper_`` (set by ``est.abundance_intervals()``) in the navigation shape, like the loadings:
    (k, ny, nx) each - the ends of the profile-likelihood interval of every abundance; the upper map is the detection limit where
    the lower one is 0."""
    if not hasattr(est, "H_upper_"):
        raise AttributeError("call est.abundance_intervals() first: it sets H_lower_ and H_upper_")
    ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
    return tuple(np.asarray(a).reshape((-1, ny, nx)) for a in (est.H_lower_, est.H_upper_))


def calibrated_deviance_maps(est, shape_2d=None):
    """``est.deviance_z_`` and ``est.deviance_pvalue_`` (set by ``est.calibrate_deviance()``) in the navigation shape: (ny, nx) each."""
    if not hasattr(est, "deviance_z_"):
        raise AttributeError("call est.calibrate_deviance() first: it sets deviance_z_ and deviance_pvalue_")
    ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
    return np.asarray(est.deviance_z_).reshape((ny, nx)), np.asarray(est.deviance_pvalue_).reshape((ny, nx))


def bootstrap_maps(est, shape_2d=None):
    """``est.H_boot_std_`` (set by ``est.bootstrap()``) in the navigation shape, like the loadings: (k, ny, nx)."""
    if not hasattr(est, "H_boot_std_"):
        raise AttributeError("call est.bootstrap() first: it sets H_boot_std_")
    ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
    return np.asarray(est.H_boot_std_).reshape((-1, ny, nx))


def component_count_maps(est, shape_2d=None):
    """``est.pixel_counts_`` (set by ``est.attribute_counts()``) in the navigation shape, like the loadings: (k, ny, nx) maps of the
    measured counts behind every component.  ``shape_2d``: the image grid, by default the estimator's."""
    if not hasattr(est, "pixel_counts_"):
        raise AttributeError("call est.attribute_counts() first: it sets pixel_counts_ and channel_counts_")
    ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
    return np.asarray(est.pixel_counts_).reshape((-1, ny, nx))


def component_spectra(est):
    """``est.channel_counts_`` (set by ``est.attribute_counts()``) on the signal axis, like the factors: (k, n) spectra of the measured
    counts behind every component; they add up to the measured sum spectrum (less the unattributed counts)."""
    if not hasattr(est, "channel_counts_"):
        raise AttributeError("call est.attribute_counts() first: it sets pixel_counts_ and channel_counts_")
    return np.asarray(est.channel_counts_).T


def line_maps(est, shape_2d=None):
    """``est.line_net_``, ``est.line_net_std_``, ``est.line_model_`` as (g, ny, nx) and ``est.line_components_`` as (g, k, ny, nx) (set by
    ``est.line_maps()``) in the navigation shape, like the loadings: the measured line next to the modelled one and every component's
    share of it.  ``shape_2d``: the image grid, by default the estimator's."""
    if not hasattr(est, "line_net_"):
        raise AttributeError("call est.line_maps() first: it sets line_net_, line_net_std_, line_model_ and line_components_")
    ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
    g, k = np.asarray(est.line_components_).shape[:2]
    return (np.asarray(est.line_net_).reshape((g, ny, nx)), np.asarray(est.line_net_std_).reshape((g, ny, nx)),
            np.asarray(est.line_model_).reshape((g, ny, nx)), np.asarray(est.line_components_).reshape((g, k, ny, nx)))


def region_spectra(est):
    """``est.region_counts_``, ``est.region_model_`` and ``est.region_deviance_`` as (L, n) (set by ``est.region_spectra()``) on the
    signal axis, like the factors: the measured, the modelled and the residual spectrum of every region."""
    if not hasattr(est, "region_counts_"):
        raise AttributeError("call est.region_spectra() first: it sets region_counts_, region_model_, region_deviance_ and region_pixels_")
    return np.asarray(est.region_counts_).T, np.asarray(est.region_model_).T, np.asarray(est.region_deviance_).T


def residual_components(est, shape_2d=None):
    """``est.residual_maps_`` as (r, ny, nx), in the navigation shape like the loadings, and ``est.residual_spectra_`` as (r, n), on
    the signal axis like the factors (set by ``est.residual_components()``): where a missing phase sits and what it looks like.
    ``shape_2d``: the image grid, by default the estimator's."""
    if not hasattr(est, "residual_maps_"):
        raise AttributeError("call est.residual_components() first: it sets residual_maps_ and residual_spectra_")
    ny, nx = (int(v) for v in (shape_2d if shape_2d is not None else est.shape_2d))
    return np.asarray(est.residual_maps_).reshape((-1, ny, nx)), np.asarray(est.residual_spectra_).T


def diagnostic_spectra(est):
    """``est.channel_deviance_``, ``est.sum_spectrum_``, ``est.model_spectrum_`` (n,) and ``est.D_std_`` as (k, n) (set by
    ``est.spectral_diagnostics()``) on the signal axis, like the factors: the residual spectrum next to the measured and the
    modelled sum spectrum, and the error band of every component's spectrum."""
    if not hasattr(est, "channel_deviance_"):
        raise AttributeError("call est.spectral_diagnostics() first: it sets channel_deviance_, sum_spectrum_, model_spectrum_ and D_std_")
    return (np.asarray(est.channel_deviance_), np.asarray(est.sum_spectrum_), np.asarray(est.model_spectrum_),
            np.asarray(est.D_std_).T)


def register():
    """``espm.estimators.NMFEstimator.register(espm_amd.estimators.NMFEstimator)`` where espm is importable: the reference's
    ``isinstance(learning_results.decomposition_algorithm, NMFEstimator)`` gates then accept this package's estimators.
    Returns True when registered."""
    from espm_amd.estimators import NMFEstimator
    try:
        from espm.estimators import NMFEstimator as RefBase
    except Exception:
        return False
    RefBase.register(NMFEstimator)
    return True


def _check_split(split, bin):
    """(q, seed) of ``split``; ValueError when ``bin`` is given too (a binned fit of a thinned image is two calls, in that order)."""
    if bin is not None:
        raise ValueError("split and bin exclude each other: thin the image (SpectrumImage.thin) and decompose a part with bin")
    try:
        q, seed = split
    except (TypeError, ValueError):
        raise ValueError(f"split is a pair (q, seed), not {split!r}") from None
    return q, seed


def decompose(signal, est, bin=None, split=None, **kwargs):
    """``signal.decomposition(algorithm=est)`` with the estimator set up for hyperspy's calling convention.  ``bin=(by, bx)``
    routes to ``est.fit_binned``: the spectra are fitted on the binned image and ``learning_results`` holds full-resolution
    loadings (a ``SpectrumImage``, or any signal with ``shape_2d`` and a (pixels, channels) view of its data).
    ``split=(q, seed)`` routes to ``est.fit_split``: the fit of the thinned image, ``est.heldout_deviance_`` its score on the counts
    held out; together with ``bin``: ValueError."""
    if split is not None:
        _check_split(split, bin)
    if not getattr(est, "hspy_comp", False):
        raise ValueError("hyperspy hands (pixels, channels) to the estimator: build it with hspy_comp=True "
                         "(espm/estimators/base.py:249-259 only warns)")
    if getattr(est, "shape_2d", None) is None and hasattr(signal, "shape_2d"):
        est.shape_2d = tuple(int(v) for v in signal.shape_2d)
    register()
    if bin is None and split is None:
        signal.decomposition(algorithm=est, **kwargs)
    elif isinstance(signal, SpectrumImage):
        signal.decomposition(algorithm=est, bin=bin, split=split, **kwargs)
    else:   # (hyperspy's own decomposition knows no bin and no split: its results are filled as it fills them for a custom algorithm)
        if kwargs:
            raise TypeError(f"unsupported decomposition arguments with {'bin' if split is None else 'split'}: {sorted(kwargs)}")
        data = np.asarray(signal.data)
        flat = data.reshape((-1, data.shape[-1]))
        loadings = est.fit_binned(flat, bin) if split is None else est.fit_split(flat, q=split[0], seed=split[1])
        lr = signal.learning_results
        lr.decomposition_algorithm = est
        lr.loadings, lr.factors = np.asarray(loadings), np.asarray(est.components_).T
        lr.output_dimension = lr.factors.shape[1]
    return signal.learning_results


try:  # the real signal class, where hyperspy is installed (hyperspy_extension.yaml names it)
    import hyperspy.api as _hs

    class EDSespmAMD(_hs.signals.Signal1D):
        """hyperspy signal with the reference's ``X`` / ``shape_2d`` accessors (eds_spim.py:113-131); decompositions go
        through hyperspy's own ``decomposition`` with an ``espm_amd`` estimator as the ``algorithm`` object."""
        _signal_type = "EDS_espm_amd"

        @property
        def shape_2d(self):
            return self.axes_manager[1].size, self.axes_manager[0].size

        @property
        def X(self):
            shape = self.axes_manager[1].size, self.axes_manager[0].size, self.axes_manager[2].size
            return self.data.reshape((shape[0] * shape[1], shape[2])).T

        def get_decomposition_diagnostic_spectra(self):
            """(channel_deviance, sum_spectrum, model_spectrum (n,), D_std (k, n)) of the kept estimator, after its
            ``spectral_diagnostics()``."""
            return diagnostic_spectra(self.learning_results.decomposition_algorithm)
except Exception:  # pragma: no cover - hyperspy is absent in the build image
    EDSespmAMD = None
