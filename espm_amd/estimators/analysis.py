"""What an estimator does with a fit besides fitting (no reference analogue; ``NMFEstimator`` inherits the mixin): the fits around
``fit_transform`` - on the binned image, on a thinned image - and the analyses of a fitted model - diagnostics, count attribution,
line maps and region spectra, residual components, draws from the model.  Each method prepares host arrays and hands them to ``espm_amd.binning``,
``splitting``, ``measures``, ``attribution``, ``marginals``, ``residuals``, ``presence``, ``spectra_ml``, ``channel_ml`` or ``sampling``, imported when it is called; the set-up they share stands once, ahead of them.  The fit itself, ``unmix``
and the engine plumbing are next door in base.py.
"""
from __future__ import annotations

import numpy as np
from sklearn.utils.validation import check_is_fitted


class _FitAnalysis:
    """The post-fit methods of ``NMFEstimator``.  No ``__init__`` and no parameters: ``get_params``, ``clone`` and pickling are the
    estimator's."""

    # (what fit_binned and fit_split set beside the fit's own attributes: a later plain fit removes them)
    _BINNED_ATTRIBUTES = ("bin_", "binned_shape_2d_", "W_binned_", "H_binned_")
    _SPLIT_ATTRIBUTES = ("split_q_", "split_seed_", "heldout_deviance_", "train_deviance_", "heldout_deviance_map_", "train_deviance_map_",
                         "heldout_counts_")

    # ---- set-up the methods share ------------------------------------------------------------------------------------------------
    def _layout(self):
        """How the estimator's X is laid out: "pm", (pixels, channels), with ``hspy_comp``, else "cm"."""
        return "pm" if self.hspy_comp else "cm"

    def _model_factors(self):
        """(G, W, H) of the fitted model in fp64, G None for an identity G: for the callers that need the factors apart (they form
        G @ W, if at all, from these - in fp64 - and not through ``_model_counts``)."""
        G = None if self._identity_G else np.asarray(self.G_, dtype=np.float64)
        return G, np.asarray(self.W_, dtype=np.float64), np.asarray(self.H_, dtype=np.float64)

    def _model_counts(self):
        """(D, H) in fp64: the fitted spectra ``G_ @ W_`` (n, k) - ``W_`` itself for an identity G - and ``H_`` (k, p), in counts.
        (The product is formed in the fit's own dtype and then widened.)"""
        D = np.asarray(self.W_ if self._identity_G else self.G_ @ self.W_, dtype=np.float64)
        return D, np.asarray(self.H_, dtype=np.float64)

    def _fitted_binned(self):
        return getattr(self, "bin_", None) is not None

    def _refuse_binned_X(self, who):
        """After fit_binned, X_ is the BINNED image while W_, H_ and norm_factor_ belong to full-resolution pixels."""
        if self._fitted_binned():
            raise ValueError(f"{who}: this estimator was fitted by fit_binned with bin {self.bin_}: X_ holds the binned image, "
                             "H_ the full-resolution pixels - pass the full-resolution X")

    def _image_argument(self, X, who):
        """(X, layout) of the ``X`` argument of ``who``: ``None`` is the fit's ``X_`` un-scaled, channel-major (refused after
        ``fit_binned``); a given X is laid out by ``hspy_comp`` and has the channels of ``G_`` and the pixels of ``H_`` (ValueError)."""
        if X is None:
            check_is_fitted(self, "X_")
            self._refuse_binned_X(who)
            return np.asarray(self._X_fixed()), "cm"
        if not hasattr(X, "shape") or getattr(X, "ndim", 0) != 2:
            X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("X must be 2-D")
        n, p = (X.shape[1], X.shape[0]) if self.hspy_comp else (X.shape[0], X.shape[1])
        if n != self.G_.shape[0]:
            raise ValueError(f"X has {n} channels, the fitted G_ has {self.G_.shape[0]}")
        if p != self.H_.shape[1]:
            raise ValueError(f"X has {p} pixels, the fitted H_ has {self.H_.shape[1]}")
        return X, self._layout()

    def _counts_for_fit(self, Xint):
        """Integer counts (a host array) as the floating-point image ``fit_transform`` takes."""
        # (counts up to 65535 are exact in float32; handed over as integers, scikit-learn's validation would make them float64)
        return Xint.astype(np.float64 if self._fp64() else np.float32)

    # ---- fit on the binned image, abundances at full resolution ------------------------------------------------------------------
    def fit_binned(self, X, bin, y=None, W=None):
        """Fit the spectra on the image binned by ``bin = (by, bx)`` and return H at full resolution (H.T with ``hspy_comp``): the
        workflow the reference leaves to the user around ``estimate_best_binning`` (eds_spim.py:746-798) - decompose the binned
        map, read the abundances back on the pixels - with the scaling between the two carried here.

        1. ``espm_amd.binning.rebin`` sums X over the bins on the device; ``fit_transform`` runs on the binned image with
           ``shape_2d`` set to the binned grid (``lambda_L`` acts on that grid with the value given; ``W``: its initial W).  Kept:
           ``bin_``, ``binned_shape_2d_``, ``W_binned_``, ``H_binned_`` (a later plain fit removes them); ``n_iter_``, ``losses_``
           and ``X_`` stay the coarse fit's: ``X_`` is the binned image, so ``pixel_diagnostics`` / ``spectral_diagnostics`` ask
           for the full-resolution X instead of taking ``X_`` (ValueError with ``X=None``).
        2. A pixel's model is its bin's model over B = by bx.  Under ``normalize``: ``norm_factor_`` times B - the value
           ``normalization_factor`` gives for X itself - and ``W_ = W_binned_ / B``, so that ``W_ * norm_factor_`` is the normalised
           W the coarse fit ended with.  Without: ``W_ = W_binned_ / B``, except under ``simplex_W``, where W keeps its simplex and H
           carries the 1 / B.
        3. ``H_ = unmix(X, H=H0)``: the H-only fit of X against ``W_``, started from every pixel's bin column of the coarse H
           (over B where W kept its simplex; renormalised under ``simplex_H``).  ``transform_n_iter_``, ``transform_losses_``,
           ``transform_rel_`` and ``transform_path_`` hold the record of this stage; ``shape_2d`` is the full grid again.

        X: a host array, (channels, pixels), or (pixels, channels) with ``hspy_comp``; the binned image comes back to the host for
        the coarse fit (it is B times smaller).  Sharded and fp64 fits are out of scope.  Refused before anything is uploaded: whatever ``unmix`` refuses (linesearch,
        algo='projected_gradient', l2=True, shard(), fp64 mode) and ``fixed_H``, which belongs to full-resolution pixels
        (NotImplementedError); ``shape_2d`` unset, or factors that do not divide the image (ValueError: the message names the crop
        that would)."""
        from espm_amd import binning
        why = self._transform_refusal()
        if why is not None:
            raise NotImplementedError(f"fit_binned does not cover {why}")
        if self.fixed_H is not None:
            raise NotImplementedError("fit_binned does not cover fixed_H: its entries belong to full-resolution pixels")
        if self.shape_2d is None:
            raise ValueError("fit_binned needs the grid of the pixels: build the estimator with shape_2d=(rows, columns)")
        by, bx = binning._check_bin(bin)
        full = (int(self.shape_2d[0]), int(self.shape_2d[1]))
        ny, nx = full
        if ny % by or nx % bx:
            raise ValueError(f"bin {(by, bx)} does not divide the image {full}: crop it to {(ny - ny % by, nx - nx % bx)}")
        Xb = binning.rebin(X, full, (by, bx), layout=self._layout())   # (ValueError when shape_2d does not match X)
        coarse = (ny // by, nx // bx)
        given_shape = self.shape_2d
        self.shape_2d = coarse
        try:
            self.fit_transform(Xb, W=W)
        finally:
            self.shape_2d = given_shape
        B = by * bx
        self.bin_, self.binned_shape_2d_ = (by, bx), coarse
        self.W_binned_, self.H_binned_ = self.W_, self.H_
        k = self.H_binned_.shape[0]
        H0 = np.asarray(self.H_binned_, dtype=np.float64).reshape(k, coarse[0], coarse[1]).repeat(by, axis=1).repeat(bx, axis=2).reshape(k, ny * nx)
        if self.normalize:
            self.norm_factor_ = self.norm_factor_ * B
            self.W_ = self.W_binned_ / B
        elif self.simplex_W:
            H0 = H0 / B
        else:
            self.W_ = self.W_binned_ / B
        if self.simplex_H:
            H0 = H0 / H0.sum(axis=0, keepdims=True)
        self._L_cache, self._L_pixels = None, ny * nx
        Hn = self.unmix(X, H=H0.T if self.hspy_comp else H0)
        self.H_ = Hn.T if self.hspy_comp else Hn
        self.components_ = (self.G_ @ self.W_).T if self.hspy_comp else self.H_
        return Hn

    # ---- fit on a thinned image, scored on the counts held out ----------------------------------------------------------------------
    def _split_refusal(self):
        if getattr(self, "_shard_group", None) is not None:
            raise NotImplementedError("fit_split does not cover shard(): the split and its score run on one GPU")

    def fit_split(self, X, q=0.8, seed=0, y=None, W=None, H=None):
        """Fit on a Poisson-thinned part of the count image X and score the fit on the counts it has not seen (``espm_amd.splitting``;
        no reference analogue): the honest score for ``n_components``, ``mu``, ``lambda_L`` or a bin that the in-sample deviance
        cannot be.

        1. ``splitting.thin(X, q, seed)`` on the device: X_a holds a fraction q_eff = round(q 2^32) / 2^32 of every entry's counts,
           X_b = X - X_a the rest, independent of it for Poisson X.  X_a comes to the host and ``fit_transform(X_a, W=W, H=H)`` runs on
           it as on any image.
        2. ``splitting.split_deviance`` regenerates the split from (X, seed) and evaluates the fitted model ``G_ @ W_``, ``H_`` on
           both parts, the held-out one against the model scaled by (1 - q_eff) / q_eff.

        EVERY fitted attribute (``W_``, ``H_``, ``X_``, ``norm_factor_``, ``losses_``, ...) is that of the TRAINING image, at the dose
        q_eff of X: the model is not rescaled to the full dose.  Set in addition: ``split_q_`` (q_eff), ``split_seed_``,
        ``heldout_deviance_`` and ``train_deviance_`` (totals), ``heldout_deviance_map_`` and ``train_deviance_map_`` (p,),
        ``heldout_counts_`` (p,) int64; a later plain fit removes them.  Returns what ``fit_transform`` returns.

        X: integer counts 0 .. 65535 - a host array or a device tensor, (channels, pixels), or (pixels, channels) with ``hspy_comp``;
        TypeError for floating-point X, ValueError for values out of range, before anything is uploaded.  Every solver, G kind and
        precision mode, 1 .. 32 components; ``shard()``ed estimators raise NotImplementedError before anything is uploaded."""
        from espm_amd import _image, splitting
        self._split_refusal()
        layout = self._layout()
        Xd = splitting._resident(X, q, seed, layout)   # (one upload for the split and the score: 1 or 2 bytes per entry stay on the device)
        Xa = _image.to_host(splitting._thin(Xd, q, seed, layout, False)[0])
        return self._fit_split_stages(Xd, Xa, q, seed, layout, W=W, H=H)

    def _fit_split_stages(self, X, Xa, q, seed, layout, W=None, H=None):
        """The fit of the training image Xa = thin(X, q, seed)[0] (a host array) and its score on both parts of X (the device copy);
        fit_split, and splitting.scan, which shares both among its estimators."""
        from espm_amd import splitting
        out = self.fit_transform(self._counts_for_fit(Xa), W=W, H=H)
        D, Hf = self._model_counts()
        s = splitting.split_deviance(X, D, Hf, q=q, seed=seed, log_shift=self.log_shift, layout=layout)
        self.split_q_, self.split_seed_ = s["q_eff"], int(seed)
        self.heldout_deviance_, self.train_deviance_ = s["heldout"], s["train"]
        self.heldout_deviance_map_, self.train_deviance_map_, self.heldout_counts_ = s["heldout_map"], s["train_map"], s["heldout_counts"]
        return out

    # ---- diagnostics of the fit: where it fails, and an error bar on every abundance ---------------------------------------------
    def pixel_diagnostics(self, X=None):
        """Per-pixel deviance and error bars of ``H_`` (``espm_amd.measures.pixel_diagnostics`` on ``G_ @ W_`` and ``H_``; the reference
        has no analogue - hyperspy's model fitting reports the same two things as ``red_chisq`` and the parameters' ``std``).

        Sets ``deviance_`` (p,): the Poisson deviance 2 sum_c (x ln(x / y) - x + y) of every pixel, and ``H_std_`` (k, p), oriented as
        ``H_``: the Cramer-Rao bound of every abundance given the fitted spectra, under the constraint sum_i h_i = 1 when the estimator
        has ``simplex_H``.  Pixels whose Fisher information is numerically singular hold NaN in ``H_std_`` and are counted in
        ``n_singular``.  The bound ignores the uncertainty of ``W_``, the regularisers (``mu``, ``lambda_L``) and abundances held at
        the ``log_shift`` floor: it is the error bar given the spectra.  Returns dict(deviance, H_std, n_singular); with ``hspy_comp``
        the returned ``H_std`` is (p, k), as ``fit_transform`` returns ``H_.T``.

        ``X``: the fitted image in counts - (channels, pixels), or (pixels, channels) with ``hspy_comp``, as for ``unmix`` - in any
        dtype ``measures.pixel_diagnostics`` reads; ValueError when its channels do not match ``G_`` or its pixels ``H_``.
        ``X=None`` takes the fit's ``X_`` un-scaled (``X_ / norm_factor_`` under ``normalize``); lines of the image without a count
        carry the ``log_shift`` fill there, so passing the original X is the exact one.  It is also the cheap one: under ``normalize``
        ``X=None`` builds the un-scaled image as a host array in ``X_``'s dtype and uploads it as such - for a fit of 8- or 16-bit
        counts that is 4 or 8 bytes per entry on the host and again on the device (4.3 GB each at 2048 x 512 x 512 in fp64) against 1
        or 2 for the original counts, so at large sizes pass the X that was fitted.  Computed in fp64 whatever the estimator's
        precision, on the current device (a ``shard()``ed estimator: every rank holds the whole ``W_`` and ``H_`` and computes all
        pixels on its own device).  More than 8 components raise NotImplementedError before anything is uploaded."""
        from espm_amd import measures
        check_is_fitted(self, "W_")
        k = int(self.H_.shape[0])
        if k > 8:
            raise NotImplementedError(f"pixel_diagnostics: {k} components (the kernel is built for 1..8)")
        X, layout = self._image_argument(X, "pixel_diagnostics")
        D, H = self._model_counts()
        out = measures.pixel_diagnostics(X, D, H, simplex_H=bool(self.simplex_H), log_shift=self.log_shift, layout=layout)
        self.deviance_, self.H_std_ = out["deviance"], out["H_std"]
        if self.hspy_comp:
            out = dict(out, H_std=out["H_std"].T)
        return out

    def spectral_diagnostics(self, X=None):
        """Per-channel deviance and error bars of ``W_`` (``espm_amd.measures.spectral_diagnostics`` on ``G_``, ``W_`` and ``H_``): the
        spectral half of ``pixel_diagnostics``.

        Sets ``channel_deviance_`` (n,): the Poisson deviance 2 sum_p (x ln(x / y) - x + y) of every energy channel - the residual
        spectrum, in which a missing line or element shows as a narrow band; ``sum_spectrum_`` and ``model_spectrum_`` (n,): the
        measured and the modelled sum spectrum; ``W_std_``, of ``W_``'s shape: the Cramer-Rao bound of every entry of ``W_`` given
        the fitted abundances (with a physics model or a dictionary G: the error bars of the concentrations); ``D_std_`` (n, k): the
        bound on the spectra ``G_ @ W_``.  With ``simplex_W`` the bound is the one under the constraint the fit imposed: the rows
        ``physics_model_.NMF_simplex()`` of W sum to one per component with a physics model, all rows otherwise.  Channels (or, with
        G, the whole matrix) whose Fisher information is numerically singular hold NaN and are counted in ``n_singular``.  The bound
        ignores the uncertainty of ``H_``, the regularisers (``mu``, ``lambda_L``) and entries held at the ``log_shift`` floor: it
        is the error bar given the abundances.  Returns dict(channel_deviance, sum_spectrum, model_spectrum, M, W_std, D_std,
        n_singular); all of it is indexed by channel or by W's rows, so ``hspy_comp`` changes only how ``X`` is read.

        ``X``: as for ``pixel_diagnostics`` - the fitted image in counts, (channels, pixels), or (pixels, channels) with
        ``hspy_comp``; ValueError when its channels do not match ``G_`` or its pixels ``H_``.  ``X=None`` takes the fit's ``X_``
        un-scaled, with the same cost as there: under ``normalize`` that is a host array in ``X_``'s dtype, 4 or 8 bytes per entry on
        the host and again on the device against 1 or 2 for the original counts, and lines without a count carry the ``log_shift``
        fill - at large sizes pass the X that was fitted.  Computed in fp64 whatever the estimator's precision, on the current device
        (a ``shard()``ed estimator: every rank holds the whole ``W_`` and ``H_`` and computes everything on its own device).  More
        than 8 components raise NotImplementedError before anything is uploaded, and so does an estimator with imposed ``fixed_W``
        entries: taking imposed entries out of the information matrix is a later step."""
        from espm_amd import measures
        check_is_fitted(self, "W_")
        k = int(self.H_.shape[0])
        if k > 8:
            raise NotImplementedError(f"spectral_diagnostics: {k} components (the kernel is built for 1..8)")
        if self.fixed_W is not None and (np.asarray(self.fixed_W) >= 0).any():
            raise NotImplementedError("spectral_diagnostics: the bound with imposed fixed_W entries is not implemented")
        X, layout = self._image_argument(X, "spectral_diagnostics")
        rows = None
        if self.simplex_W and getattr(self, "algo", None) != "bmd" and not self.l2:   # (the W step that had a simplex: _make_engine)
            rows = self.physics_model_.NMF_simplex() if self.physics_model_ is not None else True
        G, W, H = self._model_factors()
        out = measures.spectral_diagnostics(X, W, H, G=G, simplex_rows=rows, log_shift=self.log_shift, layout=layout)
        self.channel_deviance_, self.sum_spectrum_, self.model_spectrum_ = out["channel_deviance"], out["sum_spectrum"], out["model_spectrum"]
        self.W_std_, self.D_std_ = out["W_std"], out["D_std"]
        return out

    # ---- the measured counts behind every component: in expectation, and as a random split of the image ---------------------------
    def attribute_counts(self, X=None):
        """How many of the MEASURED counts stand behind every component (``espm_amd.attribution.expected`` on ``G_ @ W_`` and ``H_``):
        entry (c, p) of X gives x d_cj h_jp / y counts to component j.  The reference quotes the MODELLED intensity instead
        (``utils.get_explained_intensity_W``, the ``sqrt(N) / N`` of ``concentration_report(fit_error=True)``); the two agree at an
        unregularised fixed point and differ with ``mu``, ``lambda_L``, a simplex, a floor or a fit that stopped early.

        Sets ``pixel_counts_`` (k, p), oriented as ``H_``; ``channel_counts_`` (n, k); ``intensity_W_``, of ``W_``'s shape: the measured
        counts behind every entry of ``W_`` (with a physics model or a dictionary G: W o (G^T R)); ``model_intensity_W_``: the
        reference's function on ``G_``, ``W_``, ``H_``; ``intensity_rel_error_`` = 1 / sqrt(``intensity_W_``), inf where 0 (times 100:
        the reference's percentage); ``component_counts_`` (k,); ``explained_counts_ratio_`` (k,) = ``component_counts_`` / total
        counts, the NMF analogue of an explained-variance ratio; ``unattributed_counts_``: the counts of entries whose model fell
        below ``log_shift``.  Returns them as a dict (keys without the underscore); with ``hspy_comp`` the returned
        ``pixel_counts`` is (p, k), as ``fit_transform`` returns ``H_.T``.

        ``X`` as for ``pixel_diagnostics``: the fitted image in counts, (channels, pixels), or (pixels, channels) with ``hspy_comp``;
        ``X=None`` takes the fit's ``X_`` un-scaled, with the cost and the ``log_shift`` fill described there.  Computed in fp64
        whatever the estimator's precision, on the current device (a ``shard()``ed estimator: every rank computes everything on its
        own device).  1 .. 32 components."""
        from espm_amd import attribution
        from espm_amd.utils import get_explained_intensity_W
        check_is_fitted(self, "W_")
        k = int(self.H_.shape[0])
        if k > attribution.MAX_K:
            raise NotImplementedError(f"attribute_counts: {k} components (the kernels are built for 1..{attribution.MAX_K})")
        X, layout = self._image_argument(X, "attribute_counts")
        G, W, H = self._model_factors()
        out = attribution.expected(X, W if G is None else G @ W, H, log_shift=self.log_shift, layout=layout)
        self.pixel_counts_, self.channel_counts_ = out["pixel_counts"], out["channel_counts"]
        self.intensity_W_ = attribution.intensity(G, W, out["ratio_sums"])
        self.model_intensity_W_ = get_explained_intensity_W(np.asarray(self.G_, dtype=np.float64), W, H)
        with np.errstate(divide="ignore"):
            self.intensity_rel_error_ = 1.0 / np.sqrt(self.intensity_W_)
        self.component_counts_ = self.pixel_counts_.sum(axis=1)
        total = float(np.asarray(out["counts"], dtype=np.float64).sum())
        self.explained_counts_ratio_ = self.component_counts_ / total if total > 0 else np.zeros(k)
        self.unattributed_counts_ = float(out["unattributed"].sum())
        return dict(pixel_counts=self.pixel_counts_.T if self.hspy_comp else self.pixel_counts_, channel_counts=self.channel_counts_,
                    intensity_W=self.intensity_W_, model_intensity_W=self.model_intensity_W_, intensity_rel_error=self.intensity_rel_error_,
                    component_counts=self.component_counts_, explained_counts_ratio=self.explained_counts_ratio_,
                    unattributed_counts=self.unattributed_counts_)

    def assign_counts(self, X, seed=0, device=False):
        """The count image X split into k count images, one per component, that add up to X exactly
        (``espm_amd.attribution.assign`` on ``G_ @ W_`` and ``H_``): every single count goes to component j with probability
        d_cj h_jp / y.  By the Poisson splitting theorem each part is an honest noisy acquisition of its phase alone - integer
        counts that keep whatever the model missed - where ``inverse_transform`` gives only the smooth model of a phase.

        X is required (the fit's ``X_`` is not integer counts): 0 .. 65535, a host array or a device tensor, (channels, pixels), or
        (pixels, channels) with ``hspy_comp``.  Returns (k, *X.shape) in the dtype X was uploaded in (uint8 or uint16), a host array
        or with ``device=True`` a device tensor - k times the memory of X.  A function of (X, fit, seed) alone, bit for bit.
        Non-zero entries without a valid modelled rate (none, where the fit kept ``H_`` and ``W_`` above the ``log_shift`` floor) go to
        the first image, with a RuntimeWarning.  ``shard()``ed estimators raise NotImplementedError, estimators fitted by
        ``fit_binned`` ValueError, floating-point X TypeError - all before anything is uploaded."""
        import warnings

        from espm_amd import attribution
        check_is_fitted(self, "W_")
        if getattr(self, "_shard_group", None) is not None:
            raise NotImplementedError("assign_counts does not cover shard(): the split runs on one GPU")
        self._refuse_binned_X("assign_counts")
        D, H = self._model_counts()
        parts, info = attribution.assign(X, D, H, seed=seed, layout=self._layout(), device=device)
        if info["invalid"]:
            warnings.warn(f"assign_counts: {info['invalid']} non-zero entries have no valid modelled rate (not finite, or not above 0): "
                          "their counts are in the first component's image", RuntimeWarning, stacklevel=2)
        return parts

    # ---- line maps and region spectra: weighted sums of X and of the fitted model along one axis ------------------------------------
    def line_maps(self, lines, X=None):
        """Elemental line maps next to what the fit says about them (``espm_amd.marginals.line_maps`` on ``G_ @ W_`` and ``H_``):
        the counts in an energy window around an X-ray line, less a background interpolated between two side windows, with a Poisson
        error bar - exspy's ``get_lines_intensity``, on the channel windows the reference's own workflow is built on
        (``select_background_windows``, eds_spim.py:364-384) - and the modelled line with every component's share of it.

        ``lines``: a list of ``(integration, background)`` in half-open ranges of channel indices, ``background`` None or
        ``((l0, l1), (r0, r1))`` - ``marginals.line_weights`` has the rule.  Sets ``lines_`` (g, n): the weight vectors;
        ``line_net_`` (g, p): the measured net counts; ``line_net_std_`` (g, p): sqrt(sum u^2 x); ``line_model_`` (g, p):
        (U G_ W_) H_; ``line_components_`` (g, k, p): component i's share (U G_ W_)_qi H_ij.  Returns them as a dict (``lines``,
        ``net``, ``net_std``, ``model_net``, ``components``), the maps always (., p) whatever ``hspy_comp``.

        ``X`` as for ``pixel_diagnostics``: the fitted image in counts, (channels, pixels), or (pixels, channels) with ``hspy_comp``;
        ``X=None`` takes the fit's ``X_`` un-scaled, with the cost and the ``log_shift`` fill described there.  One pass over the
        lines' channels of X in fp64 on the current device, the model terms on the host: any number of components, every precision
        mode, ``shard()``ed estimators (every rank computes everything on its own device)."""
        from espm_amd import marginals
        check_is_fitted(self, "W_")
        X, layout = self._image_argument(X, "line_maps")
        D, H = self._model_counts()
        out = marginals.line_maps(X, lines, D, H, layout=layout)
        self.lines_, self.line_net_, self.line_net_std_ = out["weights"], out["net"], out["net_std"]
        self.line_model_, self.line_components_ = out["model_net"], out["components"]
        return dict(lines=self.lines_, net=self.line_net_, net_std=self.line_net_std_, model_net=self.line_model_,
                    components=self.line_components_)

    def region_spectra(self, regions, X=None):
        """The spectrum of every region of the image - measured, modelled and residual (``espm_amd.marginals.channel_spectra`` on
        ``G_ @ W_`` and ``H_``): what ``spectral_diagnostics`` gives for the whole image, per phase, where a residual peak that lives
        in one phase is not diluted by all the other pixels.

        ``regions``: an integer label map of the p pixels (any shape; negative labels belong to no region - e.g.
        ``H_.argmax(axis=0)``), or floating-point weights (L, p) (e.g. ``H_ / H_.sum(0)``: abundances as soft masks).  Sets
        ``region_counts_``, ``region_model_`` and ``region_deviance_``, each (n, L): sum_j v_j x, sum_j v_j Y and
        2 sum_j v_j (x ln(x / Y) - x + Y) with Y = max(G_ W_ H_, log_shift); and ``region_pixels_`` (L,): the sum of every
        region's weights (its number of pixels).  Returns them as a dict (``counts``, ``model``, ``deviance``, ``pixels``).

        ``X`` as for ``pixel_diagnostics``.  Computed in fp64 whatever the estimator's precision, on the current device (a
        ``shard()``ed estimator: every rank computes everything on its own device).  More than 8 components raise
        NotImplementedError, labels or weights that do not match the pixels ValueError - before anything is uploaded."""
        from espm_amd import marginals
        check_is_fitted(self, "W_")
        k, p = int(self.H_.shape[0]), int(self.H_.shape[1])
        if k > marginals.MAX_K:
            raise NotImplementedError(f"region_spectra: {k} components (the kernels are built for 1..{marginals.MAX_K})")
        R = np.asarray(regions)
        if R.dtype.kind in "iub":
            if R.size != p:
                raise ValueError(f"region_spectra: a label map of {R.size} pixels, the fitted H_ has {p}")
            V = marginals.label_weights(R)
        else:
            V = np.asarray(R, dtype=np.float64)
            if V.ndim != 2 or V.shape[1] != p:
                raise ValueError(f"region_spectra: weights of shape {V.shape}, the fitted H_ has {p} pixels (weights are (regions, {p}))")
        X, layout = self._image_argument(X, "region_spectra")
        D, H = self._model_counts()
        out = marginals.channel_spectra(X, V, D, H, log_shift=self.log_shift, layout=layout)
        self.region_counts_, self.region_model_, self.region_deviance_ = out["counts"], out["model"], out["deviance"]
        self.region_pixels_ = V.sum(axis=1)
        return dict(counts=self.region_counts_, model=self.region_model_, deviance=self.region_deviance_, pixels=self.region_pixels_)

    # ---- what the fit left in the residual: a missing phase, its spectrum and its map ----------------------------------------------
    def residual_components(self, n_vectors=4, X=None, n_null=0, seed=0):
        """Is a phase missing, and what does it look like?  The leading singular triplets of the Pearson residual matrix
        E = (X - Y) / sqrt(Y), Y = G_ W_ H_ (``espm_amd.residuals.svd``; no reference analogue).  For a correct Poisson model E is
        unit-variance noise and its top singular value sits near ``residual_edge_`` = sqrt(n) + sqrt(p); a missing phase is a value
        far above that, its left vector the residual spectrum and its right vector the map of where the phase sits - what
        ``deviance_`` (where the model fails) and ``bootstrap`` (how uncertain it is given that it is right) do not say.

        Sets ``residual_singular_values_`` (r,), ``residual_spectra_`` (n, r) - each with its largest-magnitude entry positive -,
        ``residual_maps_`` (r, p), ``residual_explained_`` (r,) = s^2 / ``residual_chi2_``, ``residual_chi2_`` (the total Pearson
        chi^2), ``residual_chi2_map_`` (p,), ``residual_edge_`` and ``residual_unmodelled_`` (entries with counts whose model is below
        ``log_shift``: they leave E).  Returns them as a dict (keys without the prefix and the underscore, with ``ritz_residuals``,
        ``n_iter`` and ``converged``); the maps are always (r, p) whatever ``hspy_comp``.  ``residual_spectra_[:, 0]`` clipped at 0 is
        a natural extra column of W for a refit with one more component.

        ``n_null >= 1``: the honest scale at EDS doses, where e is heavy-tailed and the analytic edge only a guide -
        ``residuals.null_singular_values``, the top singular value of ``n_null`` replicates (0 .. n_null - 1 under ``seed``) of the
        fitted model drawn on the device, each against the fitted model.  Sets ``residual_null_`` (n_null,), ``residual_pvalue_`` =
        (1 + #{null >= s_1}) / (n_null + 1) and ``residual_n_significant_``: the number of leading values above the largest null
        value.  The null is FRESH data against the generating model, not refitted to every replicate: the residual of the fitted
        image is in-sample and a fit takes some of the noise with it, so the top value of a right model sits a little BELOW its null
        and the calibration is conservative - a component flagged here is flagged with room to spare.

        ``n_vectors``: 1 .. 6.  ``X`` as for ``pixel_diagnostics``; ``X=None`` takes the fit's ``X_`` un-scaled, with the cost and the
        ``log_shift`` fill described there.  Computed in fp64 whatever the estimator's precision, on the current device; 1 .. 8
        components (NotImplementedError beyond).  Without a null a ``shard()``ed estimator computes everything on every rank's own
        device; with one the refusals of ``simulate`` apply (``shard()``: NotImplementedError, ``fit_binned``: ValueError) - all
        before anything is uploaded."""
        from espm_amd import residuals, sampling
        from espm_amd._image_args import check_seed
        check_is_fitted(self, "W_")
        k = int(self.H_.shape[0])
        if k > residuals.MAX_K:
            raise NotImplementedError(f"residual_components: {k} components (the kernels are built for 1..{residuals.MAX_K})")
        n, p = int(self.G_.shape[0]), int(self.H_.shape[1])
        residuals._check_iteration(n_vectors, 1e-10, 60, n, p)
        if isinstance(n_null, bool) or int(n_null) != n_null or int(n_null) < 0:
            raise ValueError(f"n_null must be a non-negative integer, not {n_null!r}")
        n_null, seed = int(n_null), check_seed(seed)
        if n_null:
            self._sampling_model("residual_components")
            sampling._check_replicate(0, n_null)
        X, layout = self._image_argument(X, "residual_components")
        D, H = self._model_counts()
        out = residuals.svd(X, D, H, n_vectors=n_vectors, log_shift=self.log_shift, layout=layout)
        self.residual_singular_values_, self.residual_spectra_, self.residual_maps_ = out["singular_values"], out["spectra"], out["maps"]
        self.residual_explained_, self.residual_chi2_, self.residual_chi2_map_ = out["explained"], out["chi2_total"], out["chi2_map"]
        self.residual_edge_, self.residual_unmodelled_ = out["edge"], out["unmodelled"]
        if n_null:
            null = residuals.null_singular_values(D, H, n_rep=n_null, seed=seed, log_shift=self.log_shift)
            cal = residuals.calibrate(out["singular_values"], null)
            self.residual_null_, self.residual_pvalue_, self.residual_n_significant_ = null, cal["pvalue"], cal["n_significant"]
            out = dict(out, null=null, pvalue=cal["pvalue"], n_significant=cal["n_significant"])
        return out

    # ---- is phase j in this pixel at all: per-pixel ML abundances and nested likelihood-ratio tests ---------------------------------
    def presence_maps(self, X=None, tol=1e-3, max_pass=None, method="em"):
        """Is phase j present in this pixel?  ``espm_amd.presence.presence`` on the fitted spectra ``G_ @ W_``, started at ``H_``: the
        Poisson maximum-likelihood abundances of every pixel given the spectra, and for every component the likelihood ratio between
        that fit and the pixel's best fit WITHOUT the component - the honest statistic where an abundance sits at or near zero and
        the Wald bar ``H_std_`` (which ignores active floors) means nothing.  No reference analogue.

        Sets ``H_ml_`` (k, p), oriented as ``H_``; ``deviance_ml_`` (p,); ``presence_lr_`` (k, p) = max(deviance without j -
        deviance_ml, 0), certified to within ``tol`` on either side; ``presence_pvalue_`` (k, p) = 1/2 erfc(sqrt(lr / 2)), the tail of
        the boundary mixture 1/2 chi2_0 + 1/2 chi2_1 - asymptotic, a guide at a few tens of counts per pixel -, 1 where lr = 0; and
        ``ml_converged_`` (bool), ``ml_gap_``, ``ml_n_pass_``, each (k + 1, p): row 0 the full fit, row 1 + j the fit without
        component j; and ``ml_method_``, the ``method`` of this call.  Returns dict(H_ml, deviance_ml, lr, pvalue, converged, gap, n_pass, unmodelled, nonfinite); with ``hspy_comp``
        the returned ``H_ml`` is (p, k), as ``fit_transform`` returns ``H_.T``; the maps stay (k, p).

        The ML is over h >= 0 alone: the regularisers of the fit (``mu``, ``lambda_L``) and ``simplex_H`` are NOT imposed.  A fit
        without ``simplex_H`` therefore has ``deviance_ml_ <= deviance_`` (+ tol) in every pixel.  Under ``simplex_H`` the per-pixel ML
        frees the pixel's scale: the fit's model is a sub-model of it, and ``H_ml_.sum(0)`` is a map of the per-pixel dose or thickness
        that the simplex model cannot express.  ``method="simplex"`` is the ML OF the fit's model instead: sum h = 1 in every pixel,
        the spectra carry the intensity, and the k reduced fits sum to 1 again (``presence.presence(method="simplex")``) - a test with
        no parameter per pixel that the fit did not have.  It needs an estimator with ``simplex_H=True`` (ValueError otherwise, before
        every other refusal) and at least two components; ``H_ml_`` then sums to 1 per pixel and ``ml_gap_`` is the Frank-Wolfe
        certificate.

        ``tol``: the certified gap, in deviance units, at which a pixel stops; ``max_pass``: the cap of a pixel's EM passes (None:
        ``presence.MAX_PASS``) - EM takes hundreds of passes, with tails of thousands, and pixels still running at the cap are False in
        ``ml_converged_``.  ``method``: "em" (the default: the rule defined bit for bit) or "newton" (the safeguarded Newton step of
        ``presence.ml_unmix``: the same certified statistic within ``tol``, tens of passes per pixel) or "simplex" (above), the one
        method for all k + 1 fits; anything else is a ValueError.  ``X`` as for ``pixel_diagnostics``; ``X=None`` takes the fit's ``X_`` un-scaled, with the cost and the
        ``log_shift`` fill described there (refused after ``fit_binned``).  Computed in fp64 whatever the estimator's precision, on the
        current device (a ``shard()``ed estimator: every rank computes all pixels on its own device); 1 .. 8 components
        (NotImplementedError beyond), all before anything is uploaded."""
        from espm_amd import presence
        if method == "simplex" and not self.simplex_H:
            raise ValueError("presence_maps: method='simplex' is the pixel model of a simplex_H fit, and this estimator has simplex_H=False")
        check_is_fitted(self, "W_")
        presence._check_method(method)
        k = int(self.H_.shape[0])
        if k > presence.MAX_K:
            raise NotImplementedError(f"presence_maps: {k} components (the kernels are built for 1..{presence.MAX_K})")
        X, layout = self._image_argument(X, "presence_maps")
        G, W, H = self._model_factors()
        D = W if G is None else G @ W
        out = presence.presence(X, D, H, tol=tol, max_pass=presence.MAX_PASS if max_pass is None else max_pass,
                                log_shift=self.log_shift, layout=layout, method=method)
        self.ml_method_ = method
        self.H_ml_, self.deviance_ml_ = out["H_ml"], out["deviance_ml"]
        self.presence_lr_, self.presence_pvalue_ = out["lr"], out["pvalue"]
        self.ml_converged_, self.ml_gap_, self.ml_n_pass_ = out["converged"], out["gap"], out["n_pass"]
        if self.hspy_comp:
            out = dict(out, H_ml=out["H_ml"].T)
        return out

    # ---- how much of phase j could be in this pixel: profile-likelihood intervals of the abundances -----------------------------------
    def abundance_intervals(self, level=0.95, X=None, components=None, tol=1e-3, lr_tol=1e-2, max_eval=None, simplex=False):
        """How much of phase j could be in this pixel?  ``espm_amd.presence.intervals`` on the fitted spectra ``G_ @ W_``, started at
        ``H_``: for every pixel and every requested component the PROFILE-LIKELIHOOD interval of the abundance - the values t whose
        best fit with h_j held at t lies within the chi2_1 quantile 2 erfinv(level)^2 of the pixel's best fit.  Where an abundance
        sits at or near zero (where the Wald bar ``H_std_`` means nothing) the interval starts at exactly 0 and ``H_upper_`` is an
        upper limit, the detection limit of the map; away from the boundary the two ends are an asymmetric error bar.
        ``presence_maps``' statistic is the same profile at the single point t = 0.  The interval is two-sided: a one-sided 95 %
        upper limit is ``H_upper_`` at ``level=0.90``.  No reference analogue.

        Sets ``H_lower_``, ``H_upper_`` (k, p), oriented as ``H_`` (NaN in rows not requested and for pixels that did not finish);
        ``H_interval_level_``; ``H_interval_converged_`` (bool) and ``H_interval_n_eval_`` (k, 2, p): [:, 0] the lower end, [:, 1] the
        upper; and ``H_ml_`` (k, p), ``deviance_ml_`` (p,), the full fit by the Newton rule.  Returns dict(H_ml, deviance_ml, lower,
        upper, level, threshold, converged, n_eval, n_pass, unmodelled, nonfinite); with ``hspy_comp`` the returned ``H_ml``,
        ``lower`` and ``upper`` are (p, k), as ``fit_transform`` returns ``H_.T``; the attributes stay (k, p).  The fitted
        attributes are not touched.

        What the interval is NOT: it holds the spectra ``G_ @ W_`` fixed (their own uncertainty is ``spectral_diagnostics``'); it
        imposes neither the regularisers of the fit (``mu``, ``lambda_L``) nor ``simplex_H``, as ``presence_maps`` does not; and it is
        ASYMPTOTIC - at a few tens of counts per pixel, and where other abundances sit on their boundaries, its coverage is a guide
        (``sampling`` / ``simulate`` draw the replicates a calibration would need).

        ``simplex=True``: the interval of a phase FRACTION under the fit's own pixel model, sum h = 1
        (``presence.intervals(simplex=True)``): 0 <= ``H_lower_`` <= ``H_ml_`` <= ``H_upper_`` <= 1, an upper end of exactly 1 where
        the pixel could be all phase j, and ``H_ml_`` the constrained fit.  It needs an estimator with ``simplex_H=True`` (ValueError
        otherwise, before every other refusal).  ``H_interval_simplex_`` (bool) records which of the two the attributes hold.  The
        spectra are still fixed, the regularisers still off, the level still asymptotic.

        ``level``: strictly between 0 and 1.  ``components``: the rows to compute (None: all).  ``tol``: the certified gap of every
        fit; ``lr_tol``: how close to the quantile an end's deviance difference must come; ``max_eval``: the cap of the pinned fits
        per end (None: 64).  ``X`` as for ``pixel_diagnostics``; ``X=None`` takes the fit's ``X_`` un-scaled, with the cost and the
        ``log_shift`` fill described there (refused after ``fit_binned``).  Computed in fp64 whatever the estimator's precision, on
        the current device (a ``shard()``ed estimator: every rank computes all pixels on its own device); 1 .. 8 components
        (NotImplementedError beyond), all before anything is uploaded."""
        from espm_amd import presence
        if simplex and not self.simplex_H:
            raise ValueError("abundance_intervals: simplex=True is the pixel model of a simplex_H fit, and this estimator has simplex_H=False")
        check_is_fitted(self, "W_")
        presence.threshold(level)
        k = int(self.H_.shape[0])
        if k > presence.MAX_K:
            raise NotImplementedError(f"abundance_intervals: {k} components (the kernels are built for 1..{presence.MAX_K})")
        if components is not None:
            presence._components(components, k)
        X, layout = self._image_argument(X, "abundance_intervals")
        G, W, H = self._model_factors()
        D = W if G is None else G @ W
        out = presence.intervals(X, D, H, level=level, components=components, tol=tol, lr_tol=lr_tol,
                                 max_eval=64 if max_eval is None else max_eval, log_shift=self.log_shift, layout=layout,
                                 simplex=bool(simplex))
        self.H_interval_simplex_ = bool(simplex)
        self.H_lower_, self.H_upper_, self.H_interval_level_ = out["lower"], out["upper"], out["level"]
        self.H_interval_converged_, self.H_interval_n_eval_ = out["converged"], out["n_eval"]
        self.H_ml_, self.deviance_ml_ = out["H_ml"], out["deviance_ml"]
        if self.hspy_comp:
            out = dict(out, H_ml=out["H_ml"].T, lower=out["lower"].T, upper=out["upper"].T)
        return out

    # ---- is element e in phase j at all: the ML of W given H and nested likelihood-ratio tests on its entries --------------------------
    def element_presence(self, X=None, entries=None, tol=1e-3, max_pass=None):
        """Is element e present in phase j?  ``espm_amd.spectra_ml.presence`` on the dictionary or physics model ``G_`` and the fitted
        abundances ``H_``, started at ``W_``: the Poisson maximum-likelihood W >= 0 given the abundances, and for every tested entry
        the likelihood ratio between that fit and the best fit WITH THE ENTRY HELD AT ZERO - the honest statistic where a
        concentration sits at or near zero (a trace element) and the Wald bar ``W_std_`` (which ignores active floors) means nothing.
        No reference analogue.

        Sets, all oriented as ``W_``: ``W_ml_`` (m, k) and ``W_deviance_ml_``, the full fit; ``W_presence_lr_`` (m, k) =
        max(deviance without (e, j) - deviance_ml, 0) and ``W_presence_pvalue_`` (m, k) = 1/2 erfc(sqrt(lr / 2)), the tail of the
        boundary mixture 1/2 chi2_0 + 1/2 chi2_1 (asymptotic), both NaN for entries that were not tested; ``W_presence_entries_``
        (E, 2), the tested (element, component) pairs; and ``W_ml_converged_`` (bool), ``W_ml_gap_``, ``W_ml_n_pass_``, each
        (1 + E,): the full fit, then the fit without each tested entry.  Returns ``spectra_ml.presence``'s dict.

        The ML is over W >= 0 with ``H_`` held: ``mu``, ``simplex_W`` and the floors of the fit are NOT imposed, so
        ``W_deviance_ml_`` is at most the fit's own deviance (+ tol).  Entries that ``fixed_W`` imposes at 0 leave the free set: their
        ``W_ml_`` is 0 and their lr NaN.  Entries imposed at a positive value, an identity G (``G=None``: the problem decouples per
        channel) and more than 8 components raise NotImplementedError; m k is at most 2048.  Every refusal happens before anything
        is uploaded.

        ``entries``: (E, 2) index pairs into ``W_`` to test (None: every free entry the model sees); ``tol``: the certified gap, in
        deviance units, at which a fit stops; ``max_pass``: the cap of a fit's passes over the image (None:
        ``spectra_ml.MAX_PASS``).  ``X`` as for ``pixel_diagnostics``; ``X=None`` takes the fit's ``X_`` un-scaled, with the cost and
        the ``log_shift`` fill described there (refused after ``fit_binned``).  Computed in fp64 whatever the estimator's precision,
        on the current device (a ``shard()``ed estimator: every rank computes everything on its own device)."""
        from espm_amd import spectra_ml
        check_is_fitted(self, "W_")
        k = int(self.H_.shape[0])
        if k > spectra_ml.MAX_K:
            raise NotImplementedError(f"element_presence: {k} components (the kernel is built for 1..{spectra_ml.MAX_K})")
        G, W, H = self._model_factors()
        if G is None:
            raise NotImplementedError("element_presence: needs a dictionary or physics model G (with an identity G the problem "
                                      "decouples per channel)")
        free = None
        if self.fixed_W is not None:
            fixed = np.asarray(self.fixed_W)
            if (fixed > 0).any():
                raise NotImplementedError("element_presence: fixed_W entries imposed at a positive value are not covered")
            free = ~(fixed == 0)
        X, layout = self._image_argument(X, "element_presence")
        out = spectra_ml.presence(X, G, H, W0=W, free=free, entries=entries, tol=tol,
                                  max_pass=spectra_ml.MAX_PASS if max_pass is None else max_pass, log_shift=self.log_shift, layout=layout)
        self.W_ml_, self.W_deviance_ml_ = out["W_ml"], out["deviance_ml"]
        self.W_presence_lr_, self.W_presence_pvalue_, self.W_presence_entries_ = out["lr"], out["pvalue"], out["entries"]
        self.W_ml_converged_, self.W_ml_gap_, self.W_ml_n_pass_ = out["converged"], out["gap"], out["n_pass"]
        return out

    # ---- how much of element e could be in phase j: profile-likelihood intervals of the entries of W ----------------------------------
    def concentration_intervals(self, level=0.95, X=None, entries=None, tol=1e-3, lr_tol=1e-2, max_eval=None, max_pass=None):
        """How much of element e could be in phase j?  ``espm_amd.spectra_ml.intervals`` on the dictionary or physics model ``G_``
        and the fitted abundances ``H_``, started at ``W_``: for every tested entry the PROFILE-LIKELIHOOD interval of the
        concentration - the values t whose best fit with W_ej held at t lies within the chi2_1 quantile 2 erfinv(level)^2 of the best
        fit.  What an analyst reports: "0.8 (0.5 - 1.2)" away from the boundary, and for a trace element, where the interval starts
        at exactly 0, the upper limit "< 0.05 at 95 %" - where the Wald bar ``W_std_`` means nothing and ``element_presence`` says only
        "present or not".  The interval is two-sided: a one-sided 95 % upper limit is ``W_upper_`` at ``level=0.90``.  No reference
        analogue.

        Sets, oriented as ``W_``: ``W_lower_``, ``W_upper_`` (m, k), NaN for entries that were not tested and for ends that were not
        found; ``W_interval_level_``; ``W_interval_entries_`` (E, 2), the tested (element, component) pairs;
        ``W_interval_converged_`` (bool) and ``W_interval_n_eval_`` (E, 2): [:, 0] the lower end, [:, 1] the upper; and ``W_ml_``
        (m, k), ``W_deviance_ml_``, the full fit.  Returns ``spectra_ml.intervals``'s dict.  The fitted attributes are not touched.

        What the interval is NOT: it holds ``H_`` fixed (the abundances' own uncertainty is not in it); it is the interval of W_ej
        itself, not of a normalised concentration W_ej / sum_e W_ej; ``mu``, ``simplex_W`` and the floors of the fit are NOT imposed;
        it is ASYMPTOTIC; and it runs on one GPU.  Set-up and refusals are ``element_presence``'s: entries that ``fixed_W`` imposes at
        0 leave the free set (their ends are NaN, and they are not tested); entries imposed at a positive value, an identity G
        (``G=None``) and more than 8 components raise NotImplementedError; m k is at most 2048; refused after ``fit_binned``.  Every
        refusal happens before anything is uploaded.

        ``level``: strictly between 0 and 1.  ``entries``: (E, 2) index pairs into ``W_`` (None: every free entry the model sees).
        ``tol``: the certified gap of every fit; ``lr_tol``: how close to the quantile an end's deviance difference must come;
        ``max_eval``: the cap of the pinned fits per end (None: 64); ``max_pass``: the cap of a fit's passes over the image (None:
        ``spectra_ml.MAX_PASS_PINNED``).  ``X`` as for ``pixel_diagnostics``.  Computed in fp64 whatever the estimator's precision, on
        the current device."""
        from espm_amd import presence, spectra_ml
        check_is_fitted(self, "W_")
        presence.threshold(level)
        k = int(self.H_.shape[0])
        if k > spectra_ml.MAX_K:
            raise NotImplementedError(f"concentration_intervals: {k} components (the kernel is built for 1..{spectra_ml.MAX_K})")
        G, W, H = self._model_factors()
        if G is None:
            raise NotImplementedError("concentration_intervals: needs a dictionary or physics model G (with an identity G the problem "
                                      "decouples per channel)")
        free = None
        if self.fixed_W is not None:
            fixed = np.asarray(self.fixed_W)
            if (fixed > 0).any():
                raise NotImplementedError("concentration_intervals: fixed_W entries imposed at a positive value are not covered")
            free = ~(fixed == 0)
        X, layout = self._image_argument(X, "concentration_intervals")
        out = spectra_ml.intervals(X, G, H, W0=W, free=free, entries=entries, level=level, tol=tol, lr_tol=lr_tol,
                                   max_eval=64 if max_eval is None else max_eval,
                                   max_pass=spectra_ml.MAX_PASS_PINNED if max_pass is None else max_pass, log_shift=self.log_shift,
                                   layout=layout)
        self.W_lower_, self.W_upper_, self.W_interval_level_ = out["lower"], out["upper"], out["level"]
        self.W_interval_entries_, self.W_interval_converged_, self.W_interval_n_eval_ = out["entries"], out["converged"], out["n_eval"]
        self.W_ml_, self.W_deviance_ml_ = out["W_ml"], out["deviance_ml"]
        return out

    # ---- is this line of phase j real, and how much could be under it: free spectra given H, channel by channel -----------------------
    def _channel_ml_refusal(self, who):
        """The refusals ``spectrum_presence`` and ``spectrum_intervals`` share, raised before anything is uploaded.  Returns k."""
        from espm_amd import channel_ml
        check_is_fitted(self, "W_")
        if getattr(self, "_shard_group", None) is not None:
            raise NotImplementedError(f"{who} does not cover shard(): the channel fits run on one GPU")
        k = int(self.H_.shape[0])
        if k > channel_ml.MAX_K:
            raise NotImplementedError(f"{who}: {k} components (the kernels are built for 1..{channel_ml.MAX_K})")
        return k

    def spectrum_presence(self, X=None, windows=None, tol=1e-3, max_pass=None):
        """Is this line of phase j real?  ``espm_amd.channel_ml.presence`` on the fitted abundances ``H_``, started at the fitted
        spectra D = ``W_`` (identity G) or ``G_ @ W_``: the Poisson maximum-likelihood spectra given the abundances with NO dictionary
        behind them - every channel a problem of its own - and for every channel and component the likelihood ratio between that fit
        and the channel's best fit WITHOUT the component.  It is the test for a fit with ``G=None``, where most channels of a phase
        spectrum sit at or near zero and the Wald bar ``W_std_`` means nothing; with a dictionary it is the dictionary-free fit to
        hold ``G_ @ W_`` against - a line the element list missed shows in ``D_excess_deviance_``.  No reference analogue.

        Sets ``D_ml_`` (n, k) and ``D_deviance_ml_`` (n,), the free fit; ``D_excess_deviance_`` (n,) = the deviance of every channel at
        the fitted spectra less ``D_deviance_ml_``: what the fitted (or dictionary-bound) spectra lose against free spectra, at least
        -tol; ``D_presence_lr_`` (n, k) = max(deviance without j - deviance_ml, 0), exactly 0 where ``D_ml_`` is 0, and
        ``D_presence_pvalue_`` (n, k), its tail under 1/2 chi2_0 + 1/2 chi2_1 (asymptotic); ``D_ml_converged_`` (k + 1, n): row 0 the
        full fit, row 1 + j the fit without j.  With ``windows`` - half-open ranges (lo, hi) of channel indices, one per line - also
        ``line_presence_lr_`` and ``line_presence_pvalue_`` (windows, k): the test of "phase j has nothing in the whole window"
        (``channel_ml.line_presence``: given ``H_`` the channels are independent and their ratios add).  Returns
        ``channel_ml.presence``'s dict, with ``excess_deviance`` and, with ``windows``, ``line_lr`` and ``line_pvalue``.

        The ML is over D >= 0 with ``H_`` held: ``mu``, ``simplex_W`` and the floors of the fit are NOT imposed, and the uncertainty of
        ``H_`` is not in the statistic.  At least 2 and at most 8 components (ValueError, NotImplementedError); ``shard()``ed
        estimators raise NotImplementedError; ``windows`` are checked against the channels - all before anything is uploaded.

        ``tol``: the certified gap, in deviance units, at which a channel stops; ``max_pass``: the cap of a fit's passes over the
        image (None: ``channel_ml.MAX_PASS``).  ``X`` as for ``pixel_diagnostics``; ``X=None`` takes the fit's ``X_`` un-scaled, with
        the cost and the ``log_shift`` fill described there (refused after ``fit_binned``).  Computed in fp64 whatever the estimator's
        precision, on the current device."""
        from espm_amd import channel_ml, marginals
        k = self._channel_ml_refusal("spectrum_presence")
        if k < 2:
            raise ValueError("spectrum_presence: one component (without it the model is empty: nothing to test)")
        if windows is not None:
            windows = list(windows)
            marginals.window_weights(int(self.G_.shape[0]), windows)
        X, layout = self._image_argument(X, "spectrum_presence")
        D, H = self._model_counts()
        out = channel_ml.presence(X, H, D0=D, tol=tol, max_pass=channel_ml.MAX_PASS if max_pass is None else max_pass,
                                  log_shift=self.log_shift, layout=layout)
        out = dict(out, excess_deviance=out["deviance_start"] - out["deviance_ml"])
        self.D_ml_, self.D_deviance_ml_, self.D_excess_deviance_ = out["D_ml"], out["deviance_ml"], out["excess_deviance"]
        self.D_presence_lr_, self.D_presence_pvalue_, self.D_ml_converged_ = out["lr"], out["pvalue"], out["converged"]
        if windows is not None:
            line = channel_ml.line_presence(out["lr"], windows)
            self.line_presence_lr_, self.line_presence_pvalue_ = line["lr"], line["pvalue"]
            out = dict(out, line_lr=line["lr"], line_pvalue=line["pvalue"])
        return out

    def spectrum_intervals(self, level=0.95, X=None, components=None, tol=1e-3, lr_tol=1e-2, max_eval=None, max_pass=None):
        """How much could be under this peak at most?  ``espm_amd.channel_ml.intervals`` on the fitted abundances ``H_``, started at
        the fitted spectra D = ``W_`` (identity G) or ``G_ @ W_``: for every channel and every requested component the
        PROFILE-LIKELIHOOD band of the spectrum - the values t whose best fit with d_cj held at t lies within the chi2_1 quantile
        2 erfinv(level)^2 of the channel's best fit with free spectra.  Where the spectrum sits at or near zero the band starts at
        exactly 0 and ``D_upper_`` is an upper limit; on a peak the two ends are an asymmetric error bar.  ``spectrum_presence``'s
        statistic is the same profile at the single point t = 0.  Two-sided: a one-sided 95 % upper limit is ``D_upper_`` at
        ``level=0.90``.  No reference analogue.

        Sets ``D_lower_``, ``D_upper_`` (n, k) (NaN in columns not requested and for channels that did not finish);
        ``D_interval_level_``; ``D_interval_converged_`` (bool) and ``D_interval_n_eval_`` (k, 2, n): [:, 0] the lower end, [:, 1] the
        upper; and ``D_ml_`` (n, k), ``D_deviance_ml_`` (n,), the free fit.  Returns ``channel_ml.intervals``'s dict.  The fitted
        attributes are not touched.

        What the band is NOT: it holds ``H_`` fixed (the abundances' own uncertainty is not in it); ``mu``, ``simplex_W`` and the
        floors of the fit are NOT imposed; it is ASYMPTOTIC in the counts of a channel; and it runs on one GPU.  1 .. 8 components
        (NotImplementedError beyond); ``shard()``ed estimators raise NotImplementedError - before anything is uploaded.

        ``level``: strictly between 0 and 1.  ``components``: the columns to compute (None: all).  ``tol``: the certified gap of
        every fit; ``lr_tol``: how close to the quantile an end's deviance difference must come; ``max_eval``: the cap of the pinned
        fits per end (None: 64); ``max_pass``: the cap of a fit's passes over the image (None: ``channel_ml.MAX_PASS``).  ``X`` as for
        ``pixel_diagnostics`` (``X=None`` is refused after ``fit_binned``).  Computed in fp64 whatever the estimator's precision, on
        the current device."""
        from espm_amd import channel_ml, presence
        k = self._channel_ml_refusal("spectrum_intervals")
        presence.threshold(level)
        if components is not None:
            presence._components(components, k)
        X, layout = self._image_argument(X, "spectrum_intervals")
        D, H = self._model_counts()
        out = channel_ml.intervals(X, H, D0=D, level=level, components=components, tol=tol, lr_tol=lr_tol,
                                   max_eval=64 if max_eval is None else max_eval,
                                   max_pass=channel_ml.MAX_PASS if max_pass is None else max_pass, log_shift=self.log_shift, layout=layout)
        self.D_lower_, self.D_upper_, self.D_interval_level_ = out["lower"], out["upper"], out["level"]
        self.D_interval_converged_, self.D_interval_n_eval_ = out["converged"], out["n_eval"]
        self.D_ml_, self.D_deviance_ml_ = out["D_ml"], out["deviance_ml"]
        return out

    # ---- draws from the fitted model: a simulated image, a scale for the deviance map, the parametric bootstrap -------------------
    def _sampling_model(self, who):
        """(D, H): the fitted model ``G_ @ W_`` (n, k) and ``H_`` (k, p) in counts, in fp64, after the refusals of ``simulate``,
        ``calibrate_deviance`` and ``bootstrap`` - all raised before anything is uploaded."""
        from espm_amd import sampling
        check_is_fitted(self, "W_")
        if getattr(self, "_shard_group", None) is not None:
            raise NotImplementedError(f"{who} does not cover shard(): the draws run on one GPU")
        if self._fitted_binned():
            raise ValueError(f"{who}: this estimator was fitted by fit_binned with bin {self.bin_}: its fit is a coarse fit and an "
                             "H-only fit, which a draw from G_ W_ H_ does not stand for")
        k = int(self.H_.shape[0])
        if k > sampling.MAX_K:
            raise NotImplementedError(f"{who}: {k} components (the sampling kernels are built for 1..{sampling.MAX_K})")
        return self._model_counts()

    def simulate(self, seed=0, replicate=0, device=False):
        """A count image drawn from the fitted model: replicate ``replicate`` (0 .. 2^32 - 2) of ``G_ @ W_``, ``H_`` under ``seed``
        (0 .. 2^64 - 1) by the rule of ``espm_amd.sampling`` - X* ~ Poisson(G_ W_ H_) entry by entry, a function of (model, seed,
        replicate) alone, bit for bit.  The reference draws its synthetic images with ``np.random.poisson`` on the host
        (datasets/base.py:68).

        Returns uint16 counts, (channels, pixels), or (pixels, channels) with ``hspy_comp`` - the orientation ``fit`` takes - as a
        host array, or with ``device=True`` a device tensor.  The model is in count units whatever ``normalize`` was (``W_`` is the
        un-normalised one, as for ``pixel_diagnostics``).  ValueError if any entry saturated (a rate above 65535, or a draw above
        it).  ``shard()``ed estimators raise NotImplementedError, estimators fitted by ``fit_binned`` ValueError, before anything is
        uploaded."""
        from espm_amd import sampling
        D, H = self._sampling_model("simulate")
        X, info = sampling.sample(D, H, seed=seed, replicate=replicate, dtype=np.uint16, layout=self._layout(), device=device)
        if info["saturated"] or info["invalid"]:
            raise ValueError(f"simulate: {info['saturated']} entries saturated the 16-bit counts and {info['invalid']} had no valid rate")
        return X

    def calibrate_deviance(self, X=None, n_rep=100, seed=0):
        """The deviance map on the scale of its own null distribution.  At EDS doses (a fraction of a count to a few counts per entry)
        the Poisson deviance of a pixel is far from chi-square, so ``deviance_`` alone cannot say whether a pixel is badly fitted or
        merely faint.  Runs ``pixel_diagnostics(X)`` for ``deviance_``, then ``sampling.null_deviance`` - the deviance of ``n_rep``
        replicates (0 .. n_rep - 1 under ``seed``) of the fitted model against the fitted model, on the device, none of them stored -
        and ``sampling.calibrate``.  Sets, each (p,): ``deviance_null_mean_``, ``deviance_null_std_`` (ddof = 1), ``deviance_z_`` =
        (deviance_ - mean) / std and ``deviance_pvalue_`` = (1 + #{r : null_r >= deviance_}) / (n_rep + 1); and ``deviance_null_rep_``,
        the number of replicates.  Returns them as a dict with ``deviance``.

        The null is FRESH data against the generating model, not refitted to every replicate: the deviance of the fitted image is
        in-sample and sits about k (the degrees of freedom a pixel's abundances took) lower than a fresh draw's, so the calibration is
        conservative - a pixel flagged here is flagged with room to spare.

        ``X`` as for ``pixel_diagnostics``; 1 .. 8 components, the diagnostics' limit; at least 2 replicates.  Refusals as for
        ``simulate``, before anything is uploaded."""
        from espm_amd import sampling
        from espm_amd._image_args import check_seed
        D, H = self._sampling_model("calibrate_deviance")
        n_rep = sampling._check_n_rep(n_rep)
        if n_rep < 2:
            raise ValueError("calibrate_deviance needs at least two replicates (the null standard deviation has ddof = 1)")
        check_seed(seed)
        self.pixel_diagnostics(X)
        null = sampling.null_deviance(D, H, n_rep=n_rep, seed=seed, replicate0=0, log_shift=self.log_shift)
        cal = sampling.calibrate(self.deviance_, null)
        self.deviance_null_mean_, self.deviance_null_std_ = cal["null_mean"], cal["null_std"]
        self.deviance_z_, self.deviance_pvalue_, self.deviance_null_rep_ = cal["z"], cal["pvalue"], n_rep
        return dict(deviance=self.deviance_, null_mean=cal["null_mean"], null_std=cal["null_std"], z=cal["z"], pvalue=cal["pvalue"])

    def _bootstrap_start(self):
        """(W, H) a refit of a replicate starts from: the fit itself - under ``normalize`` with W in the normalised units the fit
        iterates in (``W_`` is divided by ``norm_factor_`` at the end of a fit)."""
        W = np.asarray(self.W_)
        return (W * self.norm_factor_ if self.normalize else W), np.asarray(self.H_)

    def _bootstrap_copy(self, max_iter=None):
        """An unfitted estimator with this one's parameters (``sklearn.base.clone``), the same G, ``shape_2d``, ``fixed_W`` /
        ``fixed_H`` objects and precision mode."""
        from sklearn.base import clone
        boot = clone(self)
        boot.G, boot.shape_2d, boot.fixed_W, boot.fixed_H = self.G, self.shape_2d, self.fixed_W, self.fixed_H
        if self._fp64():
            boot.set_precision("fp64")
        if max_iter is not None:
            boot.max_iter = int(max_iter)
        return boot

    def bootstrap(self, n_boot=20, seed=0, max_iter=None, return_samples=False):
        """Parametric bootstrap of the fit AS IT WAS RUN: for r = 0 .. n_boot - 1, replicate r of the fitted model is drawn on the
        device (``simulate(seed, r)``) and fitted by a copy of this estimator - ``sklearn.base.clone`` of its parameters with the same
        G, ``shape_2d``, ``fixed_W`` / ``fixed_H`` and precision mode - warm-started at the fit (``fit_transform(X*, W=W_, H=H_)``,
        W in the units the fit iterates in; ``max_iter``: the copies' limit, by default the estimator's own).  The spread of the
        refits is the error bar of W and H TOGETHER, with ``mu``, ``lambda_L``, the simplex and the floors in force - what the
        Cramer-Rao bounds ``H_std_`` (given the spectra) and ``W_std_`` (given the abundances) leave out.  It does not include the
        bias of the fit, the error of the model itself (a missing phase), or starts other than the fit; with few iterations it is
        the spread after that many iterations.  The warm start keeps the components' order: no matching step.

        Sets ``W_boot_mean_``, ``W_boot_std_`` (the shape of ``W_``), ``H_boot_mean_``, ``H_boot_std_`` (k, p) and ``D_boot_std_``
        (n, k: of the spectra ``G_ @ W_``) - means and standard deviations (ddof = 1) over the replicates, accumulated in fp64
        (Welford) - and ``n_boot_``, ``boot_seed_``.  No fitted attribute of the estimator itself changes.  Returns them as a dict;
        with ``return_samples=True`` the dict also holds ``W_samples`` (n_boot, ...) and ``H_samples`` (n_boot, k, p) for
        percentile intervals.  At least 2 replicates; refusals as for ``simulate``, before anything is uploaded."""
        from espm_amd import sampling
        from espm_amd._image_args import check_seed
        D, H = self._sampling_model("bootstrap")
        n_boot, seed = sampling._check_n_rep(n_boot), check_seed(seed)
        if n_boot < 2:
            raise ValueError("bootstrap needs at least two replicates (the standard deviations have ddof = 1)")
        sampling._check_replicate(0, n_boot)
        D, H = sampling._model(D, H)
        W0, H0 = self._bootstrap_start()
        layout = self._layout()
        Dd, Hd, dev = sampling._upload(D, H)
        stats = [None, None, None]   # (mean, M2) of W, H, G W
        samples = ([], []) if return_samples else None
        for r in range(n_boot):
            Xr, saturated, invalid = sampling._draw(Dd, Hd, dev, seed, r, np.dtype(np.uint16), layout)
            if saturated or invalid:
                raise ValueError(f"bootstrap: replicate {r} has {saturated} saturated entries and {invalid} without a valid rate")
            boot = self._bootstrap_copy(max_iter)
            boot.fit_transform(self._counts_for_fit(Xr.cpu().numpy()), W=W0.copy(), H=H0.copy())
            Wr, Hr = np.asarray(boot.W_, dtype=np.float64), np.asarray(boot.H_, dtype=np.float64)
            for i, v in enumerate((Wr, Hr, Wr if boot._identity_G else np.asarray(boot.G_, dtype=np.float64) @ Wr)):
                if stats[i] is None:
                    stats[i] = [v.copy(), np.zeros_like(v)]
                else:
                    delta = v - stats[i][0]
                    stats[i][0] += delta / (r + 1)
                    stats[i][1] += delta * (v - stats[i][0])
            if return_samples:
                samples[0].append(Wr), samples[1].append(Hr)
        std = [np.sqrt(m2 / (n_boot - 1)) for _, m2 in stats]
        self.W_boot_mean_, self.W_boot_std_ = stats[0][0], std[0]
        self.H_boot_mean_, self.H_boot_std_ = stats[1][0], std[1]
        self.D_boot_std_ = std[2]
        self.n_boot_, self.boot_seed_ = n_boot, seed
        out = dict(W_mean=self.W_boot_mean_, W_std=self.W_boot_std_, H_mean=self.H_boot_mean_, H_std=self.H_boot_std_, D_std=self.D_boot_std_)
        if return_samples:
            out.update(W_samples=np.stack(samples[0]), H_samples=np.stack(samples[1]))
        return out
