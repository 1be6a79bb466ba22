"""sklearn-style NMF estimator base with the reference's surface (espm/estimators/base.py:20-529).

The fit loop of the reference (base.py:313-394) calls ``_iteration`` + ``loss`` on numpy arrays
once per multiplicative-update iteration.  Here the loop drives a device engine
(:class:`espm_amd.engine.MUEngine`): X, W, H stay in HBM, every iteration is a short chain of HIP
kernels, and the loss of a state is produced by the H-step that starts the NEXT iteration (it
forms the same G W H), so the reference's per-iteration bookkeeping costs no extra pass over X.
Stop rules, attribute names, printed messages and return conventions follow the reference.

This file holds the fit, ``unmix`` and their stages, ``loss``, the engine plumbing, ``L_``, ``get_losses`` and truth tracking.  What is done
with a fit - ``fit_binned``, ``fit_split``, the diagnostics, count attribution, draws from the model - lives next door in analysis.py
(``_FitAnalysis``, a mixin of ``NMFEstimator``).
"""
from __future__ import annotations

import os
import time
from abc import ABC, abstractmethod

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils.metaestimators import available_if
from sklearn.utils.validation import check_is_fitted, validate_data

from espm_amd.conf import log_shift
from espm_amd.estimators import ingest
from espm_amd.estimators.analysis import _FitAnalysis
from espm_amd.estimators.ingest import _DEVICE_PREP_MIN_SIZE, _HostCopy  # noqa: F401 - (their names before ingest.py, kept importable)
from espm_amd.estimators.updates import initialize_algorithms
from espm_amd.sharding import FitShard as _Shard   # (its name while it lived here, kept importable)
from espm_amd.utils import create_laplacian_matrix, identity_laplacian, rescaled_DH


def normalization_factor(X, nc):
    """espm/estimators/base.py:16-18."""
    m = np.mean(X)
    return nc / (m * X.shape[0])


def _is_physical_model(G):
    return G is not None and not isinstance(G, np.ndarray) and hasattr(G, "NMF_update")


def stop_message(rel_W, rel_H, eval_before, eval_after, eval_init, tol):
    """The stop rules of the reference's loop (base.py:354-378) in its order - relative change of W and H, relative change of the loss, NaN,
    a loss that went up - with the message the reference prints, or None while none of them holds.  (The iteration limit, and who prints,
    are the loop's.)"""
    decrease = eval_before - eval_after
    if max(rel_H, rel_W) < tol:
        return "exits because of relative change rel_A {} and rel_P {} < tol ".format(rel_H, rel_W)
    if abs(decrease / eval_init) < tol:
        return "exits because of relative change < tol: {}".format(decrease / eval_init)
    if np.isnan(eval_after):
        return "exit because of the presence of NaN"
    if decrease < 0:
        return "exit because of negative decrease {}: {}, {}".format(decrease, eval_before, eval_after)
    return None


def _rows_are_pixels(est):
    return bool(est.hspy_comp)


class _PixelTransform:
    """``transform`` of an estimator whose rows are pixels (``hspy_comp=True``: X is (pixels, channels), what hyperspy's decomposition
    hands over and what its contract - "fit() and transform()" - asks for).  There scikit-learn's meaning of ``transform`` and the H-only
    fit coincide: samples in, one row of abundances per sample out, ``fit_transform`` returning the same kind of array (H.T).  With
    ``hspy_comp=False`` the rows of X are channels and ``fit_transform`` returns G W, one row per CHANNEL: a ``transform`` that
    returned H there would break scikit-learn's transformer contract (``transform(X)`` ~ ``fit_transform(X)``, same number of rows,
    the column count of ``fit`` enforced - the pixel count, which new data need not share), so the method is not available there
    (``hasattr`` is False, scikit-learn's ``available_if``) and the same computation is ``unmix``.

    A mixin of its own, ahead of TransformerMixin: that class wraps the ``transform`` it finds in a subclass's own namespace for
    ``set_output``, which would replace the conditional descriptor with a plain function."""

    @available_if(_rows_are_pixels)
    def transform(self, X, H=None, shape_2d=None):
        """``unmix(X, H, shape_2d)`` for X (pixels, channels): returns H.T, (pixels, components), as ``fit_transform`` does."""
        return self.unmix(X, H=H, shape_2d=shape_2d)


class NMFEstimator(ABC, _PixelTransform, _FitAnalysis, TransformerMixin, BaseEstimator):
    """Abstract NMF estimator, X (n, p) ~ G (n, m) W (m, k) H (k, p); parameters and attributes as in
    espm/estimators/base.py:68-152."""

    loss_names_ = ["KL_div_loss"]
    const_KL_ = None

    def __init__(self, n_components=2, init=None, tol=1e-4, max_iter=200, random_state=None, verbose=1, debug=False,
                 l2=False, G=None, shape_2d=None, normalize=False, log_shift=log_shift, eval_print=10, true_D=None,
                 true_H=None, fixed_H=None, fixed_W=None, hspy_comp=False, no_stop_criterion=False, simplex_H=False,
                 simplex_W=True):
        self.n_components = n_components
        self.init = init
        self.tol = tol
        self.max_iter = max_iter
        self.random_state = random_state
        self.verbose = verbose
        self.log_shift = log_shift
        self.debug = debug
        self.l2 = l2
        self.G = G
        self.shape_2d = shape_2d
        self.eval_print = eval_print
        self.true_D = true_D
        self.true_H = true_H
        self.fixed_H = fixed_H
        self.fixed_W = fixed_W
        self.hspy_comp = hspy_comp
        self.normalize = normalize
        self.no_stop_criterion = no_stop_criterion
        self.simplex_H = simplex_H
        self.simplex_W = simplex_W

    def __sklearn_tags__(self):
        tags = super().__sklearn_tags__()
        tags.input_tags.positive_only = True
        return tags

    def _more_tags(self):
        return {"requires_positive_X": True}

    def __getstate__(self):
        state = super().__getstate__()
        state = dict(state)
        for key in ("_engine", "_truth_engine", "_shard_group", "_shard"):  # device buffers / ctypes pointers / process groups are not picklable
            state.pop(key, None)
        return state

    # ---- one fit over the GPUs of a node ----------------------------------------------------------------
    def shard(self, group):
        """Run the fits of this estimator sharded by image rows over the ranks of ``group`` (a ``torch.distributed`` process
        group with one GPU per rank; ``None`` switches it off).  Every rank calls ``fit`` / ``fit_transform`` with the same
        arguments - the same script under ``torchrun`` - and gets the same results: W replicated (bit-identical across the
        ranks), H and the returned arrays assembled from the ranks' blocks.  No reference analogue.
        Returns self."""
        self._shard_group = group
        return self

    # ---- arithmetic precision of the fits --------------------------------------------------------------
    def set_precision(self, mode):
        """Arithmetic of the fits: ``"fp32"`` (the default: fp32 kernels, fp64 loss sums) or ``"fp64"`` (every array and operation
        in fp64, with the reference's simplex bisection and its global stop, dicotomy.py:111-173 - the mode that follows the
        reference's trajectories, and its ``n_iter_``, at a small ``tol``).  Not a constructor argument: ``get_params()`` stays the
        reference's.  Scope of ``"fp64"``: algo="log_surrogate" without linesearch, l2=False, no true_D / true_H, one GPU (no
        ``shard()``), 1..8 components; anything else raises NotImplementedError from ``fit``.  Returns self."""
        if mode not in ("fp32", "fp64"):
            raise ValueError(f"precision must be 'fp32' or 'fp64', got {mode!r}")
        self._precision = mode
        return self

    def _fp64(self):
        return getattr(self, "_precision", "fp32") == "fp64"

    def _fp64_refusal(self):
        """Why a fit of this configuration cannot run in fp64 mode, or None."""
        from espm_amd._lib import F64_MAX_K
        if getattr(self, "algo", "log_surrogate") != "log_surrogate":
            return f"algo={self.algo!r} (fp64 mode: algo='log_surrogate' only)"
        if getattr(self, "linesearch", False):
            return "linesearch=True"
        if self.l2:
            return "l2=True"
        if self.true_D is not None or self.true_H is not None:
            return "true_D / true_H tracking"
        if getattr(self, "_shard_group", None) is not None:
            return "shard() (fp64 mode runs on one GPU)"
        if not 1 <= int(self.n_components) <= F64_MAX_K:
            return f"n_components={self.n_components} (fp64 mode: 1..{F64_MAX_K} components)"
        return None

    # ---- hooks implemented by the concrete estimator -------------------------------------------------
    @abstractmethod
    def _iteration(self, W, H):
        pass

    def _engine_kwargs(self):
        return {}

    def _detailed(self, lkl, reg, lap):
        return [lkl]

    # ---- loss -----------------------------------------------------------------------------------------
    def _make_engine(self, X_fixed, xscale, G, filled_channels=None, filled_pixels=None, layout="cm", autotune=False, shard=None, x_facts=None,
                     x_local=False):
        """The device engine of a fit; with ``shard`` (a sharding.FitShard) X_fixed is the WHOLE image and the engine takes this rank's
        block of it - or, with ``x_local``, that block already (then ``filled_pixels`` is the block's mask too)."""
        from espm_amd.engine import MUEngine
        shape_2d, fixed_H, group = self.shape_2d, self.fixed_H, None
        if shard is not None:
            if not x_local:
                X_fixed = X_fixed[shard.sl] if layout == "pm" else X_fixed[:, shard.sl]
                filled_pixels = shard.cols(filled_pixels)
            shape_2d, group = shard.shape_2d, shard.group
            fixed_H = shard.cols(np.asarray(fixed_H)) if fixed_H is not None else None
            x_facts = None      # (they describe the whole image)

        rows = None
        if self.physics_model_ is not None and self.simplex_W:
            rows = self.physics_model_.NMF_simplex()
        # (the Bregman W update has no simplex branch, updates.py:40-48: algo="bmd" ignores simplex_W there, like the reference)
        simplex_W = self.simplex_W and getattr(self, "algo", None) != "bmd"
        if self.l2:
            # Frobenius data term (only kept by SmoothNMF with algo="l2_surrogate", smooth_nmf.py:223-237): the W step has no
            # simplex there (updates.py:31-36); the engine's Frobenius mode takes the scaled X itself
            simplex_W = False
            if xscale != 1.0:
                X_fixed, xscale, x_facts = X_fixed * xscale, 1.0, None
        # (and the projected-gradient W step of a fit is called without fixed_W, smooth_nmf.py:430-437)
        fixed_W = None if getattr(self, "algo", None) == "projected_gradient" else self.fixed_W
        return MUEngine(X_fixed, self.n_components, G=G, shape_2d=shape_2d, simplex_H=self.simplex_H,
                        simplex_W=simplex_W, log_shift=self.log_shift, tol=self.tol, fixed_H=fixed_H,
                        fixed_W=fixed_W, simplex_rows=rows, xscale=xscale, max_iter=self.max_iter,
                        fix_zero_lines=False, filled_channels=filled_channels, filled_pixels=filled_pixels, layout=layout,
                        autotune=autotune, group=group, x_facts=x_facts, **self._engine_kwargs(),
                        **({"precision": "fp64"} if self._fp64() else {}))

    def _engine_G(self):
        G = self.G_
        if self._identity_G:
            return None
        return G

    def loss(self, W, H, average=True, X=None):
        """Loss of (W, H) (espm/estimators/base.py:167-207): generalised KL divergence of X from
        G W H (plus the regularisers of the subclass), evaluated on the device."""
        self.GWH_numel_ = self.G_.shape[0] * H.shape[1]
        if X is None:
            eng = self._get_engine()
        else:
            assert X.shape == (self.G_.shape[0], H.shape[1])
            eng = self._make_engine(np.asarray(X), 1.0, self._engine_G())
        eng.load_state(W, self._local_H(eng, H))   # (the sharded engine of a fit: this rank's block of H; the loss is summed over the ranks)
        eng.eval_current(advance_h=False)
        h = eng.history(upto=0, average=average)
        kl, loss = float(h["kl"][0]), float(h["loss"][0])
        if X is not None and not self.l2 and self.const_KL_ is not None:
            # base.py:196-203: the constant of the KL term is the one cached for the FITTED data, also when another X is
            # handed in (the reference never recomputes it): replace the engine's own constant of `X`
            Xa = np.asarray(X, dtype=np.float64)
            own = float(np.sum(Xa * np.log(np.maximum(Xa, self.log_shift))) - np.sum(Xa))
            shift = (self.const_KL_ - own) / (float(self.GWH_numel_) if average else 1.0)
            kl, loss = kl + shift, loss + shift
        self.detailed_loss_ = self._detailed(kl, float(h["reg"][0]), float(h["lap"][0]))
        return loss

    def _get_engine(self):
        eng = getattr(self, "_engine", None)
        if eng is None:
            check_is_fitted(self, "X_")
            scale = getattr(self, "norm_factor_", 1.0) if self.normalize else 1.0
            eng = self._engine = self._make_engine(self._X_fixed(), scale, self._engine_G(), shard=getattr(self, "_shard", None))
        return eng

    def _X_fixed(self):
        X = self.X_
        if self.normalize:
            X = X / self.norm_factor_
        return X

    # ---- fit --------------------------------------------------------------------------------------------
    def fit_transform(self, X, y=None, W=None, H=None):
        """Learn X ~ G W H and return G W (or H.T with ``hspy_comp``), espm/estimators/base.py:209-420.

        Six stages, each a method that reads and fills the fit's context ``f`` (a SimpleNamespace; the stages' docstrings name the reference lines
        they stand for): validation, ingest (for a large X: ONE upload whose scans replace the reference's host passes), the initial W / H / G, the
        engine, the iteration loop with the stop rules, the results."""
        import types
        # (fit_binned sets its attributes again after its coarse fit, fit_split its own after the fit of the training part)
        for name in self._BINNED_ATTRIBUTES + self._SPLIT_ATTRIBUTES:
            self.__dict__.pop(name, None)
        f = types.SimpleNamespace()
        self._fit_validate(f, X)
        self._fit_ingest(f)
        self._fit_initial_state(f, W, H)
        eng = self._fit_engine(f)
        self._fit_loop(f, eng)
        return self._fit_results(f, eng)

    def _fit_validate(self, f, X):
        """base.py:243-259: scikit-learn's validation (the finiteness scan of a large array moves to its device copy), the hyperspy caller check, the l2 guard."""
        # base.py:243-247.  For a large array that will be uploaded anyway the finiteness scan of validate_data (a full
        # host pass: 0.18 s at 2048 x 512^2 fp32) moves to the device copy below; everything else
        # (dtype, shape, n_features_in_, feature names) is still scikit-learn's.
        # ESPM_FIT_TIMING=1: host-side time stamps of the fit's sections (no device synchronisation), printed at its end
        if self._fp64():   # (before anything is uploaded)
            why = self._fp64_refusal()
            if why is not None:
                raise NotImplementedError(f"fp64 mode (set_precision('fp64')) does not cover {why}")
        marks = [("enter", time.perf_counter())] if os.environ.get("ESPM_FIT_TIMING") else None
        mark = (lambda name: marks.append((name, time.perf_counter()))) if marks is not None else (lambda name: None)
        big = ingest.device_prep_applies(X, self._fp64())
        vkw = dict(dtype=[np.float64, np.float32], ensure_all_finite=not big)
        if self.hspy_comp:
            Xv = validate_data(self, X.T, **vkw)
        else:
            Xv = validate_data(self, X, **vkw)
        mark("validate_data")
        if self.hspy_comp is False:
            try:  # base.py:249-259
                # (the reference asks inspect.getouterframes(inspect.currentframe(), 2) for calframe[1][3] and calframe[1][1]: the
                #  caller's function name and file.  The frame object has both; inspect also loads two lines of source context for
                #  EVERY frame of the stack - linecache stat calls that took 76 ms in one fit of five - and its list of frames
                #  holds this frame, which holds the list: a cycle that kept every local of the fit alive until the collector ran.)
                import sys
                caller = sys._getframe(2)   # (this method <- fit_transform <- the caller the reference's check looks at)
                calframe = [None, (caller, caller.f_code.co_filename, caller.f_lineno, caller.f_code.co_name)]
                caller = None
                if calframe[1][3] == "decomposition" and "hyperspy" in calframe[1][1]:
                    print("Are you calling the function decomposition from Hyperspy?\n"
                          "If so, please set the compatibility argument 'hspy_comp' to True.\n\n"
                          "If this argument is not set correctly, the function will not work properly!!!")
            except Exception:
                pass
            finally:
                calframe = None      # (no frame reference outlives the check: tools/analysis/est_cycle_probe.py)
        mark("caller check (inspect)")
        if self.l2 and getattr(self, "algo", None) != "l2_surrogate":
            raise NotImplementedError("the Frobenius loss (l2=True) is built for SmoothNMF(algo='l2_surrogate'), the one "
                                      "combination in which the reference keeps it (smooth_nmf.py:223-237)")
        f.marks, f.mark, f.big, f.Xv = marks, mark, big, Xv

    def _fit_ingest(self, f):
        """base.py:261-268, :519-528, :200-201: sign check, zero lines, mean / normalisation, X_, const_KL_ - for a large X on ONE device copy (a sharded fit: on this rank's block, scans combined over the ranks)."""
        Xv, mark = f.Xv, f.mark
        # one fit over several GPUs (shard()): decided BEFORE the upload, so that a large X goes to the device as this rank's block
        # of image rows only - its scans are combined over the ranks, the initialisation's passes run on the blocks
        # (espm_amd/init_device.py), the engine takes the block as it is.  Set-up time and device memory per rank shrink with the
        # number of ranks like the iteration does (the reference: base.py:243-295, updates.py:160-223).
        grp = getattr(self, "_shard_group", None)
        shard = None
        if grp is not None:
            import torch
            if torch.distributed.get_world_size(grp) > 1:
                shard = _Shard(grp, self.shape_2d, int(Xv.shape[1]))
        # Large X: ONE upload whose scans stand for the reference's host passes (ingest_device).  Small X, fp64 mode: the host path, like the
        # reference.  (The validated array is float and 2-D: its size decides; the finiteness scan is owed only where validate_data skipped it.)
        if ingest.device_prep_applies(Xv, self._fp64()):
            rec = ingest.ingest_device(Xv, self.log_shift, shard=shard, check_finite=f.big, keep_host_copy=True, mark=mark)
        else:
            mark("finite / sign checks read back")
            rec = ingest.ingest_host(Xv, self.log_shift, self.remove_zeros_lines)
            mark("empty lines, mean read back")
        self.const_KL_ = None
        xscale, x_init = 1.0, None   # (x_init: the device image as the initialisation and the loop see it; None on the host path)
        if self.normalize:
            self.norm_factor_ = (normalization_factor(rec.X_fixed, self.n_components) if rec.mean_x is None
                                 else self.n_components / (rec.mean_x * Xv.shape[0]))
            xscale = float(self.norm_factor_)
        if rec.lazy is not None:   # the estimator's own host copy X_ of a large X, made on a worker thread (ingest._HostCopy)
            # X_ is the estimator's own array, like the reference's (remove_zeros_lines copies): the worker thread fills the empty
            # lines and applies the normalisation
            zp_all = rec.empty_px
            if rec.fill and rec.x_local:   # (the host copy is the whole image: it fills the empty pixels of every rank's block)
                import torch
                zp_all = torch.from_numpy(shard.gather_cols(zp_all.to(torch.uint8)[None, :])[0].astype(bool))
            rec.lazy.finish(zp_all.cpu().numpy() if rec.fill else None, rec.empty_ch.cpu().numpy() if rec.fill else None, self.log_shift,
                        self.norm_factor_ if self.normalize else None)
            self.X_ = rec.lazy
            # the copy runs from here on - behind the upload, next to the initialisation, the engine set-up and the loop (~120 ms
            # for its ~45): joined at the end of the fit it has long finished.  (Rounds 2-3 started it at the loop, because
            # started earlier it "stalled" whatever phase it overlapped: that was the container's CPU quota, _cpu_budget.py.
            # ESPM_HOSTCOPY_START=loop restores that; profiles/r03ac_fit_timing_*.log.)
            if os.environ.get("ESPM_HOSTCOPY_START", "early") == "early":
                rec.lazy.start()
            x_init = rec.Xd * xscale if self.normalize else rec.Xd
            rec = rec._replace(const_kl=ingest.const_kl_device(rec, x_init, self.normalize, self.log_shift, shard))
        else:
            self.X_ = self.norm_factor_ * rec.X_fixed if self.normalize else rec.X_fixed
        mark("const_KL read back")
        f.rec, f.shard, f.xscale, f.x_init = rec, shard, xscale, x_init

    def _fit_initial_state(self, f, W, H):
        """base.py:269-295 with updates.py:160-223: the physics model's G, W0 / H0 (NNDSVD on the device for a large X), rank 0's arrays on every rank of a sharded fit."""
        mark, shard, rec, X_init_dev = f.mark, f.shard, f.rec, f.x_init
        f.x_init = None
        if _is_physical_model(self.G):
            self.physics_model_ = self.G
            G = self.physics_model_.NMF_update()
        else:
            self.physics_model_ = None
            G = self.G
        self._identity_G = G is None
        # (Round 5, measured and withdrawn: the engine's build - it needs the uploaded X and G, not W or H - on a worker thread and a stream of its
        #  own BESIDE the initialisation: the two take 28.5 + 12.6 ms one after the other and 39.6 + 0.1 side by side - both are chains of
        #  launches that fill the device, not waits; profiles/r05g_fit_timing*.log)
        self.G_, self.W_, self.H_ = initialize_algorithms(X=self.X_, G=G, W=W, H=H, n_components=self.n_components,
                                                          init=self.init, random_state=self.random_state,
                                                          simplex_H=self.simplex_H, simplex_W=self.simplex_W,
                                                          physics_model=self.physics_model_, X_device=X_init_dev,
                                                          shard=shard if rec.x_local else None,   # (X_device is this rank's block of pixels)
                                                          # (the mean of what the initialisation sees: known from the upload's scans)
                                                          X_mean=None if rec.mean_x is None else rec.mean_x * f.xscale)
        del X_init_dev
        mark("initialize_algorithms")
        # one fit over several GPUs (shard()): this rank's block of image rows; every rank starts from rank 0's W, H, G
        if shard is not None:
            import torch
            dev = f"cuda:{torch.cuda.current_device()}"
            self.G_, self.W_, self.H_ = shard.broadcast([self.G_, self.W_, self.H_], dev)
        self._shard = shard
        say = print if shard is None or shard.rank == 0 else (lambda *a, **k: None)   # (the reference's messages: once, not per rank)
        # L_ (base.py:286-291) is only an attribute here - the kernels apply the Laplacian as a stencil - and building the
        # sparse matrix of a 512 x 512 grid costs 0.07 s: it is built on first access (property L_ below)
        self._L_cache = None
        self._L_pixels = int(self.X_.shape[1])

        out_dtype = np.dtype(np.float64) if self._fp64() else self.X_.dtype   # (fp64 mode: W_, H_ from the fp64 state)
        f.say, f.out_dtype = say, out_dtype

    def _fit_engine(self, f):
        """The device engine of the fit with its state loaded (a sharded fit: the record exchange rehearsed), const_KL_."""
        mark, shard, rec = f.mark, f.shard, f.rec
        f.rec = rec.without_x()   # (the context must not keep the device copies of X alive past the engine's build)
        on_device = rec.Xd_raw is not None
        # (the masks are passed where the upload's scans - or the host's sums - found lines to fill: no read-back to ask again)
        self._engine = eng = self._make_engine(rec.Xd_raw if on_device else rec.X_fixed, f.xscale, None if self._identity_G else self.G_,
                                                filled_channels=rec.empty_ch if rec.fill and bool(rec.empty_ch.any()) else None,
                                                filled_pixels=rec.empty_px if rec.fill and bool(rec.empty_px.any()) else None, layout=rec.layout,
                                                x_facts=rec.x_facts,
                                                # (timing the launch plans costs ~30 ms of device time and gains a few per cent
                                                #  per iteration: it pays for itself only in very long fits of large images)
                                                autotune="auto" if on_device else False,   # (MUEngine: from AUTOTUNE_MIN_ITERS iterations on)
                                                shard=shard, x_local=rec.x_local)
        self._ingest_layout = rec.layout   # "pm": the (pixels, channels) input went to the device without a transpose
        mark("engine built")
        del rec
        mark("device copies of X released")
        eng.load_state(self.W_, self.H_ if shard is None else shard.cols(self.H_))
        if shard is not None and getattr(eng, "sharded", False) and eng.exchange.ctx is not None:
            # the one-shot record exchange is rehearsed with the fit's own kernels before the loop depends on it; every rank
            # moves to the collective transport together if a wait gave up (MUEngine.settle_exchange), then the state again
            eng.settle_exchange()
            eng.load_state(self.W_, shard.cols(self.H_))
        self.GWH_numel_ = self.G_.shape[0] * self.H_.shape[1]
        self.const_KL_ = f.rec.const_kl   # (computed on the device copy of a large X)
        if self.const_KL_ is None:
            self.const_KL_ = float(np.sum(self.X_ * np.log(np.maximum(self.X_, self.log_shift))) - np.sum(self.X_))

        mark("state loaded, const_KL")
        return eng

    def _fit_loop(self, f, eng):
        """base.py:313-394: the iterations, the bookkeeping of every one of them and the stop rules; a sharded fit that loses a peer restarts once on the collective transport."""
        mark, shard, lazy, say, out_dtype = f.mark, f.shard, f.rec.lazy, f.say, f.out_dtype
        algo_start = time.time()
        self.n_iter_ = 0
        self._begin_fit()
        self.losses_, self.rel_, self.detailed_losses_ = [], [], []
        # ground-truth tracking (base.py:301-311): every iteration compares G W with true_D, H with true_H and
        # evaluates the loss against the noiseless true_D @ true_H (a second, loss-only engine holds that X)
        track = self._begin_truth_tracking()
        pg_ls = bool(getattr(self, "linesearch", False)) and getattr(self, "algo", None) == "projected_gradient"
        adapt = bool(getattr(self, "linesearch", False)) and not pg_ls
        sync_each = (not self.no_stop_criterion) or self.physics_model_ is not None or track or adapt or pg_ls or bool(self.l2)
        eval_before = np.inf
        eval_init = None
        stop = False
        if lazy is not None:
            lazy.start()
        G_start = None if self.physics_model_ is None else np.array(self.G_, copy=True)
        retried = False
        try:
            while True:   # (a second pass only after a sharded fit has had to change its record exchange, below)
                try:
                    eng.eval_current(advance_h=True)  # loss of the initial state rides on the first H-step
                    while not stop:
                        # how many iterations may run before the host has to look at a loss value
                        if sync_each:
                            chunk = 1
                        else:
                            chunk = self.max_iter - self.n_iter_
                            if self.verbose > 0:
                                chunk = min(chunk, self.eval_print - self.n_iter_ % self.eval_print)
                            chunk = max(chunk, 1)
                        if pg_ls:  # smooth_nmf.py:382-401: gamma_H from the quadratic bound, before the W-step
                            self.gamma_[0] = eng.pg_linesearch_h(self.gamma_[0])
                        eng.finish_iteration()
                        if adapt:  # smooth_nmf.py:376-381: gamma_ follows the Laplacian surrogate; in effect from the next H-step
                            self.gamma_ = eng.linesearch_step(self._gamma_value())
                        if chunk > 1:
                            eng.iterate(chunk - 1, final_loss=False)
                            eng.eval_current(advance_h=(self.n_iter_ + chunk) < self.max_iter)
                        else:
                            last = self.n_iter_ + 1 >= self.max_iter
                            refresh_G = self.physics_model_ is not None and (self.n_iter_ + 1) % 3 == 0
                            eng.eval_current(advance_h=not (last or refresh_G))
                        if pg_ls:  # smooth_nmf.py:438-447: gamma_W, once the new state has been evaluated
                            self.gamma_[1] = eng.pg_linesearch_w(self.gamma_[1])
                        first = self.n_iter_ + 1
                        self.n_iter_ += chunk
                        h = eng.history(upto=self.n_iter_)
                        if eval_init is None:
                            eval_init = float(h["loss"][0])
                        for t in range(first, self.n_iter_ + 1):
                            self.losses_.append(float(h["loss"][t]))
                            self.detailed_losses_.append(self._detailed(float(h["kl"][t]), float(h["reg"][t]),
                                                                        float(h["lap"][t])))
                            self.rel_.append([float(h["rel_W"][t]), float(h["rel_H"][t])])
                        if track:
                            self._track_truth(eng)
                        eval_after = self.losses_[-1]
                        rel_W, rel_H = self.rel_[-1]

                        if self.n_iter_ >= self.max_iter:  # base.py:354-378
                            say("exits because max_iteration was reached")
                            break
                        why = None if self.no_stop_criterion else stop_message(rel_W, rel_H, eval_before, eval_after, eval_init, self.tol)
                        if why is not None:
                            say(why)
                            break
                        if self.verbose > 0 and np.mod(self.n_iter_, self.eval_print) == 0:
                            say(f"It {self.n_iter_} / {self.max_iter}: loss {eval_after:3e},  "
                                  f"{self.n_iter_ / (time.time() - algo_start + log_shift):0.3f} it/s")
                        if self.physics_model_ is not None and self.n_iter_ % 3 == 0:  # base.py:388-392
                            self.G_ = self.physics_model_.NMF_update(eng.get_W().astype(out_dtype))
                            eng.set_G(self.G_)
                            eng.eval_current(advance_h=True)
                            eval_before = float(eng.history(upto=self.n_iter_)["loss"][self.n_iter_])
                        else:
                            eval_before = eval_after
                    break
                except Exception as e:   # noqa: BLE001
                    # A sharded fit on the one-shot record exchange whose bounded waits gave up AFTER the rehearsal before the loop
                    # (MUEngine.settle_exchange): history() raises on every rank at the same read-back (the health is a maximum over the ranks).
                    # Every rank then moves to the collective transport and the fit starts again from its initial W, H, G (the
                    # estimator needs the fallback bench.py has).  Anything else, or a second failure, is the caller's.
                    from espm_amd._lib import LostPeerError
                    if not isinstance(e, LostPeerError) or retried or shard is None or getattr(eng.exchange, "ctx", None) is None:
                        raise
                    retried = True
                    say("record exchange: a peer was lost on the one-shot transport; restarting the fit on the collective transport")
                    eng.use_collective_exchange()
                    if G_start is not None:
                        # the physics model's own state followed the abandoned iterates (NMF_update(W) every third iteration, base.py:388-392):
                        # it is brought back to the fit's start the way the fit got there - NMF_update() without W (base.py:269-274)
                        if self.physics_model_ is not None:
                            self.physics_model_.NMF_update()
                        self.G_ = G_start
                        eng.set_G(self.G_)
                    eng.load_state(self.W_, shard.cols(self.H_))
                    self.n_iter_, stop, eval_before, eval_init = 0, False, np.inf, None
                    self.losses_, self.rel_, self.detailed_losses_ = [], [], []
                    self._begin_fit()
                    track = self._begin_truth_tracking()
        except KeyboardInterrupt:
            pass
        finally:
            mark("loop (losses read back)")
            if lazy is not None:   # the host copy that was made meanwhile - also when the loop raised: X_ must not stay a stand-in
                self.X_ = lazy.result()   # (holding a thread and an event: not picklable)
        mark("host copy X_ joined")
        f.algo_start = algo_start

    def _fit_results(self, f, eng):
        """base.py:396-420: W_, H_ read back, rescaled_DH without a simplex, reconstruction_err_, the un-normalised W_, the return value by hspy_comp."""
        mark, marks, say, out_dtype, algo_start = f.mark, f.marks, f.say, f.out_dtype, f.algo_start
        self.W_ = eng.get_W().astype(out_dtype)
        self.H_ = self._full_H(eng).astype(out_dtype)
        mark("W, H read back")
        if marks is not None:
            print("[fit timing, ms] " + ", ".join(f"{n} {1e3 * (t - marks[i][1]):.1f}" for i, (n, t) in enumerate(marks[1:])) +
                  f" | total {1e3 * (marks[-1][1] - marks[0][1]):.1f}", flush=True)
        if not self.simplex_H and not self.simplex_W:
            self.W_, self.H_ = rescaled_DH(self.W_, self.H_)  # base.py:399-400

        algo_time = time.time() - algo_start
        say(f"Stopped after {self.n_iter_} iterations in {algo_time // 60} minutes "
              f"and {np.round(algo_time) % 60} seconds.")
        if not self.simplex_H and not self.simplex_W:
            self.reconstruction_err_ = self.loss(self.W_, self.H_)
        else:
            self.reconstruction_err_ = self.losses_[-1] if self.losses_ else self.loss(self.W_, self.H_)
            if self.losses_:
                self.detailed_loss_ = self.detailed_losses_[-1]
        if self.normalize:
            self.W_ = self.W_ / self.norm_factor_

        GW = self.G_ @ self.W_
        self.n_components_ = self.H_.shape[0]
        if self.hspy_comp:
            self.components_ = GW.T
            return self.H_.T
        self.components_ = self.H_
        return GW

    def _begin_fit(self):
        pass

    def _local_H(self, eng, H):
        """The block of H an engine holds: all of it, or this rank's image rows for the sharded engine of a fit."""
        return self._shard.cols(np.asarray(H)) if getattr(eng, "world", 1) > 1 else H

    def _full_H(self, eng):
        """H of the whole image: the engine's, or the ranks' blocks of a sharded fit assembled on every rank."""
        shard = getattr(self, "_shard", None)
        if shard is None or getattr(eng, "world", 1) == 1:
            return eng.get_H()
        return shard.gather_cols(eng.h[eng.st.cur][:, :eng.p])

    def fit(self, X, y=None, **params):
        """Learn a NMF model for the data X (espm/estimators/base.py:422-441).

        Deviation from the reference: ``n_components`` is limited to 32 (``NotImplementedError`` above that, raised before anything is
        uploaded).  The reference has no limit (base.py:126-132 stores the argument, updates.py:160-223 initialise any rank); here the
        kernels are compiled per component count - 1..8 in libespm_mu.so, 9..16 in libespm_mu_wide.so, 17..32 in libespm_mu_wide32.so -
        with the components of a pixel or channel in registers.  The sparse count store serves up to 16 components: sparse count data with
        more, or with 13-16 components and more than 2048-2144 channels (9-12: 2896-3024), take the dense 8-bit store (below 17 components
        with a RuntimeWarning: the sparse store's G W table would not fit a workgroup's LDS).

        After ``set_precision("fp64")`` the fit computes in fp64 with the reference's simplex bisection and its global stop, so that
        ``n_iter_`` and the trajectory follow the reference at a small ``tol``; ``W_`` and ``H_`` are float64.  Its scope:
        algo="log_surrogate" (mu, epsilon_reg, lambda_L), simplex_H or simplex_W, fixed_H / fixed_W, G identity / dictionary /
        physics model, normalize, hspy_comp, 1..8 components on one GPU; linesearch, l2, true_D / true_H, the other solvers,
        shard() and more than 8 components raise NotImplementedError before X is uploaded."""
        self.fit_transform(X, **params)
        return self

    # ---- transform: H of new data against the fitted W (an H-only fit) ---------------------------------------------------------
    def _transform_refusal(self):
        """Why ``transform`` cannot serve this estimator, or None."""
        if self._fp64():
            return "fp64 mode (set_precision('fp64')): its engine has no H-only iteration"
        if getattr(self, "linesearch", False):
            return "linesearch=True (gamma_ would have to adapt as in the fit)"
        if getattr(self, "algo", "log_surrogate") == "projected_gradient":
            return "algo='projected_gradient'"
        if self.l2:
            return "l2=True (the Frobenius fit)"
        if getattr(self, "_shard_group", None) is not None:
            return "an estimator that was shard()ed (transform runs on one GPU)"
        return None

    def unmix(self, X, H=None, shape_2d=None):
        """H of new data ``X`` against the fitted spectra (``transform`` is this method where the estimator is a scikit-learn transformer
        of pixels, ``hspy_comp=True``: see ``_PixelTransform``): what the reference computes with the same parameters, ``normalize=False``,
        ``fixed_W=Wf`` and ``fit_transform(Xs, W=Wf, H=H0)`` (base.py:293-420 with updates.py:75-76 overwriting every entry of W) -
        the H rule every iteration, rel_W = 0, the reference's stop rules and loss.  ``Wf``, ``Xs`` are ``W_`` and ``X``, both times
        the fit's ``norm_factor_`` under ``normalize`` (the factor is not recomputed: the objective is the one the fit minimised);
        G is the fitted ``G_`` (a physics model is not refreshed: W does not move).  ``H=None``: |lstsq(G W, X)|, normalised under
        ``simplex_H``, floored at ``log_shift`` (updates.py:213-221).  ``shape_2d``: the grid of ``X``'s pixels, by default the
        estimator's when the pixel count matches; the estimator's ``fixed_H`` belongs to the fitted image and is not applied.

        X is (channels, pixels), or (pixels, channels) with ``hspy_comp`` - then H.T is returned, as by ``fit_transform``.  The fitted
        attributes stay as they are; the run's own record goes to ``transform_n_iter_``, ``transform_losses_`` and ``transform_rel_``
        (rel_H of every iteration).  Built from the fit's stages with a context of its own; the stop-rule loop is ``_fit_loop``'s
        without the W step.  NotImplementedError, before anything is uploaded: linesearch, algo='projected_gradient', l2=True,
        shard(), fp64 mode."""
        import types
        check_is_fitted(self, "W_")
        why = self._transform_refusal()
        if why is not None:
            raise NotImplementedError(f"transform / unmix does not cover {why}")
        t = types.SimpleNamespace()
        self._transform_validate(t, X, shape_2d)
        self._transform_ingest(t)
        eng = self._transform_engine(t, H)
        self._transform_loop(t, eng)
        Hn = eng.get_H().astype(t.out_dtype)
        if not self.simplex_H and not self.simplex_W:   # base.py:399-400
            Hn = rescaled_DH(t.Wf.astype(t.out_dtype), Hn)[1]
        return Hn.T if self.hspy_comp else Hn

    def _transform_validate(self, t, X, shape_2d):
        """scikit-learn's validation against the fitted channel count (reset=False), the grid of the new pixels."""
        big = ingest.device_prep_applies(X, False)   # (fp64 mode was refused before)
        # (scikit-learn counts the PIXELS as features here, base.py:243-247: the new data may have another number of them, so the
        #  array is checked as in the fit but not against n_features_in_)
        from sklearn.utils.validation import check_array
        vkw = dict(dtype=[np.float64, np.float32], ensure_all_finite=not big)
        Xv = check_array(X.T if self.hspy_comp else X, **vkw)
        if Xv.shape[0] != self.G_.shape[0]:
            raise ValueError(f"X has {Xv.shape[0]} channels, the fitted G_ has {self.G_.shape[0]}")
        p = int(Xv.shape[1])
        if shape_2d is None and self.shape_2d is not None and int(self.shape_2d[0]) * int(self.shape_2d[1]) == p:
            shape_2d = self.shape_2d
        if shape_2d is not None and int(shape_2d[0]) * int(shape_2d[1]) != p:
            raise ValueError(f"shape_2d {tuple(shape_2d)} does not match the {p} pixels of X")
        if shape_2d is None and getattr(self, "lambda_L", 0) != 0:
            raise ValueError(f"lambda_L != 0 needs the grid of the {p} pixels of X: pass shape_2d (the estimator's is {self.shape_2d})")
        t.Xv, t.big, t.shape_2d = Xv, big, shape_2d

    def _transform_ingest(self, t):
        """_fit_ingest for data that is not kept: sign check and empty lines (base.py:519-528) on the host, or for a large X on its ONE
        device copy by the upload's scans; the fit's norm_factor_."""
        t.xscale = float(self.norm_factor_) if self.normalize else 1.0
        t.rec = (ingest.ingest_device(t.Xv, self.log_shift, shard=None, check_finite=True, keep_host_copy=False) if t.big
                 else ingest.ingest_host(t.Xv, self.log_shift, self.remove_zeros_lines))   # (ValueError on negative values)

    def _transform_engine(self, t, H):
        """The engine of the new data - the fit's parameters, the new grid, no fixed_H, W held - with (Wf, H0) loaded.  Not cached."""
        from espm_amd.engine import MUEngine
        k, rec = self.n_components, t.rec
        t.rec = None
        t.out_dtype = t.Xv.dtype
        Wf = np.maximum(np.asarray(self.W_, dtype=np.float64) * t.xscale, self.log_shift)   # (W_ is stored un-normalised, base.py:417-418)
        t.Wf = Wf
        G = None if self._identity_G else self.G_
        if H is None:   # updates.py:213-221
            GW = Wf if G is None else np.asarray(G, dtype=np.float64) @ Wf
            if rec.Xd_raw is not None:
                import torch
                gw = torch.from_numpy(GW).to(rec.Xd_raw.device)
                H0 = (torch.linalg.pinv(gw) @ (rec.Xd.to(torch.float64) * t.xscale)).abs().cpu().numpy()
            else:
                H0 = np.abs(np.linalg.lstsq(GW, np.asarray(rec.X_fixed, dtype=np.float64) * t.xscale, rcond=None)[0])
            if self.simplex_H:
                H0 = H0 / H0.sum(axis=0, keepdims=True)
        else:
            H0 = np.asarray(H.T if self.hspy_comp else H, dtype=np.float64)
            if H0.shape != (k, t.Xv.shape[1]):
                raise ValueError(f"H must be {(k, t.Xv.shape[1])}, got {H0.shape}")
        H0 = np.maximum(H0, self.log_shift)
        kw = dict(self._engine_kwargs())
        kw.pop("frobenius", None)
        kw.pop("pg_gamma_w", None)
        eng = MUEngine(rec.X_fixed if rec.Xd_raw is None else rec.Xd_raw, k, G=G, shape_2d=t.shape_2d, simplex_H=self.simplex_H,
                       simplex_W=False, log_shift=self.log_shift, tol=self.tol, fixed_H=None, fixed_W=None, xscale=t.xscale,
                       max_iter=self.max_iter, fix_zero_lines=False, filled_channels=rec.empty_ch if rec.fill else None,
                       filled_pixels=rec.empty_px if rec.fill else None, layout=rec.layout, autotune=False, x_facts=rec.x_facts, **kw)
        del rec
        eng.load_state(Wf, H0)
        # which store the new data went on and whether its iteration is one launch (include/espm_mu.h: espm_mu_h_chain_applies)
        self.transform_path_ = dict(x_store=eng.x_store, n_heavy=int(eng.n_heavy), h_chain=int(eng.h_chain_applies()))
        return eng

    def _transform_loop(self, t, eng):
        """_fit_loop's logic (base.py:313-394) without the W step, truth tracking or G refresh: rel_W = 0."""
        say = print if self.verbose else (lambda *a, **k: None)
        self.transform_n_iter_ = 0
        self.transform_losses_, self.transform_rel_ = [], []
        n, eval_before, eval_init = 0, np.inf, None
        if self.no_stop_criterion and not self.verbose:
            eng.iterate_h(self.max_iter, final_loss=True)
            n = self.max_iter
            h = eng.history(upto=n)
            self.transform_losses_ = [float(v) for v in h["loss"][1:n + 1]]
            self.transform_rel_ = [float(v) for v in h["rel_H"][1:n + 1]]
            self.transform_n_iter_ = n
            return
        eng.advance_h_only()   # the loss of the initial state rides on the first H-step
        while True:
            n += 1             # state n is the current one; the H-step FROM it evaluates it (and proposes state n + 1)
            last = n >= self.max_iter
            if last:
                eng.eval_current(advance_h=False)
            else:
                eng.advance_h_only()
            h = eng.history(upto=n)
            if eval_init is None:
                eval_init = float(h["loss"][0])
            eval_after, rel_H = float(h["loss"][n]), float(h["rel_H"][n])
            self.transform_losses_.append(eval_after)
            self.transform_rel_.append(rel_H)
            self.transform_n_iter_ = n
            if last:
                say("exits because max_iteration was reached")
                break
            why = None if self.no_stop_criterion else stop_message(0.0, rel_H, eval_before, eval_after, eval_init, self.tol)
            if why is not None:
                say(why)
                eng.retreat_h()   # (state n + 1 was proposed, state n is the result)
                break
            if self.verbose > 0 and np.mod(n, self.eval_print) == 0:
                say(f"It {n} / {self.max_iter}: loss {eval_after:3e}")
            eval_before = eval_after

    def inverse_transform(self, W):
        """G W H_ (espm/estimators/base.py:461-477)."""
        check_is_fitted(self)
        return self.G_ @ W @ self.H_

    @property
    def L_(self):
        """Laplacian of the pixel grid (espm/utils.py:39-76) or the identity without ``shape_2d`` (base.py:286-291), built on
        first access."""
        if getattr(self, "_L_cache", None) is None:
            if not hasattr(self, "_L_pixels"):
                raise AttributeError("L_")
            self._L_cache = (create_laplacian_matrix(*self.shape_2d) if self.shape_2d is not None
                             else identity_laplacian(self._L_pixels))
        return self._L_cache

    @L_.setter
    def L_(self, value):
        self._L_cache = value

    def get_losses(self):
        """Structured array of the loss history (espm/estimators/base.py:479-517); with true_D / true_H given also the
        spectral angles, the map errors and the loss against the noiseless truth of every iteration."""
        names = ["full_loss"] + self.loss_names_ + ["rel_W", "rel_H"]
        tracked = self.true_D is not None and self.true_H is not None
        if tracked:  # base.py:483-499 (the reference fails here when the truth was ignored for its shape; so does this)
            names += [f"ang_p{i}" for i in range(self.n_components)] + [f"mse_p{i}" for i in range(self.n_components)]
            names += ["true_KL_loss"]
        dt = np.dtype([(elt, "float64") for elt in names])
        rows = []
        for i in range(len(self.losses_)):
            row = (self.losses_[i],) + tuple(self.detailed_losses_[i]) + tuple(self.rel_[i])
            if tracked:
                row += tuple(self.angles_[i]) + tuple(self.mse_[i]) + (self.true_losses_[i],)
            rows.append(row)
        return np.array(rows, dtype=dt)

    # ---- ground-truth tracking (espm/estimators/base.py:301-311, :335-347) ------------------------------------------
    def _begin_truth_tracking(self):
        self._truth_engine = None
        if self.true_D is None or self.true_H is None:
            return False
        true_D, true_H = np.asarray(self.true_D), np.asarray(self.true_H)
        if true_D.shape[1] != self.n_components or true_H.shape[0] != self.n_components:
            print("The chosen number of components does not match the number of components of the provided truth. "
                  "The ground truth will be ignored.")
            return False
        self.angles_, self.mse_, self.true_losses_ = [], [], []
        true_DH = (true_D @ true_H).astype(np.float64)
        # loss(W, H, X = true_DH) adds the constant cached for the DATA, not the one of true_DH (base.py:196-203)
        self._truth_const = float(np.sum(true_DH * np.log(np.maximum(true_DH, self.log_shift))) - np.sum(true_DH))
        self._truth_engine = self._make_engine(true_DH, 1.0, self._engine_G())
        return True

    def _track_truth(self, eng):
        from espm_amd.measures import find_min_angle, find_min_MSE
        W, H = eng.get_W().astype(np.float64), self._full_H(eng).astype(np.float64)   # (sharded fit: every rank tracks the whole image)
        Wc, Hc = (W, H) if (self.simplex_H or self.simplex_W) else rescaled_DH(W, H)
        GW = self.G_ @ Wc
        self.angles_.append(find_min_angle(np.asarray(self.true_D).T, GW.T, unique=True))
        self.mse_.append(find_min_MSE(np.asarray(self.true_H), Hc, unique=True))
        te = self._truth_engine
        te.load_state(W, Hc)                      # base.py:344: loss(self.W_, H, X = true_DH) - W as fitted, H rescaled
        te.eval_current(advance_h=False)
        h = te.history(upto=0, average=False)
        numel = float(self.G_.shape[0] * Hc.shape[1])
        lkl = float(h["kl"][0]) if self.l2 else float(h["kl"][0]) - self._truth_const + self.const_KL_
        self.true_losses_.append((lkl + float(h["reg"][0]) + float(h["lap"][0])) / numel)

    def remove_zeros_lines(self, X, epsilon):
        """All-zero rows / columns of X become epsilon (espm/estimators/base.py:519-528)."""
        if np.all(X >= 0):
            new_X = X.copy()
            new_X[:, X.sum(axis=0) == 0] = epsilon
            new_X[X.sum(axis=1) == 0, :] = epsilon
            return new_X
        raise ValueError("Negative values in data")
