"""Poisson sampling on the device (csrc/mu_sample.hip): count images drawn from a model D H, the deviance of such draws against the
model that generated them, and what both are for - a scale for the deviance map and the parametric bootstrap of a fit
(``NMFEstimator.simulate``, ``calibrate_deviance``, ``bootstrap``).  The reference draws its noisy images with ``np.random.poisson`` on
the host (datasets/base.py:68).

The sample is defined by a rule, not by the kernel (include/espm_mu.h, "Poisson sampling"): element (c, j) of the image, seen as
(channels, pixels), has the index e = c p + j and the rate y = sum_i D[c, i] H[i, j], formed in fp64 with every product and sum
rounded on its own.  With m = floor(y) and thr = floor((y - m) 2^32), its count is m unit Poisson draws - one per 32-bit word of
Philox4x32-10 on the counter (e low, e high, block, replicate + 1) with the key (seed low, seed high), a word w giving
#{i : w >= UNIT_CDF[i]} - plus a unit draw thinned to the fraction thr / 2^32.  So a replicate depends on (D, H, seed, replicate)
alone, bit for bit - not on the layout it is written in, the device, or how the work was cut.  Rates above 65535 saturate (the dtype's
maximum, no draw), rates that are negative or not finite give 0; both are counted.

There is no CPU path: ``sample`` and ``null_deviance`` need the GPU.  ``calibrate`` is host numpy."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_layout, check_log_shift, check_model, check_seed, layout_code

# T_i = floor(2^32 sum_{j <= i} e^-1 / j!): a 32-bit word w is the Poisson(1) draw #{i : w >= UNIT_CDF[i]}
UNIT_CDF = (0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f, 0xfffffe21,
            0xffffffd4, 0xfffffffc)
MAX_K = 32          # ESPM_SAMPLE_MAX_K
MAX_RATE = 65535    # ESPM_SAMPLE_MAX_RATE
MAX_REPLICATE = 2 ** 32 - 2


def _check_replicate(replicate, n_rep=1):
    if isinstance(replicate, bool) or int(replicate) != replicate or not 0 <= int(replicate) <= MAX_REPLICATE - (n_rep - 1):
        raise ValueError(f"replicate must be an integer with replicate + n_rep - 1 in 0 .. 2^32 - 2, not {replicate!r} (n_rep = {n_rep})")
    return int(replicate)


def _check_n_rep(n_rep):
    if isinstance(n_rep, bool) or int(n_rep) != n_rep or not 1 <= int(n_rep) <= 2 ** 31 - 1:
        raise ValueError(f"n_rep must be a positive integer, not {n_rep!r}")
    return int(n_rep)


def _model(D, H):
    """D (n, k) and H (k, p) as contiguous fp64 host arrays after every check: nothing is uploaded here."""
    _, _, _, D, H = check_model(D, H, "sampling", MAX_K)
    for name, A in (("D", D), ("H", H)):
        if not np.isfinite(A).all():
            raise ValueError(f"{name} holds values that are not finite")
        if (A < 0).any():
            raise ValueError(f"{name} holds negative values: a Poisson rate is D H >= 0")
    return D, H


def _upload(D, H):
    """(Dd, Hd, device): the model on the GPU."""
    from espm_amd.engine import require_gpu
    dev = require_gpu(None)
    return (*_image.model_on_device(dev, D, H), dev)   # (D and H may be read-only arrays: those are copied)


def _draw(Dd, Hd, dev, seed, replicate, dtype, layout):
    """One replicate of the resident model: (X on the device, saturated, invalid)."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    n, k = (int(v) for v in Dd.shape)
    p = int(Hd.shape[1])
    with torch.cuda.device(dev):
        X = torch.empty((n, p) if layout == "cm" else (p, n), dtype=torch.uint8 if dtype == np.uint8 else torch.uint16, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib.espm_poisson_sample(_ptr(Dd), _ptr(Hd), k, n, p, p, 0, seed, replicate, _ptr(X),
                                                _lib.DIAG_X_U8 if dtype == np.uint8 else _lib.DIAG_X_U16,
                                                layout_code(layout), int(X.stride(0)), _ptr(counts), _stream()))
        saturated, invalid = (int(v) for v in counts.cpu().numpy())
    return X, saturated, invalid


def _check_sample_args(seed, replicate, dtype, layout):
    seed, replicate = check_seed(seed), _check_replicate(replicate)
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise ValueError(f"dtype must be uint8 or uint16 (counts), not {dtype}")
    check_layout(layout)
    return seed, replicate, dtype


def sample(D, H, seed=0, replicate=0, dtype=np.uint16, layout="cm", device=False):
    """(X, info): replicate ``replicate`` of the model D (n, k) H (k, p) by the module's rule - X ~ Poisson(D H) entry by entry, as
    ``dtype`` (uint8 or uint16), (n, p) for ``layout="cm"`` or (p, n) for "pm", a host array, or with ``device=True`` a device tensor.
    ``info = dict(saturated=, invalid=)``: the entries stored as the dtype's maximum because their rate is above 65535 or their draw
    above the maximum, and the entries stored as 0 because their rate is negative or not finite (none, after the checks here).

    D and H are checked on the host - finite, non-negative, matching shapes, at most 32 components - and ``seed`` (0 .. 2^64 - 1),
    ``replicate`` (0 .. 2^32 - 2), ``dtype`` and ``layout`` too: ValueError (NotImplementedError for the components) before anything is
    uploaded.  One HIP kernel; the values use no atomics: the result is a function of (D, H, seed, replicate) alone, bit for bit, in
    both layouts."""
    seed, replicate, dtype = _check_sample_args(seed, replicate, dtype, layout)
    D, H = _model(D, H)
    Dd, Hd, dev = _upload(D, H)
    X, saturated, invalid = _draw(Dd, Hd, dev, seed, replicate, dtype, layout)
    return (X if device else X.cpu().numpy()), dict(saturated=saturated, invalid=invalid)


def null_deviance(D, H, n_rep=100, seed=0, replicate0=0, log_shift=1e-14):
    """(n_rep, p) float64: the per-pixel Poisson deviance 2 sum_c (x ln(x / Y) - x + Y), Y = max(D H, log_shift), of the replicates
    ``replicate0 .. replicate0 + n_rep - 1`` of the model against the model itself - the distribution a pixel's deviance has when the
    model is right.  Row r is the deviance of ``sample(D, H, seed, replicate0 + r)``; the replicates are never stored.  Checks as for
    ``sample``.  One HIP kernel, sums in channel order in the pixel's own thread: two calls give the same bits."""
    seed, n_rep = check_seed(seed), _check_n_rep(n_rep)
    replicate0 = _check_replicate(replicate0, n_rep)
    check_log_shift(log_shift)
    D, H = _model(D, H)
    Dd, Hd, dev = _upload(D, H)
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    n, k = D.shape
    p = H.shape[1]
    with torch.cuda.device(dev):
        out = torch.empty((n_rep, p), dtype=torch.float64, device=dev)
        _lib.check(_lib.lib.espm_sample_deviance(_ptr(Dd), _ptr(Hd), k, n, p, p, 0, seed, replicate0, n_rep, float(log_shift), _ptr(out), _stream()))
        return out.cpu().numpy()


def calibrate(deviance, null):
    """The deviance map on the scale of its null distribution: ``deviance`` (p,), ``null`` (n_rep, p) from ``null_deviance``.  Returns
    dict(``null_mean``, ``null_std`` (ddof = 1), ``z`` = (deviance - null_mean) / null_std, ``pvalue`` = (1 + #{r : null_r >= deviance})
    / (n_rep + 1)), each (p,): z says how many null standard deviations a pixel lies above what a right model gives, the p-value is
    the Monte-Carlo one (never 0: at least 1 / (n_rep + 1)).  Host numpy."""
    deviance, null = np.asarray(deviance, dtype=np.float64), np.asarray(null, dtype=np.float64)
    if null.ndim != 2 or deviance.ndim != 1 or null.shape[1] != deviance.shape[0]:
        raise ValueError("deviance must be (pixels,) and null (replicates, pixels)")
    n_rep = null.shape[0]
    if n_rep < 2:
        raise ValueError("calibrate needs at least two null replicates (the standard deviation has ddof = 1)")
    mean, std = null.mean(axis=0), null.std(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (deviance - mean) / std
    pvalue = (1.0 + (null >= deviance[None, :]).sum(axis=0)) / (n_rep + 1.0)
    return dict(null_mean=mean, null_std=std, z=z, pvalue=pvalue)
