"""Poisson count splitting (data thinning) on the device (csrc/mu_split.hip): a training image and an independent held-out image of the
same specimen from ONE measured count map, and the held-out deviance of a fit of the first - an honest score for the number of
components, ``mu`` / ``lambda_L`` or a bin, which the in-sample ``deviance_`` cannot be (it falls with every added component).  The
reference has no analogue.

If x ~ Poisson(l) and x_a ~ Binomial(x, q), then x_a ~ Poisson(q l) and x_b = x - x_a ~ Poisson((1 - q) l), and the two are independent.
A model Y fitted to X_a therefore predicts r Y for X_b with r = (1 - q) / q, and 2 sum (x_b ln(x_b / (r Y)) - x_b + r Y) is the deviance
of data the fit has not seen.

The split is defined by a rule, not by the kernel (include/espm_mu.h, "count splitting"): element (c, j) of the image, seen as
(channels, pixels), has the index e = c p + j; draw d = 0 .. x - 1 of it is word (d mod 4) of Philox4x32-10 with the counter
(e low, e high, d div 4, 0) and the key (seed low, seed high), and count d goes to X_a iff its word < thr = round(q 2^32).  So the split
depends on (X, seed, q) alone - not on the layout X comes in, the device, or how the work was cut - and every function here reports
the fraction the split really has, ``q_eff = thr / 2^32``.

There is no CPU path: every function needs the GPU (X goes up as 8- or 16-bit counts, or stays where it is when it is a device
tensor)."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_log_shift, check_model, check_seed, counts_image


def threshold(q):
    """(thr, q_eff): the integer threshold round(q 2^32) (ties to even; held inside 1 .. 2^32 - 1) and the fraction thr / 2^32 of the
    counts that part A really gets.  ValueError unless 0 < q < 1."""
    try:
        q = float(q)
    except (TypeError, ValueError):
        raise ValueError(f"q must be a number with 0 < q < 1, not {q!r}") from None
    if not 0.0 < q < 1.0:
        raise ValueError(f"q must lie strictly between 0 and 1, not {q!r}")
    thr = min(max(int(round(q * 2.0 ** 32)), 1), 2 ** 32 - 1)
    return thr, thr / 2.0 ** 32


def _checked(X, q, seed, layout):
    """(image, thr, q_eff, seed) after every check of (X, q, seed, layout): the image by the counts-only rule, not yet uploaded."""
    thr, q_eff = threshold(q)
    seed = check_seed(seed)
    return _image.Resident(counts_image(X, layout)[0], layout), thr, q_eff, seed


def _resident(X, q, seed, layout):
    """X on the device as the kernels read it, after every check of (X, q, seed, layout): for callers that split and score the same
    image (one upload for both; a device tensor of 8- or 16-bit counts is returned as it is)."""
    return _checked(X, q, seed, layout)[0].upload().Xd


def _thin(X, q, seed, layout, want_b):
    img, thr, q_eff, seed = _checked(X, q, seed, layout)
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    Xd, dev = img.upload().Xd, img.dev
    with img.scope():
        Xa = torch.empty(Xd.shape, dtype=Xd.dtype, device=dev)
        Xb = torch.empty(Xd.shape, dtype=Xd.dtype, device=dev) if want_b else None
        _lib.check(_lib.lib.espm_thin_counts(*img.abi(), img.p, 0, thr, seed, _ptr(Xa), _ptr(Xb) if want_b else None, int(Xa.stride(0)),
                                             _stream()))
    return Xa, Xb, q_eff


def thin(X, q=0.5, seed=0, layout="cm", device=False):
    """(X_a, X_b): the thinning of the count image X by the module's rule - X_a holds a fraction ``threshold(q)[1]`` of every entry's
    counts in expectation, X_b = X - X_a the rest, and for Poisson X the two are independent Poisson images.  Both have X's shape and
    layout and the dtype X was uploaded in, as host arrays, or with ``device=True`` as device tensors.

    X: a host array or a device tensor of an integer dtype with values 0 .. 65535, (channels, pixels) for ``layout="cm"`` or
    (pixels, channels) for "pm"; uint8 and uint16 are read as they are, other integer dtypes are narrowed to the smaller of the two
    that holds them after a range check.  Floating-point X raises TypeError (thinning is defined for counts), negative values or
    values above 65535 ValueError, a q outside (0, 1) or a seed outside 0 .. 2^64 - 1 ValueError - all before anything is uploaded.
    One HIP kernel, no atomics: the result is a function of (X, q, seed) alone, bit for bit, in both layouts."""
    Xa, Xb, _ = _thin(X, q, seed, layout, True)
    return (Xa, Xb) if device else (_image.to_host(Xa), _image.to_host(Xb))


def split_deviance(X, D, H, q=0.5, seed=0, log_shift=1e-14, layout="cm"):
    """The in-sample and the held-out Poisson deviance of a model of the training part of X: D (n, k) and H (k, p) are ``G_ @ W_`` and
    ``H_`` of a fit of ``thin(X, q, seed)[0]``.  The kernel regenerates X_a from (X, seed) by the rule, so X_b is never stored or read
    back.  With Y = max(D H, log_shift) and r = (1 - q_eff) / q_eff, returns dict(

    * ``train_map`` (p,): 2 sum_c (x_a ln(x_a / Y) - x_a + Y) per pixel,
    * ``heldout_map`` (p,): 2 sum_c (x_b ln(x_b / (r Y)) - x_b + r Y) per pixel,
    * ``train``, ``heldout``: their totals, summed on the host in index order,
    * ``heldout_counts`` (p,) int64: sum_c x_b per pixel, exact,
    * ``q_eff``).

    X as for ``thin``; 1 .. 32 components; everything in fp64, sums in channel order: two calls, and both layouts, give the same
    bits."""
    img, thr, q_eff, seed = _checked(X, q, seed, layout)
    from espm_amd import _lib
    n, p, k, D, H = check_model(D, H, "split_deviance", _lib.SPLIT_MAX_K, tuple(img.host.shape), layout)
    check_log_shift(log_shift)
    import torch

    from espm_amd.engine import _ptr, _stream
    dev = img.upload().dev
    with img.scope():
        Dd, Hd = img.model(D, H)
        da = torch.empty(p, dtype=torch.float64, device=dev)
        db = torch.empty(p, dtype=torch.float64, device=dev)
        cb = torch.empty(p, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib.espm_split_deviance(*img.abi(), p, 0, thr, seed, _ptr(Dd), _ptr(Hd), k, float(log_shift), _ptr(da), _ptr(db),
                                                _ptr(cb), _stream()))
        train_map, heldout_map, counts = da.cpu().numpy(), db.cpu().numpy(), cb.cpu().numpy()
    return dict(train_map=train_map, heldout_map=heldout_map, train=_ordered_sum(train_map), heldout=_ordered_sum(heldout_map),
                heldout_counts=counts, q_eff=q_eff)


def _ordered_sum(v):
    """The sum of v in index order (numpy's pairwise ``sum`` is another order; ``cumsum`` adds one element after the other)."""
    return float(np.cumsum(v)[-1])


def scan(X, estimators, q=0.8, seeds=(0,)):
    """Score a list of candidate estimators (numbers of components, ``mu``, ``lambda_L``, ...) on one image by count splitting: X goes
    to the device once, for every seed it is thinned once (X_a comes to the host once and is shared), every estimator runs
    ``fit_transform`` on X_a and is scored with ``split_deviance`` - the stages of ``NMFEstimator.fit_split``, whose attributes every
    estimator carries afterwards, from the last seed.  Returns dict(``heldout`` and ``train`` (len(estimators), len(seeds)), ``best``:
    the index of the estimator with the least mean held-out deviance, ``q_eff``)."""
    estimators, seeds = list(estimators), [check_seed(s) for s in seeds]
    if not estimators or not seeds:
        raise ValueError("scan needs at least one estimator and one seed")
    thr, q_eff = threshold(q)
    for est in estimators:
        est._split_refusal()
    held, train = np.empty((len(estimators), len(seeds))), np.empty((len(estimators), len(seeds)))
    resident = {}   # X on the device, per layout the estimators read it in
    for s, seed in enumerate(seeds):
        parts = {}
        for i, est in enumerate(estimators):
            layout = "pm" if est.hspy_comp else "cm"
            if layout not in resident:
                resident[layout] = _resident(X, q, seed, layout)
            if layout not in parts:
                parts[layout] = _image.to_host(_thin(resident[layout], q, seed, layout, False)[0])
            est._fit_split_stages(resident[layout], parts[layout], q, seed, layout)
            held[i, s], train[i, s] = est.heldout_deviance_, est.train_deviance_
    return dict(heldout=held, train=train, best=int(np.argmin(held.mean(axis=1))), q_eff=q_eff)
