"""Count attribution on the device (csrc/mu_attrib.hip): how many of the MEASURED counts stand behind every component of a fitted model
D H (D = G W in counts) - the question to answer before a concentration is quoted.  The reference answers it for the modelled intensity
(``utils.get_explained_intensity_W``, used by ``EDSespm.concentration_report(fit_error=True)``); that equals the measured one only at an
unregularised fixed point of the fit.

``expected``: the EM responsibilities.  With Y = max(D H, log_shift), entry (c, p) of X gives x d_cj h_jp / Y counts to component j;
summed over the channels that is ``pixel_counts`` (k, p), summed over the pixels ``channel_counts`` (n, k), and ``intensity`` carries
the latter through a dictionary or physics-model G to the entries of W.

``assign``: the same responsibilities as probabilities.  Every single count of X is handed to component j with probability
d_cj h_jp / y: by the Poisson splitting theorem the k parts of x ~ Poisson(sum_j l_j) are independent Poisson(l_j) images - integer
spectrum images, one per component, that add up to X exactly and keep whatever the model missed.  The parts are defined by a rule, not
by the kernel (include/espm_mu.h, "count attribution"): they depend on (X, D, H, seed) alone, bit for bit, in both layouts.  They cost
k times X in memory and in traffic (k = 5 at 2048 x 512 x 512 in 8 bits: 2.7 GB written for 0.54 GB read).

There is no CPU path: every function but ``intensity`` needs the GPU."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_image, check_log_shift, check_model, check_seed, counts_image

MAX_K = 32   # ESPM_ATTRIB_MAX_K


def expected(X, D, H, log_shift=1e-14, layout="cm"):
    """The expected attribution of the counts of X to the components of the model D (n, k), H (k, p).  With Y = max(D H, log_shift),
    returns dict(

    * ``pixel_counts`` (k, p): h_jp sum_c x_cp d_cj / Y_cp, the counts of pixel p attributed to component j,
    * ``ratio_sums`` (n, k): R_cj = sum_p x_cp h_jp / Y_cp,
    * ``channel_counts`` (n, k): D o R, the counts of channel c attributed to component j,
    * ``counts`` (p,): sum_c x_cp - int64 and exact for 8- or 16-bit X, float64 otherwise,
    * ``unattributed`` (p,): counts - sum_j pixel_counts, non-zero only where the model fell below ``log_shift``).

    X: the image as measured, non-negative, (channels, pixels) for ``layout="cm"`` or (pixels, channels) for "pm" - a host array or
    a device tensor in any dtype the as-measured rule reads (``_image_args.measured_dtype``).  1 .. 32 components.  Everything in
    fp64, sums in a fixed order, no atomics: two calls, and both layouts, give the same bits."""
    X = check_image(X)
    n, p, k, D, H = check_model(D, H, "expected", MAX_K, tuple(X.shape), layout)
    check_log_shift(log_shift)
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    img = _image.Resident(X, layout).upload()
    code, dev = img.code, img.dev
    with img.scope():
        Dd, Hd = img.model(D, H)
        num = torch.empty((k, p), dtype=torch.float64, device=dev)
        ratio = torch.empty((n, k), dtype=torch.float64, device=dev)
        cnt = torch.empty(p, dtype=torch.int64 if code in (_lib.DIAG_X_U8, _lib.DIAG_X_U16) else torch.float64, device=dev)
        need = int(_lib.lib.espm_attribute_expected_scratch(n, p, k))
        scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib.espm_attribute_expected(*img.abi(), _ptr(Dd), _ptr(Hd), k, float(log_shift), _ptr(num), _ptr(ratio), _ptr(cnt),
                                                    _ptr(scratch), need, _stream()))
        pixel_counts, ratio_sums, counts = num.cpu().numpy(), ratio.cpu().numpy(), cnt.cpu().numpy()
    return dict(pixel_counts=pixel_counts, ratio_sums=ratio_sums, channel_counts=D * ratio_sums, counts=counts,
                unattributed=counts - pixel_counts.sum(axis=0))


def assign(X, D, H, seed=0, layout="cm", device=False):
    """(parts, info): X split into k count images, one per component of the model D (n, k), H (k, p), by the module's rule - every
    count of entry (c, p) goes to component j with probability d_cj h_jp / (D H)_cp.  ``parts`` has the shape (k, *X.shape), X's
    layout and the dtype X was uploaded in (uint8 or uint16), and ``parts.sum(0) == X`` exactly; a host array, or with
    ``device=True`` a device tensor.  ``info = dict(invalid=)``: the non-zero entries whose modelled rate is not a finite number
    above 0 - all their counts are in ``parts[0]``.

    X as for ``splitting.thin``: integer counts 0 .. 65535, a host array or a device tensor; TypeError for floating-point X,
    ValueError for values out of range, a bad seed or shapes that do not match, NotImplementedError for more than 32 components -
    all before anything is uploaded.  One HIP kernel: the result is a function of (X, D, H, seed) alone, bit for bit."""
    seed = check_seed(seed)
    X, n, p = counts_image(X, layout)
    n, p, k, D, H = check_model(D, H, "assign", MAX_K, tuple(X.shape), layout)
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    img = _image.Resident(X, layout).upload()
    Xd, dev = img.Xd, img.dev
    with img.scope():
        Dd, Hd = img.model(D, H)
        parts = torch.empty((k,) + tuple(Xd.shape), dtype=Xd.dtype, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib.espm_assign_counts(*img.abi(), p, 0, _ptr(Dd), _ptr(Hd), k, seed, _ptr(parts), int(parts.stride(0)),
                                               int(parts.stride(1)), _ptr(cnt), _stream()))
        invalid = int(cnt.item())
    return (parts if device else parts.cpu().numpy()), dict(invalid=invalid)


def intensity(G, W, ratio_sums):
    """The measured counts behind every entry of W in D = G W: W o (G^T R) with R = ``expected(...)["ratio_sums"]`` - the measured
    counterpart of ``utils.get_explained_intensity_W``.  G None is the identity (W itself holds the spectra)."""
    W, R = np.asarray(W, dtype=np.float64), np.asarray(ratio_sums, dtype=np.float64)
    if G is None:
        if W.shape != R.shape:
            raise ValueError(f"W is {W.shape}, ratio_sums {R.shape}")
        return W * R
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != R.shape[0] or (G.shape[1], R.shape[1]) != W.shape:
        raise ValueError(f"G is {G.shape}, W {W.shape}, ratio_sums {R.shape}")
    return W * (G.T @ R)
