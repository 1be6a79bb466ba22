"""Spatial binning of a spectrum image on the device (csrc/mu_binning.hip): the binned image, and the reference's best-binning
estimate (espm/datasets/eds_spim.py:746-798) without a rebin and an upsample of the cube per candidate.

The image is ``shape_2d = (ny, nx)`` pixels, row-major, with n channels: X is (n, ny * nx) for ``layout="cm"`` or (ny * nx, n) for
``"pm"`` (hyperspy's unfolded cube).  A bin is a pair of positive integers (by, bx): pixel (y, x) belongs to bin (y // by, x // bx)
of a grid of ceil(ny / by) x ceil(nx / bx) bins.  The factors need not divide the image - the last row and column of bins are then
smaller - and a factor above the axis is the whole axis.

The estimator.  With K = ny nx pixels, L = n channels, S_gc the sum of X over bin g in channel c and n_g the pixels of the bin, the
reference's estimate for a binning - written there over the bin means spread back over the bins, u, and the pixels per bin, B:
var = mean(u / B), bias = mean((x - u)^2 - u / B - (1 - 2 / B) x), risk = var K / L + bias (eds_spim.py:782-793) - reduces to four
sums: T1 = sum x and T2 = sum x^2 over the cube, A = sum_gc S_gc^2 / n_g and C = sum_gc S_gc / n_g per candidate, with

    var = C / (K L),    bias = (T2 - T1 - A + C) / (K L),    risk = var K / L + bias.

Deviation from the reference: the estimator is defined here on INTEGER factors.  The reference feeds hyperspy's interpolating
``rebin`` with the non-integer scales ``size / i`` for i = 1 .. size // 2; that resampler is not rebuilt.  By default the candidates
are the square bins (b, b) for b = 1 .. min(ny, nx) // 2.

There is no CPU path: every function needs the GPU (X goes up in its own dtype - u8, u16, f32 or f64 are read as they are - or
stays where it is when it is a device tensor)."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_image, check_layout, image_dims


def _check(X, shape_2d, layout):
    """(X, n, ny, nx) before anything is uploaded."""
    check_layout(layout)
    X = check_image(X)
    if shape_2d is None or len(shape_2d) != 2:
        raise ValueError("shape_2d must be (rows, columns) of the image")
    ny, nx = int(shape_2d[0]), int(shape_2d[1])
    n, p = image_dims(X.shape, layout)
    if ny < 1 or nx < 1:
        raise ValueError("shape_2d must not be empty")
    if ny * nx != p:
        raise ValueError(f"shape_2d {(ny, nx)} does not match the {p} pixels of X")
    return X, n, ny, nx


def _check_bin(bin):
    try:
        by, bx = bin
    except (TypeError, ValueError):
        raise ValueError(f"a bin is a pair of positive integers (by, bx), not {bin!r}") from None
    if int(by) != by or int(bx) != bx or by < 1 or bx < 1:
        raise ValueError(f"a bin is a pair of positive integers (by, bx), not {bin!r}")
    return int(by), int(bx)


def binned_shape(shape_2d, bin):
    """The grid of bins: (ceil(ny / by), ceil(nx / bx))."""
    by, bx = _check_bin(bin)
    return -(-int(shape_2d[0]) // by), -(-int(shape_2d[1]) // bx)


def default_bins(shape_2d):
    """[(b, b) for b in 1 .. min(ny, nx) // 2] (at least (1, 1)): the integer counterpart of eds_spim.py:770-780."""
    return [(b, b) for b in range(1, max(1, min(int(shape_2d[0]), int(shape_2d[1])) // 2) + 1)]


def _is_integer(X):
    import torch
    if isinstance(X, torch.Tensor):
        return not (X.dtype.is_floating_point or X.dtype.is_complex)
    return np.asarray(X).dtype.kind in "iub"


def rebin(X, shape_2d, bin, layout="cm"):
    """The binned image: the sum of X over every (by, bx) block of pixels, per channel, as a host array in the layout given -
    (n, bins) for "cm", (bins, n) for "pm", the bins row-major on ``binned_shape(shape_2d, bin)``.

    float32 when every bin sum is exactly representable in it - integer input with max(X) by bx < 2^24 - or when X is float32;
    float64 otherwise.  Integer input is summed exactly, floating-point input in fp64, and rounded once.  X: a host array or a
    device tensor; ``bin=(1, 1)`` returns the values unchanged.  One HIP kernel; two calls give the same bits."""
    X, n, ny, nx = _check(X, shape_2d, layout)
    by, bx = _check_bin(bin)
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    integer = _is_integer(X)
    img = _image.Resident(X, layout).upload()
    Xd, dev = img.Xd, img.dev
    with img.scope():
        if integer:   # (torch has no reductions on 16-bit unsigned tensors: those go through a wider copy)
            top = np.asarray(X).max() if not isinstance(X, torch.Tensor) else (Xd.to(torch.int32) if Xd.dtype == torch.uint16 else Xd).max().item()
            f32 = int(top) * min(by, ny) * min(bx, nx) < (1 << 24)
        else:
            f32 = Xd.dtype == torch.float32
        gny, gnx = binned_shape((ny, nx), (by, bx))
        out = torch.empty((n, gny * gnx) if layout == "cm" else (gny * gnx, n), dtype=torch.float32 if f32 else torch.float64, device=dev)
        _lib.check(_lib.lib.espm_rebin_pixels(*img.abi()[:5], ny, nx, by, bx, _ptr(out), _lib.DIAG_X_F32 if f32 else _lib.DIAG_X_F64,
                                              int(out.stride(0)), _stream()))
        return out.cpu().numpy()


def binning_sums(X, shape_2d, bins, layout="cm"):
    """(T1, T2, A, C): sum x and sum x^2 over the cube, and per candidate of ``bins`` A = sum_gc S_gc^2 / n_g and
    C = sum_gc S_gc / n_g (float64 arrays of len(bins)).  One pass over X for the totals and one per candidate, fp64, without atomics:
    two calls give the same bits."""
    X, n, ny, nx = _check(X, shape_2d, layout)
    bins = [_check_bin(b) for b in bins]
    if not bins:
        raise ValueError("bins must hold at least one (by, bx)")
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    img = _image.Resident(X, layout).upload()
    dev = img.dev
    nb = len(bins)
    host_bins = np.ascontiguousarray(np.asarray(bins, dtype=np.int32).reshape(nb, 2))
    with img.scope():
        out = torch.empty(2 + 2 * nb, dtype=torch.float64, device=dev)
        nbytes = int(_lib.lib.espm_binning_sums_scratch(n, ny, nx, nb))
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib.espm_binning_sums(*img.abi()[:5], ny, nx, host_bins.ctypes.data, nb, _ptr(out), _ptr(scratch), nbytes, _stream()))
        host = out.cpu().numpy()
    return float(host[0]), float(host[1]), host[2::2].copy(), host[3::2].copy()


def risk_from_sums(T1, T2, A, C, n, ny, nx):
    """(var, bias, risk) of every candidate from the four sums (the module docstring; eds_spim.py:782-793)."""
    K, L = float(ny * nx), float(n)
    A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
    var = C / (K * L)
    bias = (T2 - T1 - A + C) / (K * L)
    return var, bias, var * K / L + bias


def binning_risk(X, shape_2d, bins=None, layout="cm"):
    """(bins, var, bias, risk): the reference's variance and squared-bias estimates and their combination for every candidate;
    ``bins=None``: ``default_bins(shape_2d)``."""
    X, n, ny, nx = _check(X, shape_2d, layout)
    bins = default_bins((ny, nx)) if bins is None else [_check_bin(b) for b in bins]
    T1, T2, A, C = binning_sums(X, (ny, nx), bins, layout=layout)
    var, bias, risk = risk_from_sums(T1, T2, A, C, n, ny, nx)
    return bins, var, bias, risk


def estimate_best_binning(X, shape_2d, bins=None, inspect=False, layout="cm"):
    """The candidate of least estimated risk, (by, bx) (eds_spim.py:746-798 on integer factors: the module docstring); with
    ``inspect=True`` (risk of every candidate, best), as the reference returns them."""
    bins, _, _, risk = binning_risk(X, shape_2d, bins=bins, layout=layout)
    best = bins[int(np.argmin(risk))]
    return (risk, best) if inspect else best
