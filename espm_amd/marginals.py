"""Line maps and region spectra on the device (csrc/mu_marginals.hip): weighted sums of the image X, of its model Y = max(D H,
log_shift) and of the deviance term along one axis, for several weight vectors at once - the two things an EDS user makes first and
last.  The reference's own workflow is built on channel windows (``select_background_windows``, ``masked_X = curr_X[mask]``,
eds_spim.py:364-384); exspy's ``get_lines_intensity`` is the line map.

Weights over the CHANNELS give maps (``pixel_maps``): a rectangular window, a background-corrected line (``line_weights``: the
correction is linear in X, so a net line is one signed weight vector, and its Poisson variance sum u^2 x the same pass with the
weights squared), a top-hat filter.  Weights over the PIXELS give spectra (``channel_spectra``): a phase mask or a label map
(``label_weights``), or abundances used as soft masks - the measured, the modelled and the residual spectrum of a region, where
``spectral_diagnostics`` has them for the whole image only.

The sums are defined by a rule (include/espm_mu.h, "weighted marginals"), in fp64, in a fixed order, without atomics: two calls, and
the two layouts of one image, give the same bits; with all weights 1 they are the diagnostics' own sums bit for bit.  A channel (or
pixel) whose weights are all zero is not read: a window of 20 channels costs 20 rows of X.

The weight builders and the host products of ``line_maps`` are numpy; everything else needs the GPU (there is no CPU path)."""
from __future__ import annotations

import numpy as np

from espm_amd import _image
from espm_amd._image_args import check_image, check_layout, check_log_shift, check_model, image_dims, narrowed_image

MAX_G = 8    # ESPM_MARG_MAX_G: weight vectors per launch (any number is accepted, in batches)
MAX_K = 8    # ESPM_MARG_MAX_K: components of a model on the device
LINE_MAX_K = 32   # line_maps' model terms are host products


# ---- weights -----------------------------------------------------------------------------------------------------------------------
def _range(r, n, what):
    try:
        lo, hi = r
        if lo != int(lo) or hi != int(hi):
            raise TypeError
        lo, hi = int(lo), int(hi)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a half-open range of channel indices (lo, hi), not {r!r}") from None
    if not 0 <= lo < hi <= n:
        raise ValueError(f"{what}: ({lo}, {hi}) is not a range 0 <= lo < hi <= {n}")
    return lo, hi


def _channels(n):
    if n != int(n) or int(n) < 1:
        raise ValueError(f"n = {n!r} channels")
    return int(n)


def window_weights(n, windows):
    """(g, n) float64 of 0 / 1: row q is 1 on the channels lo .. hi - 1 of ``windows[q] = (lo, hi)``, 0 <= lo < hi <= n.  The windows
    may overlap (every row stands alone)."""
    n = _channels(n)
    windows = list(windows)
    if not windows:
        raise ValueError("window_weights: no window")
    U = np.zeros((len(windows), n))
    for q, r in enumerate(windows):
        lo, hi = _range(r, n, f"window {q}")
        U[q, lo:hi] = 1.0
    return U


def line_weights(n, integration, background=None):
    """(n,) float64: the weight vector u whose sum over the channels, sum_c u_c x_c, is the net intensity of a line.  The module's own
    definition (not exspy's code):

    * u = 1 on the integration window I = (lo, hi), a half-open range of channel indices of width w_I = hi - lo;
    * with ``background = ((l0, l1), (r0, r1))``, two windows L and R of widths w_L, w_R: the background per channel is the mean
      count per channel of L and of R, interpolated linearly between the windows' centres at the centre of I, and it is subtracted
      w_I times: u -= w_I ((1 - s) 1_L / w_L + s 1_R / w_R), s = (c_I - c_L) / (c_R - c_L), with the centres c = (lo + hi - 1) / 2.
      s outside [0, 1] extrapolates (both windows on one side of the line); c_L == c_R raises ValueError.  The windows may overlap
      each other and I.

    A flat spectrum has net 0 and so has one that is linear in the channel index (the interpolation is exact for it)."""
    n = _channels(n)
    lo, hi = _range(integration, n, "integration window")
    u = np.zeros(n)
    u[lo:hi] = 1.0
    if background is None:
        return u
    try:
        left, right = background
    except (TypeError, ValueError):
        raise ValueError("background: two windows ((l0, l1), (r0, r1))") from None
    (l0, l1), (r0, r1) = _range(left, n, "left background window"), _range(right, n, "right background window")
    cI, cL, cR = (lo + hi - 1) / 2, (l0 + l1 - 1) / 2, (r0 + r1 - 1) / 2
    if cL == cR:
        raise ValueError(f"background: both windows are centred at channel {cL}: nothing to interpolate between")
    s = (cI - cL) / (cR - cL)
    wI = float(hi - lo)
    u[l0:l1] -= wI * (1.0 - s) / (l1 - l0)
    u[r0:r1] -= wI * s / (r1 - r0)
    return u


def label_weights(labels, n_regions=None):
    """(L, p) float64, one-hot: row r is 1 on the pixels with ``labels == r``.  ``labels``: integers, any shape (flattened in C order);
    negative labels belong to no region.  ``n_regions``: L, by default the largest label + 1; a region without a pixel is a row of
    zeros."""
    lab = np.asarray(labels)
    if lab.dtype.kind not in "iub":
        raise ValueError(f"labels must be integers, not {lab.dtype}")
    lab = lab.reshape(-1).astype(np.int64)
    if lab.size == 0:
        raise ValueError("labels: no pixel")
    top = int(lab.max())
    L = top + 1 if n_regions is None else int(n_regions)
    if L < 1 or top >= L:
        raise ValueError(f"labels up to {top} in {L} regions" if L >= 1 else "labels: no region (all negative)")
    W = np.zeros((L, lab.size))
    keep = np.nonzero(lab >= 0)[0]
    W[lab[keep], keep] = 1.0
    return W


# ---- the sums ----------------------------------------------------------------------------------------------------------------------
def _weights(W, m, axis, who):
    W = np.asarray(W, dtype=np.float64)
    if W.ndim == 1:
        W = W[None, :]
    if W.ndim != 2 or W.shape[0] < 1 or W.shape[1] != m:
        raise ValueError(f"{who}: weights of shape {W.shape} for {m} {axis} (one row of {m} per group)")
    if not np.isfinite(W).all():
        raise ValueError(f"{who}: the weights hold values that are not finite")
    return np.ascontiguousarray(W)


def _sums(X, weights, D, H, log_shift, layout, pixel_side, who):
    """(xs, ys, dev), each (g, p) for the pixel side and (g, n) for the channel side; ys and dev None without a model."""
    check_layout(layout)
    X = check_image(X)
    if (D is None) != (H is None):
        raise ValueError(f"{who}: a model is D and H together")
    if D is not None:
        n, p, k, D, H = check_model(D, H, who, MAX_K, tuple(X.shape), layout)
        check_log_shift(log_shift)
    else:
        (n, p), k = image_dims(X.shape, layout), 0
    W = _weights(weights, n if pixel_side else p, "channels" if pixel_side else "pixels", who)
    X = narrowed_image(X, who)
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    img = _image.Resident(X, layout).upload()
    dev = img.dev
    side = _lib.MARG_PIXELS if pixel_side else _lib.MARG_CHANNELS
    g, m = W.shape[0], (p if pixel_side else n)
    xs = np.empty((g, m))
    ys, dv = (np.empty((g, m)), np.empty((g, m))) if k else (None, None)
    with img.scope():
        Dd, Hd = img.model(D, H)
        need = int(_lib.lib.espm_weighted_marginals_scratch(side, n, p, min(g, MAX_G)))
        scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        for b in range(0, g, MAX_G):
            Wd = torch.from_numpy(W[b:b + MAX_G]).to(dev)
            gb = int(Wd.shape[0])
            out = [torch.empty((gb, m), dtype=torch.float64, device=dev) for _ in range(3 if k else 1)] + [None, None]
            _lib.check(_lib.lib.espm_weighted_marginals(*img.abi(), side, _ptr(Wd), gb, _ptr(Dd), _ptr(Hd), k, float(log_shift), _ptr(out[0]),
                                                        _ptr(out[1]), _ptr(out[2]), _ptr(scratch), need, _stream()))
            xs[b:b + gb] = out[0].cpu().numpy()
            if k:
                ys[b:b + gb], dv[b:b + gb] = out[1].cpu().numpy(), out[2].cpu().numpy()
    return xs, ys, dv


def pixel_maps(X, weights, D=None, H=None, log_shift=1e-14, layout="cm"):
    """Maps: for every row u of ``weights`` (g, n) - weights over the channels - and every pixel j, dict(

    * ``counts`` (g, p): sum_c u_c x_cj,
    * ``model`` (g, p): sum_c u_c Y_cj, Y = max(D H, log_shift),
    * ``deviance`` (g, p): 2 sum_c u_c (x ln(x / Y) - x + Y), the first term 0 where x == 0).

    ``model`` and ``deviance`` are None without a model (D and H None): then only the channels with a weight are read, and a zero
    entry costs its read only.  X: the image as measured, (channels, pixels) for ``layout="cm"`` or (pixels, channels) for "pm", a
    host array or a device tensor; 8- and 16-bit counts, float32 and float64 are read as they are, other integers narrowed where
    they fit.  D (n, k), H (k, p): 1 .. 8 components (NotImplementedError beyond).  Any number of weight vectors (8 per launch).
    ValueError for shapes that do not match, weights or X that are not finite - all before anything is uploaded.  The channels are
    added in ascending order in fp64 without atomics: two calls and both layouts give the same bits, and ``counts`` of integer X
    under integer weights is exact while sum |u| x < 2^53."""
    xs, ys, dv = _sums(X, weights, D, H, log_shift, layout, True, "pixel_maps")
    return dict(counts=xs, model=ys, deviance=dv)


def channel_spectra(X, weights, D=None, H=None, log_shift=1e-14, layout="cm"):
    """Spectra: for every row v of ``weights`` (L, p) - weights over the pixels: a one-hot label map (``label_weights``), a mask, or
    soft weights such as abundances - and every channel c, dict(

    * ``counts`` (n, L): sum_j v_j x_cj, the measured spectrum of the region,
    * ``model`` (n, L): sum_j v_j Y_cj, what the model predicts for it,
    * ``deviance`` (n, L): 2 sum_j v_j (x ln(x / Y) - x + Y), its residual spectrum).

    Arguments, refusals and guarantees as for ``pixel_maps``; the pixels are added in ascending order inside chunks of 2048 and the
    chunks in ascending order.  With one region of all pixels the three are ``measures.spectral_diagnostics``' ``sum_spectrum``,
    ``model_spectrum`` and ``channel_deviance``, bit for bit."""
    xs, ys, dv = _sums(X, weights, D, H, log_shift, layout, False, "channel_spectra")
    t = np.ascontiguousarray
    return dict(counts=t(xs.T), model=None if ys is None else t(ys.T), deviance=None if dv is None else t(dv.T))


def line_maps(X, lines, D=None, H=None, layout="cm"):
    """Elemental line maps with their Poisson error bars.  ``lines``: a list of ``(integration, background)``, each as for
    ``line_weights`` (``background`` None: the raw window); U (g, n) are their weight vectors.  Returns dict(

    * ``weights`` (g, n): U,
    * ``net`` (g, p): sum_c U_qc x_cj, the measured net counts of line q in pixel j - ``pixel_maps(X, U)["counts"]``,
    * ``net_std`` (g, p): sqrt(sum_c U_qc^2 x_cj), the standard deviation of ``net`` for Poisson counts (the plug-in estimate: x for
      its own variance) - the same pass with the weights squared,
    * ``model_net`` (g, p) = (U D) H and ``components`` (g, k, p), components[q, i, j] = (U D)_qi H_ij: what the model D (n, k),
      H (k, p) predicts for the line and every component's share of it, to hold next to ``net``; None without a model).

    The model terms are linear in the UNFLOORED model D H and are small host products in fp64 - no pass over X - so any k up to 32
    works here.  X, ``layout`` and the refusals as for ``pixel_maps``."""
    check_layout(layout)
    X = check_image(X)
    if (D is None) != (H is None):
        raise ValueError("line_maps: a model is D and H together")
    n, p = image_dims(X.shape, layout)
    if D is not None:
        n, p, k, D, H = check_model(D, H, "line_maps", LINE_MAX_K, tuple(X.shape), layout)
    lines = list(lines)
    if not lines:
        raise ValueError("line_maps: no line")
    rows = []
    for q, line in enumerate(lines):
        try:
            integration, background = line
        except (TypeError, ValueError):
            raise ValueError(f"line {q}: (integration, background or None), not {line!r}") from None
        rows.append(line_weights(n, integration, background))
    U = np.stack(rows)
    g = U.shape[0]
    xs, _, _ = _sums(X, np.concatenate([U, U * U]), None, None, 1.0, layout, True, "line_maps")
    out = dict(weights=U, net=np.ascontiguousarray(xs[:g]), net_std=np.sqrt(np.maximum(xs[g:], 0.0)), model_net=None, components=None)
    if D is not None:
        UD = U @ D
        out["model_net"] = UD @ H
        out["components"] = UD[:, :, None] * H[None, :, :]
    return out
