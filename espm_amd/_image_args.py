"""What the analyses of an image ask of their arguments before anything is uploaded (binning, splitting, sampling, attribution and
the diagnostics of measures): the layout of X and the shapes of a model D H against it.  Host only; nothing here touches the device."""
from __future__ import annotations

import numpy as np


def check_layout(layout):
    if layout not in ("cm", "pm"):
        raise ValueError(f"layout must be 'cm' ((channels, pixels)) or 'pm' ((pixels, channels)), not {layout!r}")


def layout_code(layout):
    """ESPM_LAYOUT_CM or ESPM_LAYOUT_PM of a checked layout."""
    from espm_amd import _lib
    check_layout(layout)
    return _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM


def image_dims(shape, layout):
    """(n, p) of a 2-D X of this shape."""
    return (int(shape[0]), int(shape[1])) if layout == "cm" else (int(shape[1]), int(shape[0]))


def check_model(D, H, who, max_k, X_shape=None, layout="cm"):
    """(n, p, k, D, H) after every check of the shapes, D (n, k) and H (k, p) as C-contiguous fp64 host arrays.  ``X_shape``: the
    image the model stands against (None: n and p are the model's own).  ValueError for shapes that do not match,
    NotImplementedError (``who``: ...) for more than ``max_k`` components."""
    check_layout(layout)
    if X_shape is not None and (len(X_shape) != 2 or X_shape[0] < 1 or X_shape[1] < 1):
        raise ValueError("X must be a non-empty 2-D array or tensor")
    D, H = np.ascontiguousarray(D, dtype=np.float64), np.ascontiguousarray(H, dtype=np.float64)
    if D.ndim != 2 or H.ndim != 2 or D.shape[1] != H.shape[0] or D.size == 0 or H.size == 0:
        raise ValueError("D must be (channels, components) and H (components, pixels), both non-empty")
    n, p = image_dims(X_shape, layout) if X_shape is not None else (int(D.shape[0]), int(H.shape[1]))
    k = int(D.shape[1])
    if D.shape[0] != n:
        raise ValueError(f"X has {n} channels, D has {D.shape[0]}")
    if H.shape[1] != p:
        raise ValueError(f"X has {p} pixels, H has {H.shape[1]}")
    if k > max_k:
        raise NotImplementedError(f"{who}: {k} components (the kernels are built for 1..{max_k})")
    return n, p, k, D, H
