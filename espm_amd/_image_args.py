"""What the analyses of an image ask of their arguments before anything is uploaded (binning, splitting, sampling, attribution,
marginals, residuals, presence and the diagnostics of measures): that X is an image, its layout, the shapes of a model D H against
it, ``log_shift`` and ``seed``, and the three rules for the dtype X goes up in.  Host only: no torch at import, and nothing here
uploads (``espm_amd/_image.py`` is the device half)."""
from __future__ import annotations

import sys

import numpy as np

MAX_COUNT = 65535   # the largest count of the 16-bit kernels


def is_tensor(v):
    """Whether v is a torch tensor, without importing torch where nobody has."""
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(v, torch.Tensor)


def _dtype_name(dt):
    """('uint8', 'float32', ...) of a numpy dtype or scalar type or of a torch dtype, and whether it is torch's."""
    s = str(dt)
    return (s[len("torch."):], True) if s.startswith("torch.") else (np.dtype(dt).name, False)


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


def check_image(X):
    """X, a non-empty 2-D array or tensor (through ``np.asarray`` when it has no ``ndim``)."""
    if getattr(X, "ndim", None) is None:
        X = np.asarray(X)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be a non-empty 2-D array or tensor")
    return X


def check_log_shift(log_shift):
    if not log_shift > 0:
        raise ValueError("log_shift must be positive")
    return float(log_shift)


def check_seed(seed):
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an integer in 0 .. 2^64 - 1, not {seed!r}")
    return int(seed)


def check_model(D, H, who, max_k, X_shape=None, layout="cm"):
    """(n, p, k, D, H) after every check of the shapes, D (n, k) and H (k, p) as C-contiguous fp64 host arrays.  ``X_shape``: the
    shape of the checked image the model stands against (None: n and p are the model's own).  ValueError for shapes that do not
    match, NotImplementedError (``who``: ...) for more than ``max_k`` components."""
    check_layout(layout)
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


# ---- the dtype X goes up in: three rules, each named by the analyses that use it -------------------------------------------------
def measured_dtype(dt):
    """The as-measured rule (the diagnostics, binning, ``attribution.expected``): the dtype an X of the numpy or torch dtype ``dt``
    is read in on the device, as a numpy dtype - u8, u16, f32 and f64 as they are, the others as f32 or f64, whichever holds every
    value exactly (64-bit integers: f64, exact up to 2^53).  TypeError for a host dtype that holds no numbers."""
    name, of_torch = _dtype_name(dt)
    if name in ("uint8", "uint16", "float32", "float64"):
        return np.dtype(name)
    if name == "bool":
        return np.dtype(np.uint8)
    if name in ("int8", "int16", "float16"):
        return np.dtype(np.float32)
    if of_torch or np.dtype(dt).kind in "iuf":
        return np.dtype(np.float64)
    raise TypeError(f"X of dtype {dt} is not an image of counts")


def narrowed_image(X, who):
    """The narrowing rule (marginals, residuals, presence): X as it goes to the device - 8- and 16-bit counts, float32 and float64
    as they are; other integer dtypes narrowed to uint8 or uint16 where the values allow (else as ``measured_dtype`` says);
    ValueError for negative integers and for values that are not finite - a NaN under a zero weight would be skipped and elsewhere
    poison its sums.  Host arrays are checked on the host, before anything is uploaded; device tensors where they are."""
    if is_tensor(X):
        if X.dtype.is_floating_point and not bool(X.isfinite().all()):
            raise ValueError(f"{who}: X holds values that are not finite")
        return X
    X = np.asarray(X)
    if X.dtype.kind == "f":
        if not np.isfinite(X).all():
            raise ValueError(f"{who}: X holds values that are not finite")
    elif X.dtype.kind in "iu" and X.dtype not in (np.uint8, np.uint16):
        lo, hi = int(X.min()), int(X.max())
        if lo < 0:
            raise ValueError(f"{who}: X holds values from {lo} to {hi}: counts are not negative")
        if hi <= MAX_COUNT:
            X = X.astype(np.uint8 if hi <= 255 else np.uint16)
    elif X.dtype.kind not in "iub":
        raise TypeError(f"{who}: X of dtype {X.dtype} is not an image of counts")
    return X


def counts_image(X, layout):
    """The counts-only rule (thinning, ``split_deviance``, ``attribution.assign``): X as the kernels read it - a host array or a
    tensor of uint8 / uint16 - and (n, p): TypeError for an X that is no image of counts, ValueError for values outside
    0 .. 65535.  Nothing is uploaded here."""
    check_layout(layout)
    X = check_image(X)
    is_t = is_tensor(X)
    integer = (not (X.dtype.is_floating_point or X.dtype.is_complex)) if is_t else X.dtype.kind in "iub"
    if not integer:
        raise TypeError(f"thinning is defined for counts: X has dtype {X.dtype} (an integer dtype with values 0 .. {MAX_COUNT})")
    n, p = image_dims(X.shape, layout)
    if _dtype_name(X.dtype)[0] in ("uint8", "uint16"):
        return X, n, p
    if is_t:
        import torch
        wide = X.to(torch.int64) if X.dtype != torch.bool else X.to(torch.uint8)
        lo, hi = int(wide.min().item()), int(wide.max().item())
    else:
        lo, hi = int(X.min()), int(X.max())
    if lo < 0 or hi > MAX_COUNT:
        raise ValueError(f"X holds values from {lo} to {hi}: counts are 0 .. {MAX_COUNT}")
    if is_t:
        return X.to(torch.uint8 if hi <= 255 else torch.uint16), n, p
    return X.astype(np.uint8 if hi <= 255 else np.uint16), n, p
