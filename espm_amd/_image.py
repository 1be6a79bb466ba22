"""The device half of an image argument (``espm_amd/_image_args.py`` is the host half): ``on_device``, the single place where an
image reaches the GPU; ``model_on_device`` for a host fp64 model; ``Resident``, a checked image that goes up once and is then read
by any number of passes; ``to_host``.  The analyses call these through the module (``_image.on_device(...)``), so that one
patched attribute shows whether anything was uploaded."""
from __future__ import annotations

import numpy as np

from espm_amd._image_args import image_dims, is_tensor, layout_code, measured_dtype

UPLOAD_ENTRIES = 16 << 20   # entries of a host X per upload step


def dtype_code(dtype):
    """ESPM_DIAG_X_* of the torch dtype of an image on the device."""
    import torch

    from espm_amd import _lib
    return {torch.uint8: _lib.DIAG_X_U8, torch.uint16: _lib.DIAG_X_U16, torch.float32: _lib.DIAG_X_F32,
            torch.float64: _lib.DIAG_X_F64}[dtype]


def on_device(X, device=None):
    """(Xd, dtype code, device): X on the GPU in the dtype ``measured_dtype`` gives it, with a row stride the kernels read.  A
    device tensor stays where it is (converted there only when its dtype needs it, copied only when its inner stride is not 1 or
    its rows overlap); a host array goes up in row chunks in its own dtype - no fp64 copy of the image, on either side.
    ``device``: where to, by default X's own device or the current one."""
    import torch

    from espm_amd.engine import require_gpu
    tensor = is_tensor(X)
    dev = require_gpu(device if device is not None else (X.device if tensor and X.is_cuda else None))
    with torch.cuda.device(dev):
        if tensor:
            Xd = X.to(dev)
            Xd = Xd.to(getattr(torch, measured_dtype(Xd.dtype).name))
            if Xd.stride(1) != 1 or Xd.stride(0) < Xd.shape[1]:
                Xd = Xd.contiguous()
        else:
            X = np.asarray(X)
            dt = measured_dtype(X.dtype)
            Xd = torch.empty(X.shape, dtype=getattr(torch, dt.name), device=dev)
            step = max(1, UPLOAD_ENTRIES // max(1, X.shape[1]))
            for a in range(0, X.shape[0], step):
                Xd[a:a + step].copy_(torch.from_numpy(np.ascontiguousarray(X[a:a + step], dtype=dt)))
    return Xd, dtype_code(Xd.dtype), dev


def model_on_device(dev, *arrays):
    """The host fp64 arrays of a model (D, H, or either; None stays None) as tensors on ``dev``.  A read-only array is copied on
    the host first (torch does not wrap those)."""
    import torch
    with torch.cuda.device(dev):
        return tuple(None if A is None else (torch.from_numpy(A) if A.flags.writeable else torch.tensor(A)).to(dev) for A in arrays)


def to_host(T):
    """A device tensor as a host array; a host array as it is."""
    return T.cpu().numpy() if is_tensor(T) else np.asarray(T)


class Resident:
    """An image, checked on the host by its caller, and its layout: ``upload()`` puts it on the GPU ONCE (``on_device``), and
    every pass after that reads the resident ``Xd``.  ``host`` is X until then and None afterwards."""

    def __init__(self, X, layout, device=None):
        self.layout = layout
        self.n, self.p = image_dims(X.shape, layout)
        self.host, self.Xd, self._device = X, None, device

    def upload(self):
        if self.Xd is None:
            self.Xd, self.code, self.dev = on_device(self.host, self._device)
            self.host = None
        return self

    def abi(self):
        """The six leading arguments of every entry point that reads an image: X, its dtype code, layout, row stride, n, p."""
        from espm_amd.engine import _ptr
        return _ptr(self.Xd), self.code, layout_code(self.layout), int(self.Xd.stride(0)), self.n, self.p

    def scope(self):
        """The context in which this image's device is the current one."""
        import torch
        return torch.cuda.device(self.dev)

    def model(self, *arrays):
        """``model_on_device`` on this image's device."""
        return model_on_device(self.dev, *arrays)
