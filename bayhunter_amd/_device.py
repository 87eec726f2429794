"""Getting rows to the device and a library handle around them: what posterior, datafits and moho share of ctypes
and torch.  torch is imported inside the functions: the package imports without it."""
import ctypes as C

import numpy as np

from . import _lib


def torch_device(device):
    import torch
    if device is None:
        return torch.device('cuda', torch.cuda.current_device())
    if isinstance(device, int):
        return torch.device('cuda', device)
    return torch.device(device)


def to_device(a, dtype, dev):
    import torch
    if isinstance(a, torch.Tensor):
        t = a.to(device=dev, dtype=dtype)
    else:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)
    return t if t.dim() < 2 or t.stride(1) == 1 else t.contiguous()


def device_rows(models, weights=None, misfits=None, device=None, per_row="one weight and one misfit per row"):
    """`models` ([rows, 2*maxlayers], float32 or float64; numpy or a torch tensor) with one weight and one misfit per
    row, or None -> (dev, rows in their own float width, weights int32, misfits float64), all on `dev`.
    ValueError(per_row) when a count differs from the number of rows."""
    import torch
    dev = torch_device(device)
    if not isinstance(models, torch.Tensor):
        models = np.asarray(models)
    if models.ndim != 2:
        raise ValueError("models: [rows, 2*maxlayers]")
    fdtype = torch.float32 if str(models.dtype).endswith('float32') else torch.float64
    rows = to_device(models, fdtype, dev)
    w = None if weights is None else to_device(weights, torch.int32, dev)
    mf = None if misfits is None else to_device(misfits, torch.float64, dev)
    if w is not None and w.numel() != rows.shape[0] or mf is not None and mf.numel() != rows.shape[0]:
        raise ValueError(per_row)
    return dev, rows, w, mf


class Handle(object):
    """A library handle of bh_<kind>_create(*args, &handle): destroyed by close(), or on leaving its `with` block."""

    def __init__(self, kind, *args):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        self._destroy = getattr(self.lib, 'bh_%s_destroy' % kind)
        _lib.check(getattr(self.lib, 'bh_%s_create' % kind)(*(args + (C.byref(self.h),))))

    def close(self):
        if self.h:
            self._destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
