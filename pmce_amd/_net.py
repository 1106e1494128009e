"""What the demo's device networks (extractor.py, vitpose.py, yolo.py; the selection also hmr.py) share on the host: the selection of a
state dict's tensors, and the shell around a handle of the library - its life, the upload and finalize of its weights
(csrc/net_weights.hpp), its workspace, the ``max_batch`` chunks of a forward and the finite check of a result.  Each network keeps its
tables, its checks and its one C call."""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _lib


PRECISIONS = ("split_f16", "f16")       # the library's precision 0 and 1 (include/pmce_hip.h: pmce_*_create_precision)


def check_precision(precision):
    """-> the library's number of a precision name; any other value raises a ValueError that lists the two choices."""
    if precision not in PRECISIONS:
        raise ValueError(f'precision must be "split_f16" or "f16" (got {precision!r})')
    return PRECISIONS.index(precision)


def clean_state_dict(sd, keep=None):
    """The entries of a state dict with an optional ``module.`` prefix stripped and ``num_batches_tracked`` dropped; ``keep(name)``
    filters the stripped names further."""
    if not hasattr(sd, "items"):
        raise ValueError(f"a state dict is a mapping of names to tensors (got {type(sd).__name__})")
    clean = {}
    for k, v in sd.items():
        k = k[len("module."):] if k.startswith("module.") else k
        if k.endswith("num_batches_tracked") or (keep is not None and not keep(k)):
            continue
        clean[k] = v
    return clean


def take_tensors(clean, required, dtype):
    """``required``: name -> shape.  -> the named tensors of ``clean`` as CPU tensors of ``dtype``, in ``required``'s order.  A missing or
    mis-shaped tensor raises a ValueError that names it."""
    out = OrderedDict()
    for name, shape in required.items():
        if name not in clean:
            raise ValueError(f"the state dict has no tensor '{name}' (expected shape {tuple(shape)})")
        t = torch.as_tensor(clean[name])
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"tensor '{name}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
        out[name] = t.detach().to(device="cpu", dtype=dtype)
    return out


class DeviceNetwork:
    """The shell of a network that lives behind a handle of the library.  A subclass names itself (``NAME``: the library's
    ``pmce_<NAME>_finalize_on`` and ``pmce_<NAME>_destroy`` are its symbols), gives the largest ``max_batch`` the library takes
    (``MAX_BATCH``), creates ``self._h`` after this constructor and hands its weights to ``_finalize``."""
    NAME = None
    MAX_BATCH = None

    def __init__(self, device, max_batch, check_finite):
        if int(max_batch) != max_batch or not 1 <= int(max_batch) <= self.MAX_BATCH:
            raise ValueError(f"max_batch must be a whole number in 1..{self.MAX_BATCH} (got {max_batch!r})")
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self.check_finite = bool(check_finite)
        self._ws = None
        self._h = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:        # (at interpreter exit the module globals are already cleared)
            getattr(_lib._lib, f"pmce_{self.NAME}_destroy")(h)

    def _finalize(self, uploads):
        """uploads: (set_call, host tensors) pairs; every tensor is uploaded as contiguous fp32 and ``set_call(*device pointers)`` hands
        them to the handle.  The uploads live until the library has packed them."""
        with torch.cuda.device(self.device):
            keep = []
            for set_call, tensors in uploads:
                dev = [t.to(self.device, torch.float32).contiguous() for t in tensors]
                keep.append(dev)
                set_call(*[_lib.ptr(d) for d in dev])
            torch.cuda.current_stream().synchronize()        # the uploads (pageable copies run on the legacy stream) are done
            _lib.check(getattr(_lib.load(), f"pmce_{self.NAME}_finalize_on")(self._h, _lib.current_stream()), f"{self.NAME}_finalize")
            del keep

    def _workspace(self, nbytes):
        """One fp32 tensor of at least ``nbytes`` (what the library's ``workspace_bytes`` returned: 0 is its error), kept and grown."""
        if nbytes == 0:
            raise _lib.PmceError(_lib.last_error())
        if self._ws is None or self._ws.numel() * 4 < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes // 4, device=self.device, dtype=torch.float32)
        return self._ws

    def _chunks(self, x):
        """x [n, ...] (a host tensor is uploaded; any strides) -> (i0, m, x[i0:i0 + m], its strides) for ``max_batch`` items at a time."""
        x = x.to(self.device)
        if any(s < 1 for s in x.stride()):
            x = x.contiguous()
        for i0 in range(0, x.shape[0], self.max_batch):
            xi = x[i0:i0 + self.max_batch]
            yield i0, xi.shape[0], xi, xi.stride()

    def _require_finite(self, t, noun, what):
        """With ``check_finite``: raise when an item of t [n, ...] is not finite, naming the first such item."""
        if self.check_finite and t.shape[0]:
            bad = ~torch.isfinite(t).reshape(t.shape[0], -1).all(dim=1)
            if bool(bad.any()):
                raise _lib.PmceError(f"{self.NAME}: {noun} {int(bad.nonzero()[0])} has non-finite {what} (an input that is not finite, or an "
                                     "activation beyond the f16 range of the matrix operands)")
