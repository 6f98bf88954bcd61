"""A stand-in for ``muygpys_amd._lib.fn`` that stops every call at the library boundary (CPU tests).

``install(monkeypatch)`` puts a :class:`Recorder` in the place of ``_lib.fn`` and stands in for the few things that need
a device -- the device check, the stream, the LOOCV scratch, the once-per-process tree self-check, pinned memory.  CPU
tensors have a ``data_ptr()``, so the marshalling of the Python functions runs for real; host functions of the library
(``mgp_packed_row_bytes``, the ``*_workspace_bytes`` queries ...) are the library's own."""

import ctypes as C

import torch

from muygpys_amd import _abi, _lib, fused

STREAM = 0x5151


class Recorder:
    """Stands in for ``_lib.fn``: notes (base, dtype, args) of every call and answers with the status queued for
    that entry point (0 when none is)."""

    def __init__(self, statuses=None):
        self.calls = []
        self.statuses = {k: list(v) for k, v in (statuses or {}).items()}

    def fn(self, base, dtype):
        def call(*args):
            self.calls.append((base, dtype, args))
            queue = self.statuses.get(base)
            return queue.pop(0) if queue else 0

        call.argtypes = _abi.signatures()[f"mgp_{base}_{_lib.suffix(dtype)}"][1]
        return call

    def of(self, *skip):
        """The calls made, without the table packs (or whatever else is named)."""
        return [c for c in self.calls if c[0] not in ("table_pack",) + skip]


def install(monkeypatch) -> Recorder:
    """A fresh recorder behind ``_lib.fn`` for the length of ``monkeypatch``; the caches of ``fused`` start empty."""
    r = Recorder()
    _lib.load()
    monkeypatch.setattr(_lib, "fn", r.fn)
    monkeypatch.setattr(_lib, "require_cuda", lambda *tensors: None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: C.c_void_p(STREAM))
    monkeypatch.setattr(_lib, "raw_stream", lambda: STREAM)
    monkeypatch.setattr(_lib, "loocv_scratch", lambda device, b=0: torch.zeros(64, dtype=torch.uint8))
    monkeypatch.setattr(_lib, "loocv_tree_selfcheck", lambda *a, **k: True)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)  # (LoocvPlan: pinned host words; no device here)
    fused.clear_caches()
    return r


def val(a):
    """A recorded argument as a plain value: pointers as integers (NULL: None), numbers as numbers."""
    return a.value if isinstance(a, C._SimpleCData) else a


def vals(call):
    return [val(a) for a in call[2]]
