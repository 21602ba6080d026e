"""What every Python owner of a ``libhificar.so`` handle shares: the handle's lifecycle — ``NativeOwner`` — and the
small idioms around a native call: ``create_handle``, the grow-only ``scratch`` buffer, the one-shot ``aligned`` allocation and
``current_stream``.  A new owner is a subclass with a destroy entry point's name and its per-process fields; how and when it creates and
invalidates its handle, and every message, stay its own."""

import ctypes

import torch

from . import _native

ABSENT = object()  # the idle value of a field that is not in ``__dict__`` at all while idle (read with ``__dict__.get``)


def current_stream():
    """torch's current stream on the current device, as the C ABI takes it."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _align(t):
    off = (-t.data_ptr()) % 256
    return t.data_ptr() + off, t.numel() * t.element_size() - off


def aligned(nbytes, device, dtype=torch.uint8):
    """(tensor, pointer): a one-shot allocation with at least ``nbytes`` bytes from ``pointer``, its first 256-byte boundary.  The tensor
    has ``nbytes`` plus 256 bytes in elements of ``dtype`` (float32: ``nbytes // 4 + 64`` floats, for owners that slice it as floats)."""
    size = dtype.itemsize
    t = torch.empty(nbytes // size + 256 // size, dtype=dtype, device=device)
    return t, _align(t)[0]


def scratch(owner, attr, nbytes, device):
    """(pointer, bytes) of the grow-only scratch buffer kept in ``owner.<attr>``: at least ``nbytes`` bytes from a 256-byte boundary.
    ``device``: where the buffer lives — one found elsewhere is replaced — or a callable that says so, asked only when a buffer is
    allocated (an owner that drops its buffers itself whenever its parameters move)."""
    n = nbytes + 256
    ws = getattr(owner, attr)
    if ws is None or ws.numel() < n or not (callable(device) or ws.device == device):
        # work already enqueued on the old buffer keeps it alive through the caching allocator's stream ordering
        ws = torch.empty(int(n * 1.25) if ws is not None else n, dtype=torch.uint8, device=device() if callable(device) else device)
        setattr(owner, attr, ws)
    return _align(ws)


def create_handle(lib, prefix, make, state, finalize):
    """A finished handle: ``make(handle)`` creates it, every tensor of ``state`` ({name: fp32 CPU tensor}) goes through
    ``<prefix>_set_weight``, ``finalize(handle)`` ends the creation.  Whatever raises after ``make``, the handle is destroyed first."""
    handle = ctypes.c_void_p()
    make(handle)
    try:
        what = prefix + "_set_weight"
        for name, t in state.items():
            shape = (ctypes.c_int64 * t.dim())(*t.shape)
            _native.check(getattr(lib, what)(handle, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()), what)
        finalize(handle)
    except Exception:
        getattr(lib, prefix + "_destroy")(handle)
        raise
    return handle


class NativeOwner:
    """Mixin (listed before ``torch.nn.Module``) of a module that owns one native handle in ``_handle``, made on first use by its own
    ``_native_handle``.  A handle is a raw pointer: it is destroyed exactly once, and copies and pickles — which skip ``__init__`` — never
    carry it, nor anything else of the two tables below.  ``__init__`` calls ``_reset_native()`` once the parameters exist."""

    _DESTROY = None              # the C destroy entry point's name
    _ENGINE = None               # the C engine accessor's name, where there is one
    _NATIVE = {"_handle": None}  # {field: idle value} of what is bound to the handle: ``_invalidate`` resets it
    _PROCESS = {"_lib": None}    # ... and of what outlives a handle but not the process: wiring, caches of the module's own tensors
    _WATCHED = False             # registered with utils.optim_hook: every optimizer.step() over the parameters calls invalidate_parameters()

    def _idle(self, table):
        d = self.__dict__  # (not setattr: torch's Module.__setattr__ may be half torn down when __del__ runs at interpreter exit)
        for k, v in table.items():
            if v is ABSENT:
                d.pop(k, None)
            else:
                d[k] = v.copy() if isinstance(v, dict) else v

    def _reset_native(self):
        self._idle(self._NATIVE)
        self._idle(self._PROCESS)
        if self._WATCHED:
            from .utils.optim_hook import watch

            watch(self)  # fused optimizers do not bump Parameter._version; a copy trains with its own optimizer

    def _invalidate(self):
        handle, lib = self.__dict__.get("_handle"), self.__dict__.get("_lib")
        self._idle(self._NATIVE)
        if handle is not None and lib is not None:
            getattr(lib, self._DESTROY)(handle)

    def __del__(self):
        try:
            self._invalidate()
        except Exception:
            pass

    def __getstate__(self):
        state = self.__dict__.copy()
        for k in (*self._NATIVE, *self._PROCESS):
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._reset_native()  # (also over a state that carries the fields as None, as earlier versions wrote them)

    def engine(self):
        """The engine handle for ``hificar_profile_begin`` / ``hificar_profile_end`` (per-kernel device times; tools/*_bench.py)."""
        handle = self._native_handle()  # first: it is what loads self._lib
        return ctypes.c_void_p(getattr(self._lib, self._ENGINE)(handle))
