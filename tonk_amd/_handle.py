"""What the classes over the batched device interfaces share (batch.py, seal.py, dgram.py, cbatch.py): the
ctypes prototypes of an interface bound once, the array marshalling, and the base class that owns a
library handle -- creation, refusals, kernel timing and release.  The library's side of this is
tonk_amd/csrc/handle.h."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

from . import lib as _lib_loader

vp, u32, u64, cp, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t
u8p, u16p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint32)
u64p, i32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32)

_bound = {}
_np = None  # numpy, imported at the first call that marshals an array


def bind(L: ctypes.CDLL, prefix: str, calls: dict) -> SimpleNamespace:
    """Set restype and argtypes of {prefix}_create/destroy/error/set_timing/kernel_ms and of the
    int-returning `calls` (name after the prefix -> argtypes), once per prefix; returns the
    functions under their names after the prefix."""
    if prefix not in _bound:
        protos = {"create": (vp, [vp, cp, sz]), "destroy": (None, [vp]), "error": (cp, [vp]),
                  "set_timing": (None, [vp, ctypes.c_int]),
                  "kernel_ms": (None, [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_uint])}
        protos.update({name: (ctypes.c_int, args) for name, args in calls.items()})
        fns = {name: getattr(L, f"{prefix}_{name}") for name in protos}
        for name, (res, args) in protos.items():
            fns[name].restype, fns[name].argtypes = res, args
        _bound[prefix] = SimpleNamespace(**fns)
    return _bound[prefix]


def _numpy():
    global _np
    import numpy
    _np = numpy
    return numpy


def arr(a, dtype: str):
    """`a` as a contiguous numpy array of the dtype named."""
    np = _np or _numpy()
    return np.ascontiguousarray(a, dtype=getattr(np, dtype))


def zeros(shape, dtype: str):
    """A result array for the library to fill."""
    np = _np or _numpy()
    return np.zeros(shape, dtype=getattr(np, dtype))


def ptr(a, t):
    """The array's data as pointer type `t`; None stays None."""
    return None if a is None else a.ctypes.data_as(t)


class Handle:
    """A library handle of the interface `_PREFIX`, whose calls beside the common five are `_CALLS`
    (reached as self._c.<name>); `_REFUSED` names its negative return codes, `KERNEL_MS_FIELDS`
    what kernel_ms returns; `_LIB` is the library's path when it is not the engine's."""

    _PREFIX, _CALLS, _REFUSED, KERNEL_MS_FIELDS, _LIB = "", {}, {}, (), None
    _h = _c = None

    @classmethod
    def _bind(cls) -> SimpleNamespace:
        return bind(_lib_loader(cls._LIB), cls._PREFIX, cls._CALLS)

    def _create(self, params: ctypes.Structure) -> None:
        self._c = self._bind()
        err = ctypes.create_string_buffer(512)
        self._h = self._c.create(ctypes.byref(params), err, len(err))
        if not self._h:
            raise RuntimeError(f"tonk_amd: {type(self).__name__} creation failed: {err.value.decode()}")

    def _check(self, rc: int, what: str) -> None:
        if rc < 0:
            err = self._c.error(self._h).decode()
            raise RuntimeError(f"tonk_amd: {what} refused (rc={rc}: {self._REFUSED.get(rc, '?')}){': ' + err if err else ''}")

    def set_timing(self, on: bool) -> None:
        self._c.set_timing(self._h, 1 if on else 0)

    def kernel_ms(self) -> dict:
        """Device time and launches of the interface's kernels since the last call."""
        out = (ctypes.c_double * len(self.KERNEL_MS_FIELDS))()
        self._c.kernel_ms(self._h, out, len(out))
        return dict(zip(self.KERNEL_MS_FIELDS, [float(v) for v in out]))

    def close(self) -> None:
        if self._h:
            self._c.destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
