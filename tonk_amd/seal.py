"""Seal and open of Tonk datagrams in the caller's own device memory (include/tonk_seal.h).

`DatagramSealer` owns the keys of `n_streams` connections on one MI355X.  Its methods take a device
pointer (an int, e.g. a torch tensor's data_ptr()) and numpy index arrays, and return numpy arrays:
datagram i of a call lives at `dev + i * pitch`, any alignment, and is ciphered and tagged (seal),
or tag-checked and deciphered (open), in place -- bit for bit what Tonk's SimpleCipher does.
Per-datagram result codes: 0 done, 1 invalid (nothing touched), 2 bad tag (open; nothing touched).
A call the library refuses as a whole (a stream id out of range, a pitch below the largest
datagram, a device error) raises RuntimeError with tamd_seal_error's text.  Every call is
synchronous.  seal reads the timestamp and flags from the datagram: write them before the call.
"""
from __future__ import annotations

import ctypes

from . import lib as _lib_loader

FOOTER_BYTES = 24  # TAMD_SEAL_FOOTER_BYTES
OK, INVALID, BAD_TAG = 0, 1, 2

_bound = False
_u32p, _u64p, _i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32)
_u16p, _u8p = ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint8)
_REFUSED = {-1: "bad handle or null pointer", -2: "stream id out of range", -3: "pitch smaller than the largest datagram",
            -4: "device error"}


class _Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("max_datagram_bytes", ctypes.c_uint32)]


def _lib() -> ctypes.CDLL:
    global _bound
    L = _lib_loader()
    if not _bound:
        vp, u32, u64, cp, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t
        L.tamd_seal_create.restype = vp
        L.tamd_seal_create.argtypes = [ctypes.POINTER(_Params), cp, sz]
        L.tamd_seal_destroy.restype = None
        L.tamd_seal_destroy.argtypes = [vp]
        L.tamd_seal_error.restype = cp
        L.tamd_seal_error.argtypes = [vp]
        for name, args in (
                ("tamd_seal_set_key", [vp, u32, u64]),
                ("tamd_seal_seal", [vp, u32, _u32p, _u64p, _u32p, _u32p, vp, u64, _i32p]),
                ("tamd_seal_open", [vp, u32, _u32p, _u64p, _u32p, _u32p, vp, u64, _i32p]),
                ("tamd_seal_cipher", [vp, u32, _u32p, _u64p, _u32p, vp, u64]),
                ("tamd_seal_tag", [vp, u32, _u32p, _u64p, _u32p, vp, u64, _u16p]),
                ("tamd_seal_footers", [vp, u32, _u32p, vp, u64, _u8p])):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = args
        L.tamd_seal_set_timing.restype = None
        L.tamd_seal_set_timing.argtypes = [vp, ctypes.c_int]
        L.tamd_seal_kernel_ms.restype = None
        L.tamd_seal_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_uint]
        _bound = True
    return L


def _arr(a, dtype):
    import numpy as np
    return np.ascontiguousarray(a, dtype=dtype)


class DatagramSealer:
    """The keys of `n_streams` connections and the calls that seal and open their datagrams on the
    device.  Raises RuntimeError when no gfx950 device is usable or the parameters are bad."""

    KERNEL_MS_FIELDS = ("packets_ms", "footers_ms", "packets_launches", "footers_launches")
    _h = None

    def __init__(self, n_streams: int, max_datagram_bytes: int, device: int = 0):
        if not (0 < int(n_streams) < 2**32 and 0 < int(max_datagram_bytes) <= 65535):
            raise RuntimeError("tonk_amd: DatagramSealer: bad parameters")
        p = _Params(int(device), int(n_streams), int(max_datagram_bytes))
        err = ctypes.create_string_buffer(512)
        self.n_streams, self.max_datagram_bytes = int(n_streams), int(max_datagram_bytes)
        self._h = _lib().tamd_seal_create(ctypes.byref(p), err, len(err))
        if not self._h:
            raise RuntimeError(f"tonk_amd: DatagramSealer creation failed: {err.value.decode()}")

    def _check(self, rc: int, what: str) -> None:
        if rc < 0:
            err = _lib().tamd_seal_error(self._h).decode()
            raise RuntimeError(f"tonk_amd: {what} refused (rc={rc}: {_REFUSED.get(rc, '?')}){': ' + err if err else ''}")

    def set_key(self, stream: int, key: int) -> None:
        """SimpleCipher::Initialize of one stream; takes effect with the next call."""
        self._check(_lib().tamd_seal_set_key(self._h, int(stream), int(key) & 0xFFFFFFFFFFFFFFFF), "set_key")

    def _datagrams(self, fn, what, stream, nonce, nbytes, message_bytes, dev: int, pitch: int):
        import numpy as np
        S, N, B, M = _arr(stream, np.uint32), _arr(nonce, np.uint64), _arr(nbytes, np.uint32), _arr(message_bytes, np.uint32)
        assert S.size == N.size == B.size == M.size
        rc = np.zeros(S.size, dtype=np.int32)
        self._check(fn(self._h, S.size, S.ctypes.data_as(_u32p), N.ctypes.data_as(_u64p), B.ctypes.data_as(_u32p),
                       M.ctypes.data_as(_u32p), dev, pitch, rc.ctypes.data_as(_i32p)), what)
        return rc

    def seal(self, stream, nonce, nbytes, message_bytes, dev_datagrams: int, pitch: int):
        """Cipher the first message_bytes[i] bytes of every datagram and write its tag; returns the result codes."""
        return self._datagrams(_lib().tamd_seal_seal, "seal", stream, nonce, nbytes, message_bytes, dev_datagrams, pitch)

    def open(self, stream, nonce, nbytes, message_bytes, dev_datagrams: int, pitch: int):
        """Check every datagram's tag and decipher those that match; returns the result codes."""
        return self._datagrams(_lib().tamd_seal_open, "open", stream, nonce, nbytes, message_bytes, dev_datagrams, pitch)

    def cipher(self, stream, nonce, nbytes, dev_data: int, pitch: int) -> None:
        """Cipher over nbytes[i] bytes of every entry, in place."""
        import numpy as np
        S, N, B = _arr(stream, np.uint32), _arr(nonce, np.uint64), _arr(nbytes, np.uint32)
        assert S.size == N.size == B.size
        self._check(_lib().tamd_seal_cipher(self._h, S.size, S.ctypes.data_as(_u32p), N.ctypes.data_as(_u64p),
                                            B.ctypes.data_as(_u32p), dev_data, pitch), "cipher")

    def tag(self, stream, nonce, nbytes, dev_data: int, pitch: int):
        """Plain Tag() of nbytes[i] bytes of every entry; returns the tags (uint16)."""
        import numpy as np
        S, N, B = _arr(stream, np.uint32), _arr(nonce, np.uint64), _arr(nbytes, np.uint32)
        assert S.size == N.size == B.size
        out = np.zeros(S.size, dtype=np.uint16)
        self._check(_lib().tamd_seal_tag(self._h, S.size, S.ctypes.data_as(_u32p), N.ctypes.data_as(_u64p),
                                         B.ctypes.data_as(_u32p), dev_data, pitch, out.ctypes.data_as(_u16p)), "tag")
        return out

    def footers(self, nbytes, dev_datagrams: int, pitch: int):
        """The last min(nbytes[i], 24) bytes of every datagram, right-aligned and zero-filled: an (n, 24) uint8 array."""
        import numpy as np
        B = _arr(nbytes, np.uint32)
        out = np.zeros((B.size, FOOTER_BYTES), dtype=np.uint8)
        self._check(_lib().tamd_seal_footers(self._h, B.size, B.ctypes.data_as(_u32p), dev_datagrams, pitch,
                                             out.ctypes.data_as(_u8p)), "footers")
        return out

    def set_timing(self, on: bool) -> None:
        _lib().tamd_seal_set_timing(self._h, 1 if on else 0)

    def kernel_ms(self) -> dict:
        """Device time and launches of the two kernels since the last call."""
        out = (ctypes.c_double * 4)()
        _lib().tamd_seal_kernel_ms(self._h, out, 4)
        return dict(zip(self.KERNEL_MS_FIELDS, [float(v) for v in out]))

    def close(self) -> None:
        if self._h:
            _lib().tamd_seal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
