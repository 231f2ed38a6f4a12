"""Building and parsing of Tonk datagrams in the caller's own device memory (include/tonk_datagram.h).

`DatagramFramer` holds no per-connection state.  `build` lays a tick's messages and footers out as
datagrams at `dev_out + i * pitch` (what Tonk's sendQueuedDatagram and PostRecovery write, short of
the cipher and the tag, which are `DatagramSealer.seal`'s); `parse` walks the frame headers of
deciphered message sections (ProcessDatagram's walk, or resumeProcessing's and onCompressed's with
`mode=1`) and returns where every message is and which span of the section is reliable.  Device
pointers are ints (e.g. a torch tensor's data_ptr()), lists are numpy arrays or sequences, results
numpy arrays.  A call the library refuses as a whole raises RuntimeError with tamd_dgram_error's
text.  Every call is synchronous.
"""
from __future__ import annotations

import ctypes

from . import lib as _lib_loader

HANDSHAKE_BYTES = 12
TYPE_RAW = 255          # build: the headerless body of an OnlyFEC datagram
SEQCOMP, ONLYFEC = 0x20, 0x10
OK, INVALID, TRUNCATED, BAD_FRAME, BAD_ACKACK = 0, 1, 2, 3, 4

_bound = False
_u32p, _u64p, _i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_REFUSED = {-1: "bad handle or null pointer", -2: "datagram index out of range or decreasing", -3: "pitch too small",
            -4: "device error"}


class _Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("max_datagram_bytes", ctypes.c_uint32)]


def _lib() -> ctypes.CDLL:
    global _bound
    L = _lib_loader()
    if not _bound:
        vp, u32, u64, cp, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t
        L.tamd_dgram_create.restype = vp
        L.tamd_dgram_create.argtypes = [ctypes.POINTER(_Params), cp, sz]
        L.tamd_dgram_destroy.restype = None
        L.tamd_dgram_destroy.argtypes = [vp]
        L.tamd_dgram_error.restype = cp
        L.tamd_dgram_error.argtypes = [vp]
        L.tamd_dgram_build.restype = ctypes.c_int
        L.tamd_dgram_build.argtypes = [vp, u32, u32, _u32p, _u32p, _u32p, _u64p, _u32p, _u32p, _u32p, _u32p, _u8p, _u8p, _u32p, _u32p,
                                       vp, u64, _u32p, _u32p, _u32p, _u32p, _i32p]
        L.tamd_dgram_parse.restype = ctypes.c_int
        L.tamd_dgram_parse.argtypes = [vp, u32, _u32p, _u32p, vp, u64, u32, u32, _u32p, _u32p, _u32p, _u32p, _u32p]
        L.tamd_dgram_set_timing.restype = None
        L.tamd_dgram_set_timing.argtypes = [vp, ctypes.c_int]
        L.tamd_dgram_kernel_ms.restype = None
        L.tamd_dgram_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_uint]
        _bound = True
    return L


def _arr(a, dtype):
    import numpy as np
    return np.ascontiguousarray(a, dtype=dtype)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


class DatagramFramer:
    """The calls that build and parse datagrams on the device.  Raises RuntimeError when no gfx950
    device is usable or the parameters are bad."""

    KERNEL_MS_FIELDS = ("build_ms", "parse_ms", "build_launches", "parse_launches")
    _h = None

    def __init__(self, max_datagram_bytes: int, device: int = 0):
        if not 8 <= int(max_datagram_bytes) <= 65535:
            raise RuntimeError("tonk_amd: DatagramFramer: bad parameters")
        p = _Params(int(device), int(max_datagram_bytes))
        err = ctypes.create_string_buffer(512)
        self.max_datagram_bytes = int(max_datagram_bytes)
        self._h = _lib().tamd_dgram_create(ctypes.byref(p), err, len(err))
        if not self._h:
            raise RuntimeError(f"tonk_amd: DatagramFramer creation failed: {err.value.decode()}")

    def _check(self, rc: int, what: str) -> None:
        if rc < 0:
            err = _lib().tamd_dgram_error(self._h).decode()
            raise RuntimeError(f"tonk_amd: {what} refused (rc={rc}: {_REFUSED.get(rc, '?')}){': ' + err if err else ''}")

    def build(self, dgram, mtype, mbytes, src, seq, seq_bytes, nonce, nonce_bytes, timestamp24, flag_bits, dev_out: int,
              pitch: int, handshake=None, has_handshake=None):
        """Messages (dgram, mtype, mbytes, src per message; src 0: zeros) into the datagrams whose
        footer fields the per-datagram lists give.  `handshake`: (n, 12) uint8 with `has_handshake`
        per datagram, or None.  Returns (out_bytes, message_bytes, reliable_offset, reliable_bytes, rc)."""
        import numpy as np
        D, T, B, S = _arr(dgram, np.uint32), _arr(mtype, np.uint32), _arr(mbytes, np.uint32), _arr(src, np.uint64)
        Q, QB, N, NB = _arr(seq, np.uint32), _arr(seq_bytes, np.uint32), _arr(nonce, np.uint32), _arr(nonce_bytes, np.uint32)
        TS, F = _arr(timestamp24, np.uint32), _arr(flag_bits, np.uint32)
        n, m = Q.size, D.size
        assert T.size == B.size == S.size == m and QB.size == N.size == NB.size == TS.size == F.size == n
        H = HH = None
        if handshake is not None:
            H, HH = _arr(handshake, np.uint8), _arr(has_handshake, np.uint8)
            assert H.size == n * HANDSHAKE_BYTES and HH.size == n
        out = [np.zeros(n, dtype=np.uint32) for _ in range(4)]
        rc = np.zeros(n, dtype=np.int32)
        self._check(_lib().tamd_dgram_build(self._h, n, m, _p(D, _u32p), _p(T, _u32p), _p(B, _u32p), _p(S, _u64p), _p(Q, _u32p),
                                            _p(QB, _u32p), _p(N, _u32p), _p(NB, _u32p), _p(H, _u8p), _p(HH, _u8p), _p(TS, _u32p),
                                            _p(F, _u32p), dev_out, pitch, *[_p(o, _u32p) for o in out], _p(rc, _i32p)), "build")
        return (*out, rc)

    def parse(self, nbytes, dev: int, pitch: int, mode: int = 0, cap: int = 16, offset=None, table=None):
        """Walk section i (nbytes[i] bytes at dev + i * pitch + offset[i]).  Returns (status,
        n_messages, reliable_offset, reliable_bytes, table), the table (n, cap) uint32 with row i's
        first min(n_messages[i], cap) entries written: type << 27 | bytes << 16 | payload_offset.
        A given `table` (n * cap uint32) is written in place."""
        import numpy as np
        B = _arr(nbytes, np.uint32)
        O = None if offset is None else _arr(offset, np.uint32)
        assert O is None or O.size == B.size
        n = B.size
        if table is None:
            table = np.zeros((n, cap), dtype=np.uint32)
        assert table.dtype == np.uint32 and table.size >= n * cap and table.flags.c_contiguous
        out = [np.zeros(n, dtype=np.uint32) for _ in range(4)]
        self._check(_lib().tamd_dgram_parse(self._h, n, _p(B, _u32p), _p(O, _u32p), dev, pitch, int(mode), int(cap),
                                            *[_p(o, _u32p) for o in out], _p(table, _u32p) if table.size else None), "parse")
        return (*out, table)

    def set_timing(self, on: bool) -> None:
        _lib().tamd_dgram_set_timing(self._h, 1 if on else 0)

    def kernel_ms(self) -> dict:
        """Device time and launches of the two kernels since the last call."""
        out = (ctypes.c_double * 4)()
        _lib().tamd_dgram_kernel_ms(self._h, out, 4)
        return dict(zip(self.KERNEL_MS_FIELDS, [float(v) for v in out]))

    def close(self) -> None:
        if self._h:
            _lib().tamd_dgram_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
