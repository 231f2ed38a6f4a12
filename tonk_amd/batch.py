"""Batched encoders and decoders over the caller's own device packets (include/tonk_batch.h).

`BatchCodec` owns `n_streams` connections on one MI355X, each with a Siamese encoder and decoder.
Its methods take device pointers (ints, e.g. a torch tensor's data_ptr()) and numpy index arrays,
and return numpy arrays: packet i of a call lives at `dev + i * pitch`.  Per-packet and per-stream
result codes are the siamese.h values (0 Success, 1 InvalidInput, 2 NeedMoreData,
3 MaxPacketsReached, 4 DuplicateData, 5 Disabled); a call the library refuses as a whole (a stream
id out of range, a pitch below the largest packet, a device error) raises RuntimeError with
tamd_batch_error's text.  Every call is synchronous.
"""
from __future__ import annotations

import ctypes

from . import lib as _lib_loader

RECOVERY_OVERHEAD = 11  # TAMD_BATCH_RECOVERY_OVERHEAD

_bound = False
_u32p, _i32p, _u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
_REFUSED = {-1: "bad handle or null pointer", -2: "stream id out of range", -3: "pitch smaller than the largest packet",
            -4: "device error"}


class _Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("max_packet_bytes", ctypes.c_uint32),
                ("arena_bytes", ctypes.c_uint64)]


def _lib() -> ctypes.CDLL:
    global _bound
    L = _lib_loader()
    if not _bound:
        vp, u32, u64, cp, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t
        L.tamd_batch_create.restype = vp
        L.tamd_batch_create.argtypes = [ctypes.POINTER(_Params), cp, sz]
        L.tamd_batch_destroy.restype = None
        L.tamd_batch_destroy.argtypes = [vp]
        L.tamd_batch_error.restype = cp
        L.tamd_batch_error.argtypes = [vp]
        for name, args in (
                ("tamd_batch_encoder_add", [vp, u32, _u32p, _u32p, vp, u64, _u32p, _i32p]),
                ("tamd_batch_encoder_add_at", [vp, u32, _u32p, _u32p, _u32p, vp, u64, _u32p, _i32p]),
                ("tamd_batch_decoder_add_original_at", [vp, u32, _u32p, _u32p, _u32p, _u32p, vp, u64, _i32p]),
                ("tamd_batch_encode", [vp, u32, _u32p, vp, u64, _u32p, _i32p]),
                ("tamd_batch_encoder_ack", [vp, u32, cp, u32, _u32p]),
                ("tamd_batch_decoder_add_original", [vp, u32, _u32p, _u32p, _u32p, vp, u64, _i32p]),
                ("tamd_batch_decoder_add_recovery", [vp, u32, _u32p, _u32p, vp, u64, _i32p]),
                ("tamd_batch_decode", [vp, u32, _u32p, vp, u64, u32, _u32p, _u32p, _u32p, _u32p, _i32p]),
                ("tamd_batch_decoder_ack", [vp, u32, _u8p, u32, _u32p])):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = args
        L.tamd_batch_set_timing.restype = None
        L.tamd_batch_set_timing.argtypes = [vp, ctypes.c_int]
        L.tamd_batch_kernel_ms.restype = None
        L.tamd_batch_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_uint]
        _bound = True
    return L


def _u32(a):
    import numpy as np
    return np.ascontiguousarray(a, dtype=np.uint32)


class BatchCodec:
    """`n_streams` encoder/decoder pairs over device packets.  Raises RuntimeError when no gfx950
    device is usable or the parameters are bad."""

    KERNEL_MS_FIELDS = ("frame_ms", "unframe_ms", "tails_ms", "program_ms", "frame_launches", "unframe_launches",
                        "tails_launches", "program_launches", "frame_bytes", "unframe_bytes")
    _h = None

    def __init__(self, n_streams: int, max_packet_bytes: int, arena_bytes: int, device: int = 0):
        if not (0 < int(n_streams) < 2**32 and 0 < int(max_packet_bytes) <= 65535 and 0 < int(arena_bytes) < 2**64):
            raise RuntimeError("tonk_amd: BatchCodec: bad parameters")
        p = _Params(int(device), int(n_streams), int(max_packet_bytes), int(arena_bytes))
        err = ctypes.create_string_buffer(512)
        self.n_streams, self.max_packet_bytes = int(n_streams), int(max_packet_bytes)
        self._h = _lib().tamd_batch_create(ctypes.byref(p), err, len(err))
        if not self._h:
            raise RuntimeError(f"tonk_amd: BatchCodec creation failed: {err.value.decode()}")

    def _check(self, rc: int, what: str) -> None:
        if rc < 0:
            err = _lib().tamd_batch_error(self._h).decode()
            raise RuntimeError(f"tonk_amd: {what} refused (rc={rc}: {_REFUSED.get(rc, '?')}){': ' + err if err else ''}")

    def encoder_add(self, stream, lens, dev_payloads: int, pitch: int, offset=None):
        """Add originals (packet i at dev_payloads + i * pitch + offset[i]); returns (packet numbers, result codes)."""
        import numpy as np
        S, L = _u32(stream), _u32(lens)
        O = None if offset is None else _u32(offset)
        assert S.size == L.size and (O is None or O.size == S.size)
        pn, rc = np.zeros(S.size, dtype=np.uint32), np.zeros(S.size, dtype=np.int32)
        self._check(_lib().tamd_batch_encoder_add_at(self._h, S.size, S.ctypes.data_as(_u32p), L.ctypes.data_as(_u32p),
                                                     None if O is None else O.ctypes.data_as(_u32p), dev_payloads, pitch,
                                                     pn.ctypes.data_as(_u32p), rc.ctypes.data_as(_i32p)), "encoder_add")
        return pn, rc

    def encode(self, stream, dev_out: int, pitch: int):
        """One recovery packet per list entry at dev_out + i * pitch; returns (bytes, result codes)."""
        import numpy as np
        S = _u32(stream)
        nb, rc = np.zeros(S.size, dtype=np.uint32), np.zeros(S.size, dtype=np.int32)
        self._check(_lib().tamd_batch_encode(self._h, S.size, S.ctypes.data_as(_u32p), dev_out, pitch,
                                             nb.ctypes.data_as(_u32p), rc.ctypes.data_as(_i32p)), "encode")
        return nb, rc

    def encoder_ack(self, stream: int, data: bytes):
        """siamese_encoder_ack of one stream; returns (result code, next expected packet number)."""
        nxt = ctypes.c_uint32(0)
        rc = _lib().tamd_batch_encoder_ack(self._h, stream, bytes(data), len(data), ctypes.byref(nxt))
        self._check(rc, "encoder_ack")
        return rc, int(nxt.value)

    def decoder_add_original(self, stream, packet_num, lens, dev_payloads: int, pitch: int, offset=None):
        """Add received originals (packet i at dev_payloads + i * pitch + offset[i]); returns the result codes."""
        import numpy as np
        S, P, L = _u32(stream), _u32(packet_num), _u32(lens)
        O = None if offset is None else _u32(offset)
        assert S.size == P.size == L.size and (O is None or O.size == S.size)
        rc = np.zeros(S.size, dtype=np.int32)
        self._check(_lib().tamd_batch_decoder_add_original_at(self._h, S.size, S.ctypes.data_as(_u32p), P.ctypes.data_as(_u32p),
                                                              L.ctypes.data_as(_u32p),
                                                              None if O is None else O.ctypes.data_as(_u32p), dev_payloads,
                                                              pitch, rc.ctypes.data_as(_i32p)), "decoder_add_original")
        return rc

    def decoder_add_recovery(self, stream, nbytes, dev_packets: int, pitch: int):
        """Add received recovery packets; returns the result codes."""
        import numpy as np
        S, B = _u32(stream), _u32(nbytes)
        assert S.size == B.size
        rc = np.zeros(S.size, dtype=np.int32)
        self._check(_lib().tamd_batch_decoder_add_recovery(self._h, S.size, S.ctypes.data_as(_u32p), B.ctypes.data_as(_u32p),
                                                           dev_packets, pitch, rc.ctypes.data_as(_i32p)),
                    "decoder_add_recovery")
        return rc

    def decode(self, stream, dev_out: int, pitch: int, cap: int):
        """Decode every listed stream that is ready; recovered payload j at dev_out + j * pitch.
        Returns (per-stream result codes, out_stream, out_packet_num, out_bytes)."""
        import numpy as np
        S = _u32(stream)
        rc = np.zeros(S.size, dtype=np.int32)
        os_, op, ob = (np.zeros(max(cap, 1), dtype=np.uint32) for _ in range(3))
        n = ctypes.c_uint32(0)
        self._check(_lib().tamd_batch_decode(self._h, S.size, S.ctypes.data_as(_u32p), dev_out, pitch, cap,
                                             os_.ctypes.data_as(_u32p), op.ctypes.data_as(_u32p), ob.ctypes.data_as(_u32p),
                                             ctypes.byref(n), rc.ctypes.data_as(_i32p)), "decode")
        k = int(n.value)
        return rc, os_[:k].copy(), op[:k].copy(), ob[:k].copy()

    def decoder_ack(self, stream: int, limit: int = 256):
        """siamese_decoder_ack of one stream; returns (result code, ack bytes)."""
        buf = (ctypes.c_uint8 * max(limit, 1))()
        used = ctypes.c_uint32(0)
        rc = _lib().tamd_batch_decoder_ack(self._h, stream, buf, limit, ctypes.byref(used))
        self._check(rc, "decoder_ack")
        return rc, bytes(buf[:used.value])

    def set_timing(self, on: bool) -> None:
        _lib().tamd_batch_set_timing(self._h, 1 if on else 0)

    def kernel_ms(self) -> dict:
        """Device time and launches of the helper kernels and the codec programs since the last call."""
        out = (ctypes.c_double * 10)()
        _lib().tamd_batch_kernel_ms(self._h, out, 10)
        return dict(zip(self.KERNEL_MS_FIELDS, [float(v) for v in out]))

    def close(self) -> None:
        if self._h:
            _lib().tamd_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
