"""Helpers of tests/test_batch_gpu.py: the reference codec
(oracle/_ref/libsiamese_ref.so) through ctypes, one encoder or decoder per object, and guarded
device buffers.  Test infrastructure only."""
from __future__ import annotations

import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libsiamese_ref.so")

# the framing checks' lengths (tests/native/frame_check.cpp); the short-packet parity tests use the first 18
# (through 4000), the long-packet ones their own list up to 65535 (test_batch_gpu.py LONG_LENS)
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 127, 128, 129, 1023, 1024, 1025, 1300, 1535, 1536, 1537, 4000, 16383, 16384, 65535]
SUCCESS, INVALID, NEED_MORE, MAX_PACKETS, DUPLICATE, DISABLED = range(6)


class Orig(ctypes.Structure):
    _fields_ = [("PacketNum", ctypes.c_uint), ("DataBytes", ctypes.c_uint), ("Data", ctypes.c_void_p)]


class Rec(ctypes.Structure):
    _fields_ = [("DataBytes", ctypes.c_uint), ("Data", ctypes.c_void_p)]


_ref = None


def ref_lib():
    global _ref
    if _ref is None:
        L = ctypes.CDLL(REF)
        assert L.siamese_init_(5) == 0
        vp = ctypes.c_void_p
        for n in ("siamese_encoder_create", "siamese_decoder_create"):
            getattr(L, n).restype = vp
        for n in ("siamese_encoder_free", "siamese_decoder_free"):
            getattr(L, n).argtypes = [vp]
            getattr(L, n).restype = None
        for n in ("siamese_encoder_add", "siamese_encode", "siamese_decoder_add_original", "siamese_decoder_add_recovery"):
            getattr(L, n).argtypes = [vp, vp]
        L.siamese_encoder_ack.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint)]
        L.siamese_decoder_is_ready.argtypes = [vp]
        L.siamese_decode.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Orig)), ctypes.POINTER(ctypes.c_uint)]
        L.siamese_decoder_ack.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint)]
        _ref = L
    return _ref


class RefEncoder:
    def __init__(self):
        self.L = ref_lib()
        self.h = self.L.siamese_encoder_create()
        assert self.h

    def add(self, data: bytes):
        buf = ctypes.create_string_buffer(data, len(data))
        o = Orig(0, len(data), ctypes.cast(buf, ctypes.c_void_p))
        rc = self.L.siamese_encoder_add(self.h, ctypes.byref(o))
        return rc, (o.PacketNum if rc == 0 else 0)

    def encode(self):
        r = Rec()
        rc = self.L.siamese_encode(self.h, ctypes.byref(r))
        return rc, (ctypes.string_at(r.Data, r.DataBytes) if rc == 0 else b"")

    def ack(self, data: bytes):
        nxt = ctypes.c_uint(0)
        rc = self.L.siamese_encoder_ack(self.h, data, len(data), ctypes.byref(nxt))
        return rc, nxt.value

    def close(self):
        if self.h:
            self.L.siamese_encoder_free(self.h)
            self.h = None


class RefDecoder:
    def __init__(self):
        self.L = ref_lib()
        self.h = self.L.siamese_decoder_create()
        assert self.h

    def add_original(self, num: int, data: bytes):
        buf = ctypes.create_string_buffer(data, len(data))
        return self.L.siamese_decoder_add_original(self.h, ctypes.byref(Orig(num, len(data), ctypes.cast(buf, ctypes.c_void_p))))

    def add_recovery(self, data: bytes):
        buf = ctypes.create_string_buffer(data, len(data))
        return self.L.siamese_decoder_add_recovery(self.h, ctypes.byref(Rec(len(data), ctypes.cast(buf, ctypes.c_void_p))))

    def decode_if_ready(self):
        """is_ready, and when it is, decode (tamd_batch_decode's flow): (rc, [(num, payload)])."""
        rc = self.L.siamese_decoder_is_ready(self.h)
        if rc != 0:
            return rc, []
        pp, cnt = ctypes.POINTER(Orig)(), ctypes.c_uint(0)
        rc = self.L.siamese_decode(self.h, ctypes.byref(pp), ctypes.byref(cnt))
        if rc != 0:
            return rc, []
        return rc, [(pp[i].PacketNum, ctypes.string_at(pp[i].Data, pp[i].DataBytes)) for i in range(cnt.value)]

    def ack(self, limit: int = 256):
        buf, used = ctypes.create_string_buffer(limit), ctypes.c_uint(0)
        rc = self.L.siamese_decoder_ack(self.h, buf, limit, ctypes.byref(used))
        return rc, buf.raw[:used.value]

    def close(self):
        if self.h:
            self.L.siamese_decoder_free(self.h)
            self.h = None


class Guarded:
    """A caller buffer on the device with 64 guard bytes of 0xA5 on each side (`skew` moves its
    start off the allocation's alignment)."""
    GUARD, FILL = 64, 0xA5

    def __init__(self, hip, nbytes: int, skew: int = 0):
        self.hip, self.n, self.skew = hip, nbytes, skew
        self.base = hip.malloc(nbytes + 2 * self.GUARD + skew, fill=self.FILL)
        self.ptr = self.base + self.GUARD + skew

    def fill(self):
        assert self.hip.L.hipMemset(self.ptr, self.FILL, self.n) == 0

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        assert arr.size <= self.n
        self.hip.upload(self.ptr, arr)

    def download(self, n=None):
        return self.hip.download(self.ptr, self.n if n is None else n)

    def check(self):
        lo = self.hip.download(self.base, self.GUARD + self.skew)
        hi = self.hip.download(self.ptr + self.n, self.GUARD)
        assert (lo == self.FILL).all() and (hi == self.FILL).all(), "guard bytes of a caller buffer were written"


def slots(packets, pitch: int, n=None) -> np.ndarray:
    """Packets (bytes, or None for an empty slot) laid out at i * pitch, gaps 0xA5."""
    out = np.full((len(packets) if n is None else n) * pitch, Guarded.FILL, dtype=np.uint8)
    for i, p in enumerate(packets):
        if p:
            out[i * pitch:i * pitch + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return out
