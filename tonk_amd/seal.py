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

from ._handle import Handle, arr, i32p, ptr, u8p, u16p, u32, u32p, u64, u64p, vp, zeros

FOOTER_BYTES = 24  # TAMD_SEAL_FOOTER_BYTES
OK, INVALID, BAD_TAG = 0, 1, 2


class _Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("max_datagram_bytes", ctypes.c_uint32)]


class DatagramSealer(Handle):
    """The keys of `n_streams` connections and the calls that seal and open their datagrams on the
    device.  Raises RuntimeError when no gfx950 device is usable or the parameters are bad."""

    KERNEL_MS_FIELDS = ("packets_ms", "footers_ms", "packets_launches", "footers_launches")
    _PREFIX = "tamd_seal"
    _CALLS = {"set_key": [vp, u32, u64],
              "seal": [vp, u32, u32p, u64p, u32p, u32p, vp, u64, i32p],
              "open": [vp, u32, u32p, u64p, u32p, u32p, vp, u64, i32p],
              "cipher": [vp, u32, u32p, u64p, u32p, vp, u64],
              "tag": [vp, u32, u32p, u64p, u32p, vp, u64, u16p],
              "footers": [vp, u32, u32p, vp, u64, u8p]}
    _REFUSED = {-1: "bad handle or null pointer", -2: "stream id out of range", -3: "pitch smaller than the largest datagram",
                -4: "device error"}

    def __init__(self, n_streams: int, max_datagram_bytes: int, device: int = 0):
        if not (0 < int(n_streams) < 2**32 and 0 < int(max_datagram_bytes) <= 65535):
            raise RuntimeError("tonk_amd: DatagramSealer: bad parameters")
        self.n_streams, self.max_datagram_bytes = int(n_streams), int(max_datagram_bytes)
        self._create(_Params(int(device), int(n_streams), int(max_datagram_bytes)))

    def set_key(self, stream: int, key: int) -> None:
        """SimpleCipher::Initialize of one stream; takes effect with the next call."""
        self._check(self._c.set_key(self._h, int(stream), int(key) & 0xFFFFFFFFFFFFFFFF), "set_key")

    def _datagrams(self, what, stream, nonce, nbytes, message_bytes, dev: int, pitch: int):
        S, N, B, M = arr(stream, "uint32"), arr(nonce, "uint64"), arr(nbytes, "uint32"), arr(message_bytes, "uint32")
        assert S.size == N.size == B.size == M.size
        rc = zeros(S.size, "int32")
        self._check(getattr(self._c, what)(self._h, S.size, ptr(S, u32p), ptr(N, u64p), ptr(B, u32p), ptr(M, u32p), dev, pitch,
                                           ptr(rc, i32p)), what)
        return rc

    def seal(self, stream, nonce, nbytes, message_bytes, dev_datagrams: int, pitch: int):
        """Cipher the first message_bytes[i] bytes of every datagram and write its tag; returns the result codes."""
        return self._datagrams("seal", stream, nonce, nbytes, message_bytes, dev_datagrams, pitch)

    def open(self, stream, nonce, nbytes, message_bytes, dev_datagrams: int, pitch: int):
        """Check every datagram's tag and decipher those that match; returns the result codes."""
        return self._datagrams("open", stream, nonce, nbytes, message_bytes, dev_datagrams, pitch)

    def cipher(self, stream, nonce, nbytes, dev_data: int, pitch: int) -> None:
        """Cipher over nbytes[i] bytes of every entry, in place."""
        S, N, B = arr(stream, "uint32"), arr(nonce, "uint64"), arr(nbytes, "uint32")
        assert S.size == N.size == B.size
        self._check(self._c.cipher(self._h, S.size, ptr(S, u32p), ptr(N, u64p), ptr(B, u32p), dev_data, pitch), "cipher")

    def tag(self, stream, nonce, nbytes, dev_data: int, pitch: int):
        """Plain Tag() of nbytes[i] bytes of every entry; returns the tags (uint16)."""
        S, N, B = arr(stream, "uint32"), arr(nonce, "uint64"), arr(nbytes, "uint32")
        assert S.size == N.size == B.size
        out = zeros(S.size, "uint16")
        self._check(self._c.tag(self._h, S.size, ptr(S, u32p), ptr(N, u64p), ptr(B, u32p), dev_data, pitch, ptr(out, u16p)), "tag")
        return out

    def footers(self, nbytes, dev_datagrams: int, pitch: int):
        """The last min(nbytes[i], 24) bytes of every datagram, right-aligned and zero-filled: an (n, 24) uint8 array."""
        B = arr(nbytes, "uint32")
        out = zeros((B.size, FOOTER_BYTES), "uint8")
        self._check(self._c.footers(self._h, B.size, ptr(B, u32p), dev_datagrams, pitch, ptr(out, u8p)), "footers")
        return out
