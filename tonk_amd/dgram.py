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

from ._handle import Handle, arr, i32p, ptr, u8p, u32, u32p, u64, u64p, vp, zeros

HANDSHAKE_BYTES = 12
TYPE_RAW = 255          # build: the headerless body of an OnlyFEC datagram
SEQCOMP, ONLYFEC = 0x20, 0x10
OK, INVALID, TRUNCATED, BAD_FRAME, BAD_ACKACK = 0, 1, 2, 3, 4


class _Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("max_datagram_bytes", ctypes.c_uint32)]


class DatagramFramer(Handle):
    """The calls that build and parse datagrams on the device.  Raises RuntimeError when no gfx950
    device is usable or the parameters are bad."""

    KERNEL_MS_FIELDS = ("build_ms", "parse_ms", "build_launches", "parse_launches")
    _PREFIX = "tamd_dgram"
    _CALLS = {"build": [vp, u32, u32, u32p, u32p, u32p, u64p, u32p, u32p, u32p, u32p, u8p, u8p, u32p, u32p, vp, u64, u32p, u32p, u32p,
                        u32p, i32p],
              "parse": [vp, u32, u32p, u32p, vp, u64, u32, u32, u32p, u32p, u32p, u32p, u32p]}
    _REFUSED = {-1: "bad handle or null pointer", -2: "datagram index out of range or decreasing", -3: "pitch too small",
                -4: "device error"}

    def __init__(self, max_datagram_bytes: int, device: int = 0):
        if not 8 <= int(max_datagram_bytes) <= 65535:
            raise RuntimeError("tonk_amd: DatagramFramer: bad parameters")
        self.max_datagram_bytes = int(max_datagram_bytes)
        self._create(_Params(int(device), int(max_datagram_bytes)))

    def build(self, dgram, mtype, mbytes, src, seq, seq_bytes, nonce, nonce_bytes, timestamp24, flag_bits, dev_out: int,
              pitch: int, handshake=None, has_handshake=None):
        """Messages (dgram, mtype, mbytes, src per message; src 0: zeros) into the datagrams whose
        footer fields the per-datagram lists give.  `handshake`: (n, 12) uint8 with `has_handshake`
        per datagram, or None.  Returns (out_bytes, message_bytes, reliable_offset, reliable_bytes, rc)."""
        D, T, B, S = arr(dgram, "uint32"), arr(mtype, "uint32"), arr(mbytes, "uint32"), arr(src, "uint64")
        Q, QB, N, NB = arr(seq, "uint32"), arr(seq_bytes, "uint32"), arr(nonce, "uint32"), arr(nonce_bytes, "uint32")
        TS, F = arr(timestamp24, "uint32"), arr(flag_bits, "uint32")
        n, m = Q.size, D.size
        assert T.size == B.size == S.size == m and QB.size == N.size == NB.size == TS.size == F.size == n
        H = HH = None
        if handshake is not None:
            H, HH = arr(handshake, "uint8"), arr(has_handshake, "uint8")
            assert H.size == n * HANDSHAKE_BYTES and HH.size == n
        out = [zeros(n, "uint32") for _ in range(4)]
        rc = zeros(n, "int32")
        self._check(self._c.build(self._h, n, m, ptr(D, u32p), ptr(T, u32p), ptr(B, u32p), ptr(S, u64p), ptr(Q, u32p),
                                  ptr(QB, u32p), ptr(N, u32p), ptr(NB, u32p), ptr(H, u8p), ptr(HH, u8p), ptr(TS, u32p),
                                  ptr(F, u32p), dev_out, pitch, *[ptr(o, u32p) for o in out], ptr(rc, i32p)), "build")
        return (*out, rc)

    def parse(self, nbytes, dev: int, pitch: int, mode: int = 0, cap: int = 16, offset=None, table=None):
        """Walk section i (nbytes[i] bytes at dev + i * pitch + offset[i]).  Returns (status,
        n_messages, reliable_offset, reliable_bytes, table), the table (n, cap) uint32 with row i's
        first min(n_messages[i], cap) entries written: type << 27 | bytes << 16 | payload_offset.
        A given `table` (n * cap uint32) is written in place."""
        B = arr(nbytes, "uint32")
        O = None if offset is None else arr(offset, "uint32")
        assert O is None or O.size == B.size
        n = B.size
        if table is None:
            table = zeros((n, cap), "uint32")
        assert table.dtype == "uint32" and table.size >= n * cap and table.flags.c_contiguous
        out = [zeros(n, "uint32") for _ in range(4)]
        self._check(self._c.parse(self._h, n, ptr(B, u32p), ptr(O, u32p), dev, pitch, int(mode), int(cap),
                                  *[ptr(o, u32p) for o in out], ptr(table, u32p) if table.size else None), "parse")
        return (*out, table)
