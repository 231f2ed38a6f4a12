"""The reference message codec from Python: the ctypes binding of oracle/_ref/libmsgcodec_ref.so
(tonk::MessageCompressor / MessageDecompressor restated over the reference's zstd,
oracle/msgcodec_ref.cpp), and the stream and case files of tests/native/unlz_check.cpp.

Stream files: "UNLZ", u32 streams; per stream u32 max, u32 messages; per message u32 is_block,
u32 bytes, the bytes.  Case files add per message i32 status, u32 restored, the restored bytes.
"""
from __future__ import annotations

import ctypes
import os
import struct

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref", "libmsgcodec_ref.so")
MAX = 1300  # kMaxCompressedBytes of TonkUnitTest.cpp:604 (Tonk's datagram budget)


def load() -> ctypes.CDLL:
    """The bound library.  Raises OSError when REF is absent (not built: the reference tree was
    not there) or cannot be loaded; callers that may do without it test for REF first."""
    L = ctypes.CDLL(REF)
    vp, cu = ctypes.c_void_p, ctypes.c_uint
    L.ref_comp_new.restype = vp
    L.ref_comp_new.argtypes = [cu]
    L.ref_comp.restype = ctypes.c_int
    L.ref_comp.argtypes = [vp, vp, cu, vp, ctypes.POINTER(cu)]
    L.ref_comp_free.argtypes = [vp]
    L.ref_decomp_new.restype = vp
    L.ref_decomp_new.argtypes = [cu]
    L.ref_insert.argtypes = [vp, vp, cu]
    L.ref_decomp.restype = ctypes.c_int
    L.ref_decomp.argtypes = [vp, vp, cu, vp, cu]
    L.ref_decomp_free.argtypes = [vp]
    return L


class RefDecompressor:
    def __init__(self, L, max_bytes=MAX):
        self.L, self.h = L, L.ref_decomp_new(max_bytes)
        self.buf = ctypes.create_string_buffer(max_bytes + 64)

    def feed(self, block: bytes, original: bytes) -> bytes:
        """Tonk's receive side: Decompress a compressed block, InsertUncompressed otherwise."""
        if not block:
            self.L.ref_insert(self.h, original, len(original))
            return original
        out = self.decompress(block)
        assert out is not None, "reference zstd rejected the block"
        return out

    def decompress(self, block: bytes):
        """The restored bytes, or None when the reference rejects the block."""
        n = self.L.ref_decomp(self.h, block, len(block), self.buf, len(self.buf))
        return self.buf.raw[:n] if n >= 0 else None


class RefCompressor:
    def __init__(self, L, max_bytes=MAX):
        self.L, self.h = L, L.ref_comp_new(max_bytes)
        self.buf = ctypes.create_string_buffer(max_bytes + 64)

    def compress(self, msg: bytes) -> bytes:
        w = ctypes.c_uint(0)
        assert self.L.ref_comp(self.h, msg, len(msg), self.buf, ctypes.byref(w)) == 0
        return self.buf.raw[:w.value]


def write_streams(path, streams):
    """A stream file: [(max, messages)], a message either its bytes (sent as is) or
    (is_block, bytes)."""
    with open(path, "wb") as f:
        f.write(b"UNLZ" + struct.pack("<I", len(streams)))
        for max_bytes, msgs in streams:
            f.write(struct.pack("<II", max_bytes, len(msgs)))
            for m in msgs:
                isb, data = (0, m) if isinstance(m, bytes) else m
                f.write(struct.pack("<II", int(isb), len(data)) + data)


def write_cases(path, streams):
    """A case file of what a compressor returned, for tests/native/lz_blocks.cpp:
    [(max, [(message, block)])], block empty when the message was sent as is."""
    with open(path, "wb") as f:
        f.write(b"UNLZ" + struct.pack("<I", len(streams)))
        for max_bytes, msgs in streams:
            f.write(struct.pack("<II", max_bytes, len(msgs)))
            for message, block in msgs:
                if block:
                    f.write(struct.pack("<II", 1, len(block)) + bytes(block) + struct.pack("<iI", 0, len(message)) + message)
                else:
                    f.write(struct.pack("<II", 0, len(message)) + message + struct.pack("<iI", 0, 0))


def read_cases(path, verdicts):
    """A case file of unlz_check: [(max, [(is_block, bytes, status, restored bytes)])]."""
    with open(path, "rb") as f:
        raw = f.read()
    assert raw[:4] == b"UNLZ"
    n, = struct.unpack_from("<I", raw, 4)
    at, out = 8, []
    for _ in range(n):
        max_bytes, m = struct.unpack_from("<II", raw, at)
        at += 8
        msgs = []
        for _ in range(m):
            isb, ln = struct.unpack_from("<II", raw, at)
            at += 8
            data = raw[at:at + ln]
            at += ln
            status, restored = 0, b""
            if verdicts:
                status, r = struct.unpack_from("<iI", raw, at)
                at += 8
                restored = raw[at:at + r]
                at += r
            msgs.append((bool(isb), data, status, restored))
        out.append((max_bytes, msgs))
    return out
