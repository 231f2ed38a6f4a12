"""Tonk's upstream compression step on MI355X (include/tonk_compress.h).

`MessageCompressor` mirrors tonk::MessageCompressor (PacketCompression.h:92-140): construct with the
maximum compressed message size (Initialize), then `compress(message)` returns the compressed
block, or b"" when the message should be sent as is (the reference's writtenBytes = 0; the
receiver then calls MessageDecompressor::InsertUncompressed).  `compress_batch` is the
device-resident batch the bench measures: many independent streams in one kernel launch.

`MessageDecompressor` mirrors tonk::MessageDecompressor (PacketCompression.h:210-260) the same
way: `decompress(block)` restores a compressed block, `insert_uncompressed(message)` takes a
message that was sent as is into the history; `decompress_batch` restores many streams in one
launch and chains after `compress_batch` on the device.
"""
from __future__ import annotations

import ctypes

from . import lib as _lib_loader

_bound = False
_u32p, _i32p, _u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
_uintp, _f32p = ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_float)


def _lib() -> ctypes.CDLL:
    global _bound
    L = _lib_loader()
    if not _bound:
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        for create, destroy in ((L.tamd_compressor_create, L.tamd_compressor_destroy),
                                (L.tamd_decompressor_create, L.tamd_decompressor_destroy)):
            create.restype = vp
            create.argtypes = [ctypes.c_uint]
            destroy.restype = None
            destroy.argtypes = [vp]
        L.tamd_compressor_compress.restype = ctypes.c_int
        L.tamd_compressor_compress.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint, vp, _uintp]
        for f in (L.tamd_compress_batch, L.tamd_compress_batch_host):
            f.restype = ctypes.c_int
            f.argtypes = [vp, u64, u32, u32, _u32p, u32, vp, _u32p, u32, _f32p]
        L.tamd_decompressor_insert_uncompressed.restype = None
        L.tamd_decompressor_insert_uncompressed.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint]
        L.tamd_decompressor_decompress.restype = ctypes.c_int
        L.tamd_decompressor_decompress.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint, vp, ctypes.c_uint, _uintp]
        for f in (L.tamd_decompress_batch, L.tamd_decompress_batch_host):
            f.restype = ctypes.c_int
            f.argtypes = [vp, u32, u32, _u32p, _u8p, u32, vp, _u32p, _i32p, _f32p]
        _bound = True
    return L


class _Handle:
    """A compressor or decompressor of the library: created or RuntimeError, destroyed once."""
    _create = _destroy = ""  # the library's calls
    _h = None

    def __init__(self, max_compressed_message_bytes: int):
        self.max = int(max_compressed_message_bytes)
        self._h = getattr(_lib(), self._create)(self.max)
        if not self._h:
            raise RuntimeError(f"tonk_amd: {self._create} failed (no gfx950 device, or bad size)")

    def close(self) -> None:
        if self._h:
            getattr(_lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        self.close()


class MessageCompressor(_Handle):
    """tonk::MessageCompressor on the GPU.  Raises when no gfx950 device is usable."""
    _create, _destroy = "tamd_compressor_create", "tamd_compressor_destroy"

    def __init__(self, max_compressed_message_bytes: int):
        super().__init__(max_compressed_message_bytes)
        self._dest = ctypes.create_string_buffer(self.max + 64)

    def compress(self, message: bytes) -> bytes:
        w = ctypes.c_uint(0)
        rc = _lib().tamd_compressor_compress(self._h, message, len(message), self._dest, ctypes.byref(w))
        if rc != 0:
            raise RuntimeError(f"tonk_amd: compress failed (rc={rc})")
        return self._dest.raw[:w.value]


def compress_batch(dev_data: int, stride: int, n_streams: int, n_msgs: int, lens, max_bytes: int, dev_out: int,
                   msgs_per_job: int = 0):
    """Compress every message of `n_streams` fresh streams (device pointers from the caller, e.g.
    torch tensors' data_ptr()).  `lens`: uint32 per message (any sequence; a contiguous numpy
    uint32 array is passed without a copy).  Returns (written bytes per message as a numpy array,
    0 = uncompressed; kernel ms)."""
    import numpy as np
    total = n_streams * n_msgs
    L = np.ascontiguousarray(lens, dtype=np.uint32)
    W = np.zeros(total, dtype=np.uint32)
    ms = ctypes.c_float(0.0)
    rc = _lib().tamd_compress_batch(dev_data, stride, n_streams, n_msgs, L.ctypes.data_as(_u32p), max_bytes, dev_out,
                                    W.ctypes.data_as(_u32p), msgs_per_job, ctypes.byref(ms))
    if rc != 0:
        raise RuntimeError(f"tonk_amd: compress_batch failed (rc={rc})")
    return W, ms.value


def compress_batch_host(data, stride: int, n_streams: int, n_msgs: int, lens, max_bytes: int,
                        msgs_per_job: int = 0) -> tuple[bytes, list[int], float]:
    """compress_batch from a host buffer (bytes-like of n_streams * stride): returns (the output
    slots, max_bytes per message; written per message; kernel ms)."""
    total = n_streams * n_msgs
    L = (ctypes.c_uint32 * total)(*lens)
    W = (ctypes.c_uint32 * total)()
    src = ctypes.create_string_buffer(bytes(data), n_streams * stride)
    out = ctypes.create_string_buffer(total * max_bytes)
    ms = ctypes.c_float(0.0)
    rc = _lib().tamd_compress_batch_host(src, stride, n_streams, n_msgs, L, max_bytes, out, W, msgs_per_job,
                                         ctypes.byref(ms))
    if rc != 0:
        raise RuntimeError(f"tonk_amd: compress_batch_host failed (rc={rc})")
    return out.raw, list(W), ms.value


class MessageDecompressor(_Handle):
    """tonk::MessageDecompressor on the GPU.  Raises when no gfx950 device is usable; after a
    block fails to decode every later call raises too (the reference's connection closes)."""
    _create, _destroy = "tamd_decompressor_create", "tamd_decompressor_destroy"

    def __init__(self, max_compressed_message_bytes: int):
        super().__init__(max_compressed_message_bytes)
        self._dest = ctypes.create_string_buffer(self.max)

    def decompress(self, block: bytes) -> bytes:
        r = ctypes.c_uint(0)
        rc = _lib().tamd_decompressor_decompress(self._h, block, len(block), self._dest, self.max, ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"tonk_amd: decompress failed (rc={rc})")
        return self._dest.raw[:r.value]

    def insert_uncompressed(self, message: bytes) -> None:
        _lib().tamd_decompressor_insert_uncompressed(self._h, message, len(message))


def decompress_batch(dev_in: int, n_streams: int, n_msgs: int, in_bytes, is_block, max_bytes: int, dev_out: int):
    """Restore every message of `n_streams` fresh streams (device pointers from the caller): slot
    i = s * n_msgs + k of `max_bytes` holds in_bytes[i] bytes, a compressed block where
    is_block[i], else the message itself; 32 readable bytes follow the last input slot.  Returns
    (restored bytes per message, status per message -- 0 or the negative reason -- as numpy
    arrays; kernel ms)."""
    import numpy as np
    total = n_streams * n_msgs
    N = np.ascontiguousarray(in_bytes, dtype=np.uint32)
    B = np.ascontiguousarray(np.asarray(is_block) != 0, dtype=np.uint8)
    assert N.size == total and B.size == total
    R = np.zeros(total, dtype=np.uint32)
    S = np.zeros(total, dtype=np.int32)
    ms = ctypes.c_float(0.0)
    rc = _lib().tamd_decompress_batch(dev_in, n_streams, n_msgs, N.ctypes.data_as(_u32p), B.ctypes.data_as(_u8p),
                                      max_bytes, dev_out, R.ctypes.data_as(_u32p), S.ctypes.data_as(_i32p), ctypes.byref(ms))
    if rc != 0:
        raise RuntimeError(f"tonk_amd: decompress_batch failed (rc={rc})")
    return R, S, ms.value


def decompress_batch_host(data, n_streams: int, n_msgs: int, in_bytes, is_block, max_bytes: int):
    """decompress_batch from a host buffer of n_streams * n_msgs slots: returns (the output slots,
    restored per message, status per message, kernel ms)."""
    total = n_streams * n_msgs
    N = (ctypes.c_uint32 * total)(*in_bytes)
    B = (ctypes.c_uint8 * total)(*[1 if b else 0 for b in is_block])
    R = (ctypes.c_uint32 * total)()
    S = (ctypes.c_int32 * total)()
    src = ctypes.create_string_buffer(bytes(data), total * max_bytes)
    out = ctypes.create_string_buffer(total * max_bytes)
    ms = ctypes.c_float(0.0)
    rc = _lib().tamd_decompress_batch_host(src, n_streams, n_msgs, N, B, max_bytes, out, R, S, ctypes.byref(ms))
    if rc != 0:
        raise RuntimeError(f"tonk_amd: decompress_batch_host failed (rc={rc})")
    return out.raw, list(R), list(S), ms.value
