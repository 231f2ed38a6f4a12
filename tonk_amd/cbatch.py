"""Stateful batched compression and decompression of Tonk's reliable messages in the caller's own
device memory (include/tonk_compress_batch.h).

`BatchCompressor` owns the compression history of `n_streams` connections on the device: the
sender's ring per stream (`COMPRESS`), the receiver's state and ring (`DECOMPRESS`), or both.
`compress` takes a tick's messages of any subset of the streams at their device addresses and
writes the blocks to `dev_out + i * out_pitch`; `written[i] == 0` means "send as is"
(MessageCompressor::Compress's contract).  `decompress` restores blocks to `dev_out + i * out_pitch`
and takes messages that were sent as is into their stream's history.  Device pointers are ints
(e.g. a torch tensor's data_ptr()), lists are numpy arrays or sequences, results numpy arrays.  A
call the library refuses as a whole raises RuntimeError with tamd_cbatch_error's text.  Every call
is synchronous.
"""
from __future__ import annotations

import ctypes

from . import CBATCH_LIB_PATH
from ._handle import Handle, arr, i32p, ptr, u8p, u32, u32p, u64, u64p, vp, zeros

COMPRESS, DECOMPRESS = 1, 2
MAX_MESSAGE_BYTES = 24000
# status values of decompress (the block reader's reasons are -1 .. -12)
OK, STREAM_FAILED, BAD_SIZE = 0, -13, -14


class _Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("device", "n_streams", "max_message_bytes", "sides", "abut")]


class BatchCompressor(Handle):
    """The compressors and decompressors of `n_streams` connections on the device.  Raises
    RuntimeError when no gfx950 device is usable or the parameters are bad.  `abut`: several
    messages of a stream per pass -- fewer launches, and a block's last sequence may differ from the
    per-message drop-in's (include/tonk_compress_batch.h)."""

    KERNEL_MS_FIELDS = ("place_ms", "compress_ms", "decompress_ms", "spare_ms", "place_launches", "compress_launches",
                        "decompress_launches", "spare_launches")
    _PREFIX = "tamd_cbatch"
    _LIB = CBATCH_LIB_PATH
    _CALLS = {"compress": [vp, u32, u32p, u64p, u32p, vp, u64, u32p],
              "decompress": [vp, u32, u32p, u64p, u32p, u8p, vp, u64, u32p, i32p],
              "reset": [vp, u32, u32p, u32]}
    _REFUSED = {-1: "bad handle, null pointer, a side the handle lacks, a message size outside 1..max or an output above 4 GiB",
                -2: "stream id out of range", -3: "out_pitch below max_message_bytes", -4: "device error"}

    def __init__(self, n_streams: int, max_message_bytes: int, sides: int = COMPRESS | DECOMPRESS, device: int = 0,
                 abut: bool = False):
        if int(n_streams) < 1 or not 1 <= int(max_message_bytes) <= MAX_MESSAGE_BYTES or not int(sides) & 3 or int(sides) & ~3:
            raise RuntimeError("tonk_amd: BatchCompressor: bad parameters")
        self.n_streams, self.max_message_bytes, self.sides = int(n_streams), int(max_message_bytes), int(sides)
        self._create(_Params(int(device), self.n_streams, self.max_message_bytes, self.sides, 1 if abut else 0))

    def compress(self, stream, src, nbytes, dev_out: int, out_pitch: int):
        """Item i: the next message of stream[i], nbytes[i] bytes at device address src[i].
        Returns written (uint32): 0 = send the message as is, else the block's bytes at
        dev_out + i * out_pitch."""
        S, A, B = arr(stream, "uint32"), arr(src, "uint64"), arr(nbytes, "uint32")
        assert A.size == B.size == S.size
        written = zeros(S.size, "uint32")
        self._check(self._c.compress(self._h, S.size, ptr(S, u32p), ptr(A, u64p), ptr(B, u32p), dev_out, out_pitch,
                                     ptr(written, u32p)), "compress")
        return written

    def decompress(self, stream, src, nbytes, is_block, dev_out: int, out_pitch: int):
        """Item i: a block (is_block[i]) restored to dev_out + i * out_pitch, or a message sent as
        is that only enters the history.  Returns (restored, status)."""
        S, A, B, K = arr(stream, "uint32"), arr(src, "uint64"), arr(nbytes, "uint32"), arr(is_block, "uint8")
        assert A.size == B.size == K.size == S.size
        restored, status = zeros(S.size, "uint32"), zeros(S.size, "int32")
        self._check(self._c.decompress(self._h, S.size, ptr(S, u32p), ptr(A, u64p), ptr(B, u32p), ptr(K, u8p), dev_out, out_pitch,
                                       ptr(restored, u32p), ptr(status, i32p)), "decompress")
        return restored, status

    def reset(self, stream, sides: int = COMPRESS | DECOMPRESS) -> None:
        """The named streams start again with an empty history on the sides named."""
        S = arr(stream, "uint32")
        self._check(self._c.reset(self._h, S.size, ptr(S, u32p), int(sides)), "reset")
