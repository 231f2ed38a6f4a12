"""The front of Tonk's receive path for datagrams in the caller's own device memory
(include/tonk_receive.h).

`DatagramReceiver` owns, per connection, the cipher key and the anti-replay state (Tonk's
StrikeRegister) of `n_streams` connections on one MI355X.  `receive` takes a tick's datagrams as
they came off the wire -- datagram i at `dev + i * pitch`, any alignment -- through footer read,
nonce expansion, duplicate check, tag check, accept and decipher, the datagrams of one stream in
list order, and returns the verdicts and the footer fields.  Device pointers are ints or torch
tensors, lists are numpy arrays or sequences, results numpy arrays.  Per-datagram result codes:
0 accepted and deciphered, 1 invalid, 2 bad tag, 3 duplicate, 4 accepted but "re-ordered" (do not
process its messages); only 0 and 4 change anything.  A call the library refuses as a whole raises
RuntimeError with tamd_recv_error's text.  Every call is synchronous.
"""
from __future__ import annotations

import ctypes

from . import RECV_LIB_PATH
from ._handle import Handle, arr, i32p, ptr, u32, u32p, u64, u64p, vp, zeros

OK, INVALID, BAD_TAG, DUPLICATE, REORDERED = 0, 1, 2, 3, 4
STATE_WORDS = 67  # TAMD_RECV_STATE_WORDS: largest, base, rotation, 64 window words
# tamd_recv_result as a numpy record
RESULT_FIELDS = [("nonce", "<u8"), ("message_bytes", "<u4"), ("timestamp24", "<u4"), ("partial_seq", "<u4"), ("flags", "u1"),
                 ("seq_bytes", "u1"), ("nonce_bytes", "u1"), ("handshake_bytes", "u1")]


class _Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("max_datagram_bytes", ctypes.c_uint32)]


def _address(dev) -> int:
    """A device pointer: an int, or a torch tensor's."""
    return int(dev.data_ptr()) if hasattr(dev, "data_ptr") else int(dev)


class DatagramReceiver(Handle):
    """The keys and anti-replay states of `n_streams` connections and the call that receives their
    datagrams on the device.  Raises RuntimeError when no gfx950 device is usable or the
    parameters are bad."""

    KERNEL_MS_FIELDS = ("predict_ms", "tag_ms", "resolve_ms", "decipher_ms", "predict_launches", "tag_launches",
                        "resolve_launches", "decipher_launches", "repaired_tags")
    _PREFIX = "tamd_recv"
    _LIB = RECV_LIB_PATH
    _CALLS = {"set_key": [vp, u32, u64],
              "reset": [vp, u32, u64],
              "receive": [vp, u32, u32p, u32p, vp, u64, i32p, vp],
              "next_expected": [vp, u32, u32p, u64p],
              "state": [vp, u32, u64p]}
    _REFUSED = {-1: "bad handle or null pointer", -2: "stream id out of range", -3: "pitch smaller than the largest datagram",
                -4: "device error"}

    def __init__(self, n_streams: int, max_datagram_bytes: int, device: int = 0):
        if not (0 < int(n_streams) < 2**32 and 0 < int(max_datagram_bytes) <= 65535):
            raise RuntimeError("tonk_amd: DatagramReceiver: bad parameters")
        self.n_streams, self.max_datagram_bytes = int(n_streams), int(max_datagram_bytes)
        self._create(_Params(int(device), int(n_streams), int(max_datagram_bytes)))

    def set_key(self, stream: int, key: int) -> None:
        """SimpleCipher::Initialize of one stream; takes effect with the next call."""
        self._check(self._c.set_key(self._h, int(stream), int(key) & 0xFFFFFFFFFFFFFFFF), "set_key")

    def reset(self, stream: int, base: int = 0) -> None:
        """StrikeRegister::Reset(base) of one stream."""
        self._check(self._c.reset(self._h, int(stream), int(base) & 0xFFFFFFFFFFFFFFFF), "reset")

    def receive(self, stream, nbytes, dev_datagrams, pitch: int):
        """Datagram i of stream[i], nbytes[i] bytes at dev_datagrams + i * pitch.  Returns (rc,
        result): the result codes (int32) and a record array with the fields of tamd_recv_result
        (all zero where rc is 1)."""
        import numpy as np
        S, B = arr(stream, "uint32"), arr(nbytes, "uint32")
        assert S.size == B.size
        rc = zeros(S.size, "int32")
        result = np.zeros(S.size, dtype=np.dtype(RESULT_FIELDS))
        assert result.dtype.itemsize == 24
        self._check(self._c.receive(self._h, S.size, ptr(S, u32p), ptr(B, u32p), _address(dev_datagrams), int(pitch), ptr(rc, i32p),
                                    result.ctypes.data_as(vp)), "receive")
        return rc, result

    def next_expected(self, stream):
        """LargestSequence + 1 of the streams named (uint64), from the host mirror: no device call."""
        S = arr(stream, "uint32")
        out = zeros(S.size, "uint64")
        self._check(self._c.next_expected(self._h, S.size, ptr(S, u32p), ptr(out, u64p)), "next_expected")
        return out

    def state(self, stream: int):
        """The stream's state read back from the device: 67 uint64 -- LargestSequence, WindowBase,
        WindowBitRotation, the 64 window words.  For tests and diagnostics."""
        out = zeros(STATE_WORDS, "uint64")
        self._check(self._c.state(self._h, int(stream), ptr(out, u64p)), "state")
        return out
