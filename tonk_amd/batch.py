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

from ._handle import Handle, arr, cp, i32p, ptr, u8p, u32, u32p, u64, vp, zeros

RECOVERY_OVERHEAD = 11  # TAMD_BATCH_RECOVERY_OVERHEAD


class _Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("max_packet_bytes", ctypes.c_uint32),
                ("arena_bytes", ctypes.c_uint64)]


class BatchCodec(Handle):
    """`n_streams` encoder/decoder pairs over device packets.  Raises RuntimeError when no gfx950
    device is usable or the parameters are bad."""

    KERNEL_MS_FIELDS = ("frame_ms", "unframe_ms", "tails_ms", "program_ms", "frame_launches", "unframe_launches",
                        "tails_launches", "program_launches", "frame_bytes", "unframe_bytes")
    _PREFIX = "tamd_batch"
    _CALLS = {"encoder_add": [vp, u32, u32p, u32p, vp, u64, u32p, i32p],
              "encoder_add_at": [vp, u32, u32p, u32p, u32p, vp, u64, u32p, i32p],
              "decoder_add_original_at": [vp, u32, u32p, u32p, u32p, u32p, vp, u64, i32p],
              "encode": [vp, u32, u32p, vp, u64, u32p, i32p],
              "encoder_ack": [vp, u32, cp, u32, u32p],
              "decoder_add_original": [vp, u32, u32p, u32p, u32p, vp, u64, i32p],
              "decoder_add_recovery": [vp, u32, u32p, u32p, vp, u64, i32p],
              "decode": [vp, u32, u32p, vp, u64, u32, u32p, u32p, u32p, u32p, i32p],
              "decoder_ack": [vp, u32, u8p, u32, u32p]}
    _REFUSED = {-1: "bad handle or null pointer", -2: "stream id out of range", -3: "pitch smaller than the largest packet",
                -4: "device error"}

    def __init__(self, n_streams: int, max_packet_bytes: int, arena_bytes: int, device: int = 0):
        if not (0 < int(n_streams) < 2**32 and 0 < int(max_packet_bytes) <= 65535 and 0 < int(arena_bytes) < 2**64):
            raise RuntimeError("tonk_amd: BatchCodec: bad parameters")
        self.n_streams, self.max_packet_bytes = int(n_streams), int(max_packet_bytes)
        self._create(_Params(int(device), int(n_streams), int(max_packet_bytes), int(arena_bytes)))

    def encoder_add(self, stream, lens, dev_payloads: int, pitch: int, offset=None):
        """Add originals (packet i at dev_payloads + i * pitch + offset[i]); returns (packet numbers, result codes)."""
        S, L = arr(stream, "uint32"), arr(lens, "uint32")
        O = None if offset is None else arr(offset, "uint32")
        assert S.size == L.size and (O is None or O.size == S.size)
        pn, rc = zeros(S.size, "uint32"), zeros(S.size, "int32")
        self._check(self._c.encoder_add_at(self._h, S.size, ptr(S, u32p), ptr(L, u32p), ptr(O, u32p), dev_payloads, pitch,
                                           ptr(pn, u32p), ptr(rc, i32p)), "encoder_add")
        return pn, rc

    def encode(self, stream, dev_out: int, pitch: int):
        """One recovery packet per list entry at dev_out + i * pitch; returns (bytes, result codes)."""
        S = arr(stream, "uint32")
        nb, rc = zeros(S.size, "uint32"), zeros(S.size, "int32")
        self._check(self._c.encode(self._h, S.size, ptr(S, u32p), dev_out, pitch, ptr(nb, u32p), ptr(rc, i32p)), "encode")
        return nb, rc

    def encoder_ack(self, stream: int, data: bytes):
        """siamese_encoder_ack of one stream; returns (result code, next expected packet number)."""
        nxt = ctypes.c_uint32(0)
        rc = self._c.encoder_ack(self._h, stream, bytes(data), len(data), ctypes.byref(nxt))
        self._check(rc, "encoder_ack")
        return rc, int(nxt.value)

    def decoder_add_original(self, stream, packet_num, lens, dev_payloads: int, pitch: int, offset=None):
        """Add received originals (packet i at dev_payloads + i * pitch + offset[i]); returns the result codes."""
        S, P, L = arr(stream, "uint32"), arr(packet_num, "uint32"), arr(lens, "uint32")
        O = None if offset is None else arr(offset, "uint32")
        assert S.size == P.size == L.size and (O is None or O.size == S.size)
        rc = zeros(S.size, "int32")
        self._check(self._c.decoder_add_original_at(self._h, S.size, ptr(S, u32p), ptr(P, u32p), ptr(L, u32p), ptr(O, u32p),
                                                    dev_payloads, pitch, ptr(rc, i32p)), "decoder_add_original")
        return rc

    def decoder_add_recovery(self, stream, nbytes, dev_packets: int, pitch: int):
        """Add received recovery packets; returns the result codes."""
        S, B = arr(stream, "uint32"), arr(nbytes, "uint32")
        assert S.size == B.size
        rc = zeros(S.size, "int32")
        self._check(self._c.decoder_add_recovery(self._h, S.size, ptr(S, u32p), ptr(B, u32p), dev_packets, pitch, ptr(rc, i32p)),
                    "decoder_add_recovery")
        return rc

    def decode(self, stream, dev_out: int, pitch: int, cap: int):
        """Decode every listed stream that is ready; recovered payload j at dev_out + j * pitch.
        Returns (per-stream result codes, out_stream, out_packet_num, out_bytes)."""
        S = arr(stream, "uint32")
        rc = zeros(S.size, "int32")
        os_, op, ob = (zeros(max(cap, 1), "uint32") for _ in range(3))
        n = ctypes.c_uint32(0)
        self._check(self._c.decode(self._h, S.size, ptr(S, u32p), dev_out, pitch, cap, ptr(os_, u32p), ptr(op, u32p),
                                   ptr(ob, u32p), ctypes.byref(n), ptr(rc, i32p)), "decode")
        k = int(n.value)
        return rc, os_[:k].copy(), op[:k].copy(), ob[:k].copy()

    def decoder_ack(self, stream: int, limit: int = 256):
        """siamese_decoder_ack of one stream; returns (result code, ack bytes)."""
        buf = (ctypes.c_uint8 * max(limit, 1))()
        used = ctypes.c_uint32(0)
        rc = self._c.decoder_ack(self._h, stream, buf, limit, ctypes.byref(used))
        self._check(rc, "decoder_ack")
        return rc, bytes(buf[:used.value])
