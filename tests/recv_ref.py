"""The front of Tonk's receive path restated in Python integers, for tests/test_recv.py and
tests/test_recv_gpu.py: the footer read, CounterExpand, StrikeRegister's IsDuplicate and Accept and
ProcessDatagram's order of checks, over tests/seal_ref.py's cipher and tag.  Checked against the
recorded transcripts of the reference (tests/golden/recv_kat.txt.gz); the GPU tests take their
expectations from it, because the GPU machine has no reference.  Test infrastructure only."""
from __future__ import annotations

import gzip
import os

import numpy as np

import seal_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "recv_kat.txt.gz")
M64 = S.M64
BITS, WORDS = 4096, 64
OK, INVALID, BAD_TAG, DUPLICATE, REORDERED = 0, 1, 2, 3, 4


def less(a: int, b: int) -> bool:
    """a < b as Counter64 compares."""
    return ((a - b) & M64) >= 1 << 63


def expand(largest: int, partial: int, nb: int) -> int:
    if nb == 0:
        return (largest + 1) & M64
    bits = 8 * nb
    gap = (partial - largest) & ((1 << bits) - 1)
    if gap >> (bits - 1):
        gap -= 1 << bits
    return (largest + gap) & M64


def footer_bytes(flags: int) -> int:
    return 6 + (12 if flags & 0x40 else 0) + ((flags >> 2) & 3) + (flags & 3)


class Register:
    """security::StrikeRegister."""

    def __init__(self, base: int = 0):
        self.reset(base)

    def reset(self, base: int) -> None:
        self.largest = self.base = base & M64
        self.rotation = 0
        self.window = [0] * WORDS

    def is_duplicate(self, seq: int) -> bool:
        if less(seq, self.base):
            return True
        distance = (seq - self.base) & M64
        if distance >= BITS:
            return False
        bit = (distance + self.rotation) % BITS
        return bool(self.window[bit // 64] >> (bit % 64) & 1)

    def accept(self, seq: int) -> None:
        if less(self.largest, seq):
            self.largest = seq
        if less(seq, self.base):
            return
        distance = (seq - self.base) & M64
        if distance >= BITS:
            slide = (distance - BITS) // 64 + 1
            if slide >= WORDS:
                self.reset(seq)
                self.window[0] = 1
                return
            word = self.rotation // 64
            for _ in range(slide):
                self.window[word] = 0
                word = (word + 1) % WORDS
            self.base = (self.base + slide * 64) & M64
            self.rotation = (self.rotation + slide * 64) % BITS
            distance -= slide * 64
        bit = (distance + self.rotation) % BITS
        self.window[bit // 64] |= 1 << (bit % 64)

    def words(self) -> np.ndarray:
        """What tamd_recv_state returns."""
        return np.array([self.largest, self.base, self.rotation] + self.window, dtype=np.uint64)

    def window_fnv(self) -> int:
        return S.fnv1a(np.array(self.window, dtype="<u8").tobytes())


class Connection:
    """One stream of the receiver: key and register."""

    def __init__(self, key: int = 0, base: int = 0):
        self.key, self.reg = key & M64, Register(base)

    def receive(self, data: np.ndarray, max_bytes: int = 65535):
        """(rc, result dict or None, the datagram after the call)."""
        n = int(data.size)
        if n < 6 or n > max_bytes:
            return INVALID, None, data
        flags = int(data[n - 3])
        if not flags & 0x80 or n < footer_bytes(flags):
            return INVALID, None, data
        hs, nb, sb = (12 if flags & 0x40 else 0), (flags >> 2) & 3, flags & 3
        T = n - 6
        field = lambda end, k: int.from_bytes(bytes(data[end - k:end]), "little")
        nonce = expand(self.reg.largest, field(T - hs, nb), nb)
        msg = n - footer_bytes(flags)
        res = dict(nonce=nonce, message_bytes=msg, timestamp24=field(T + 3, 3), partial_seq=field(T - hs - nb, sb), flags=flags,
                   seq_bytes=sb, nonce_bytes=nb, handshake_bytes=hs)
        if self.reg.is_duplicate(nonce):
            return DUPLICATE, res, data
        rc, after = S.open_(data, self.key, nonce, msg)
        if rc:
            return BAD_TAG, res, data
        self.reg.accept(nonce)
        if 0 < sb < nb and less((nonce + 1) & M64, (self.reg.largest + 1) & M64):
            return REORDERED, res, after
        return OK, res, after


def wire(key: int, k: int, nonce: int, nb: int, sb: int, hs: int, nbytes: int, corrupt: int = 0) -> np.ndarray:
    """Datagram k of a connection of the fixture as its sender made it (tests/native/recv_golden.cpp)."""
    F = 6 + (12 if hs else 0) + nb + sb
    M, T = nbytes - F, nbytes - 6
    i = np.arange(M, dtype=np.uint64)
    d = np.zeros(nbytes, dtype=np.uint8)
    d[:M] = ((i * 131 + nbytes * 7 + k * 13 + 1) & 255).astype(np.uint8)
    seq = (k * 40503 + 7) & 0xFFFFFFFF
    foot = list(seq.to_bytes(4, "little")[:sb]) + list((nonce & M64).to_bytes(8, "little")[:nb])
    if hs:
        foot += [(k + j * 17 + 3) & 255 for j in range(12)]
    ts24 = (k * 2654435761 + nbytes) & 0xFFFFFF
    flags = 0x80 | (0x40 if hs else 0) | (0x20 if k % 3 == 0 else 0) | nb << 2 | sb
    foot += list(ts24.to_bytes(3, "little")) + [flags, 0, 0]
    d[M:] = foot
    d = S.seal(d, key, nonce, M)
    if corrupt:
        t = (int(d[T + 4]) | int(d[T + 5]) << 8) ^ (1 << ((corrupt - 1) & 15))
        d[T + 4], d[T + 5] = t & 255, t >> 8
    return d


_kat = None


def kat():
    """The fixture's transcripts: [(key, base, [G line as a tuple of 13 ints])]."""
    global _kat
    if _kat is None:
        out = []
        with gzip.open(KAT, "rt") as f:
            for ln in f:
                p = ln.split()
                v = tuple(int(x, 0) for x in p[1:])
                if p[0] == "S":
                    out.append((v[0], v[1], []))
                else:
                    assert p[0] == "G" and len(v) == 13
                    out[-1][2].append(v)
        _kat = out
    return _kat
