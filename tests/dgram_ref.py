"""Tonk's message frames, datagram footers and the receiver's walk restated in Python and numpy,
for tests/test_dgram.py and tests/test_dgram_gpu.py.  Checked against the recorded results of the
reference (tests/golden/dgram_kat.txt.gz, written by tests/native/dgram_golden.cpp, which states
the line formats, the draws and the section generators); the GPU tests use it to regenerate every
line's inputs and for shapes beyond the fixture.  Test infrastructure only."""
from __future__ import annotations

import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "dgram_kat.txt.gz")
M32 = 0xFFFFFFFF
ACKACK, PADDING, RELIABLE, RAW = 2, 4, 5, 255
SEQCOMP, ONLYFEC = 0x20, 0x10
TYPES = (3, 6, 0, 5, 31, 1)


def mix(seed: int, c):
    """The draw's 32-bit mix; c an int or a uint64 array of counters."""
    h = (seed ^ (c * 0x9E3779B1)) & M32
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


class Draw:
    def __init__(self, seed: int):
        self.seed, self.c = seed, 0

    def fill(self, n: int) -> np.ndarray:
        c = np.arange(self.c, self.c + n, dtype=np.uint64)
        self.c += n
        return (mix(self.seed, c) & 255).astype(np.uint8)

    def word(self, n: int) -> int:
        return int.from_bytes(self.fill(n).tobytes(), "little")


def fnv1a(b) -> int:
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def header(mtype: int, nbytes: int) -> bytes:
    return ((mtype << 11 | nbytes) & 0xFFFF).to_bytes(2, "little")


def flags_byte(seq_bytes, nonce_bytes, handshake, flag_bits) -> int:
    return 0x80 | (0x40 if handshake else 0) | (flag_bits & (SEQCOMP | ONLYFEC)) | nonce_bytes << 2 | seq_bytes


def footer(seq, seq_bytes, nonce, nonce_bytes, handshake, ts24, flag_bits) -> bytes:
    """`handshake`: 12 bytes or None.  The two tag bytes are zeros."""
    out = (seq & M32).to_bytes(4, "little")[:seq_bytes] + (nonce & M32).to_bytes(4, "little")[:nonce_bytes]
    out += bytes(handshake) if handshake is not None else b""
    return out + (ts24 & 0xFFFFFF).to_bytes(3, "little") + bytes([flags_byte(seq_bytes, nonce_bytes, handshake is not None, flag_bits), 0, 0])


def build(msgs, seq, seq_bytes, nonce, nonce_bytes, handshake, ts24, flag_bits, max_bytes=65535, pitch=1 << 40):
    """msgs: [(type, body bytes)].  Returns (rc, datagram bytes, message_bytes, reliable_offset,
    reliable_bytes); rc 1 with nothing else when the input is invalid (tonk_datagram.h)."""
    bad = (1, b"", 0, 0, 0)
    if seq_bytes > 3 or nonce_bytes > 3:
        return bad
    only_fec = bool(flag_bits & ONLYFEC)
    if only_fec and (len(msgs) != 1 or msgs[0][0] != RAW or seq_bytes):
        return bad
    out, lo, hi, padded = b"", 0, 0, False
    for t, body in msgs:
        body = bytes(body)
        if only_fec:
            out += body
            break
        if t > 31 or len(body) > 2047:
            return bad
        if t >= RELIABLE:
            if padded:
                return bad
            if hi == 0:
                lo = len(out)
            hi = len(out) + 2 + len(body)
        elif hi:
            if t != PADDING:
                return bad
            padded = True
        out += header(t, len(body)) + body
        if len(out) > 65535:
            return bad
    if hi and not seq_bytes:
        return bad
    msg = len(out)
    out += footer(seq, seq_bytes, nonce, nonce_bytes, handshake, ts24, flag_bits)
    if len(out) > max_bytes or len(out) > pitch:
        return bad
    return 0, out, msg, lo, hi - lo


def parse(section, mode: int = 0):
    """The walk of a message section: (status, entries, reliable_offset, reliable_bytes); entries
    type << 27 | bytes << 16 | payload_offset for every frame walked before the end or the error."""
    s = bytes(section)
    pos, entries, lo, hi, status = 0, [], 0, 0, 0
    while len(s) - pos >= 2:
        h = s[pos] | s[pos + 1] << 8
        n, t = h & 2047, h >> 11
        if len(s) - pos - 2 < n:
            status = 2
            break
        if mode == 0 and t == ACKACK and n != 3:
            status = 4
            break
        entries.append(t << 27 | n << 16 | (pos + 2))
        if t >= RELIABLE:
            if hi == 0:
                lo = pos
            hi = pos + 2 + n
        pos += 2 + n
    if status == 0 and len(s) - pos > 0:
        status = 3
    return status, entries, lo, hi - lo


def table_fnv(entries) -> int:
    return fnv1a(np.asarray(entries, dtype="<u4").tobytes())


# ---- the fixture ----

def b_inputs(line):
    """A B line's inputs as drawn from its seed: dict(seq, nonce, ts24, handshake (12 bytes or None),
    msgs [(type, body or None for Padding's zeros)]) beside its fields."""
    d = Draw(line["seed"])
    seq, nonce, ts24 = d.word(4), d.word(4), d.word(3)
    hs = d.fill(12).tobytes()
    msgs = [(t, None if t == PADDING else d.fill(n).tobytes(), n) for t, n in line["msgs"]]
    return dict(seq=seq, nonce=nonce, ts24=ts24, handshake=hs if line["handshake"] else None, msgs=msgs)


def b_build(line):
    """build() of a B line: (rc, bytes, message_bytes, reliable_offset, reliable_bytes)."""
    i = b_inputs(line)
    msgs = [(t, bytes(n) if body is None else body) for t, body, n in i["msgs"]]
    return build(msgs, i["seq"], line["seq_bytes"], i["nonce"], line["nonce_bytes"], i["handshake"], i["ts24"], line["flag_bits"])


def _frame(t, n, d):
    return header(t, n) + (d.fill(n).tobytes() if d else bytes(n))


def p_section(line, k=None) -> bytes:
    """The message section of a P line (generators of tests/native/dgram_golden.cpp)."""
    gen, a, b, c = line["gen"], line["a"], line["b"], line["c"]
    if gen == 0:
        k = kat() if k is None else k
        _, out, msg, _, _ = b_build(k["B"][a])
        return out[:msg]
    if gen == 1:
        d = Draw(1000 + a)
        return _frame(6 if a & 1 else 3, max(a, 2) - 2, d) + _frame(6, 7, d) + _frame(4, 1, d)
    if gen == 2:
        return b"".join(_frame(6 if i & 1 else 3, 0, None) for i in range(a))
    if gen == 3:
        return Draw(a).fill(b).tobytes()
    if gen == 4:
        d = Draw(4000 + a * 64 + b * 8 + c)
        frames = [_frame(TYPES[i % 6], (i * 5 + a) % 23, d) for i in range(a)]
        if c == 2:
            frames[b] = header(TYPES[b % 6], 2047) + frames[b][2:]
        elif c == 3:
            frames = frames[:b] + [b"\x5a"]
        else:
            frames[b] = _frame(ACKACK, c // 10, Draw(d.seed + 1000))
        return b"".join(frames)
    if gen == 5:
        d = Draw(5000)
        return b"".join(_frame(6, 2047, d) for _ in range(31)) + _frame(6, 65535 - 31 * 2049 - 2, d)
    raise ValueError(gen)


_kat = None


def kat():
    """{"B": [dict(seed, seq_bytes, nonce_bytes, handshake, flag_bits, msgs [(type, bytes)], out_bytes,
    message_bytes, reliable_offset, reliable_bytes, fnv)], "P": [dict(gen, a, b, c, bytes,
    modes [(status, count, reliable_offset, reliable_bytes, fnv)] x 2)]}."""
    global _kat
    if _kat is None:
        out = {"B": [], "P": []}
        with gzip.open(KAT, "rt") as f:
            for ln in f:
                p = ln.split()
                v = [int(x, 0) for x in p[1:]]
                if p[0] == "B":
                    cnt = v[5]
                    assert len(v) == 6 + 2 * cnt + 5
                    r = v[6 + 2 * cnt:]
                    out["B"].append(dict(seed=v[0], seq_bytes=v[1], nonce_bytes=v[2], handshake=v[3], flag_bits=v[4],
                                         msgs=[(v[6 + 2 * k], v[7 + 2 * k]) for k in range(cnt)], out_bytes=r[0],
                                         message_bytes=r[1], reliable_offset=r[2], reliable_bytes=r[3], fnv=r[4]))
                else:
                    assert p[0] == "P" and len(v) == 15
                    out["P"].append(dict(gen=v[0], a=v[1], b=v[2], c=v[3], bytes=v[4], modes=[tuple(v[5:10]), tuple(v[10:15])]))
        _kat = out
    return _kat


def first_difference(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return "equal" if bad.size == 0 else f"first differing byte {bad[0]}: got {got[bad[0]]:#04x}, want {want[bad[0]]:#04x} ({bad.size} differ)"
