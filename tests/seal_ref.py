"""Tonk's datagram cipher and tag restated in numpy and Python integers, for tests/test_seal.py
and tests/test_seal_gpu.py: the keystream is one vectorised expression, t1ha runs over Python
integers.  Checked against the recorded outputs of the reference (tests/golden/seal_kat.txt.gz);
the GPU tests use it to name the first differing byte and for shapes beyond the fixture.  Test
infrastructure only."""
from __future__ import annotations

import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "seal_kat.txt.gz")
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
P = (0x905c4577, 0xb84c88cb, 0xde0efbf1, 0x9f614c3d)
T1 = (17048867929148541611, 9386433910765580089, 15343884574428479051, 13662985319504319857,
      11242949449147999147, 13862205317416547141, 14653293970879851569)


def payload(length: int, msg: int) -> np.ndarray:
    """Byte i of a case is (i * 131 + len * 7 + msg * 13 + 1) & 255."""
    i = np.arange(length, dtype=np.uint64)
    return ((i * 131 + length * 7 + msg * 13 + 1) & 255).astype(np.uint8)


def maf19(a: int, b: int) -> int:
    p = (a & M32) * (b & M32)
    return (p ^ (p >> 19)) & M32


def expand(key: int):
    k0, k1 = key & M32, (key >> 32) & M32
    return (k0, k1, maf19(0xe7988061, k0), maf19(0xbd9fa5c7, k1))


def adder(seq: int):
    n0 = ((seq & M32) + 0x80771ab1) & M32
    n1 = maf19(((seq >> 32) + 0x55f2cc88) & M32, 0xf3f77d13)
    return tuple((maf19(p, n0) + n1) & M32 for p in P)


def keystream(key: int, seq: int, n: int) -> np.ndarray:
    """The n bytes Cipher XORs into the data: byte q is byte q & 3 of W(q >> 2)."""
    K, A = np.array(expand(key), dtype=np.uint64), np.array(adder(seq), dtype=np.uint64)
    w = np.arange((n + 3) // 4, dtype=np.uint64)
    W = ((K[w & 3] + ((w >> 2) + 1) * A[w & 3]) & M32).astype("<u4")
    return W.view(np.uint8)[:n]


def cipher(data: np.ndarray, key: int, seq: int, n=None) -> np.ndarray:
    """Cipher over the first n bytes (all by default); a copy."""
    out = np.array(data, dtype=np.uint8)
    n = out.size if n is None else n
    if key & M64:
        out[:n] ^= keystream(key, seq, n)
    return out


def rot64(v: int, s: int) -> int:
    return ((v >> s) | (v << (64 - s))) & M64


def mux64(v: int, p: int) -> int:
    r = v * p
    return (r ^ (r >> 64)) & M64


def t1ha(data: bytes, seed: int) -> int:
    n = len(data)
    a, b, at = seed & M64, n, 0
    word = lambda o, k=8: int.from_bytes(data[o:o + k], "little")
    if n > 32:
        c, d = (rot64(n, 17) + seed) & M64, n ^ rot64(seed, 17)
        while n - at >= 32:
            w0, w1, w2, w3 = (word(at + 8 * k) for k in range(4))
            d02 = w0 ^ rot64((w2 + d) & M64, 17)
            c13 = w1 ^ rot64((w3 + c) & M64, 17)
            c = (c + (a ^ rot64(w0, 41))) & M64
            d = (d - (b ^ rot64(w1, 31))) & M64
            a ^= (T1[1] * ((d02 + w3) & M64)) & M64
            b ^= (T1[0] * ((c13 + w2) & M64)) & M64
            at += 32
        a ^= (T1[6] * ((rot64(c, 17) + d) & M64)) & M64
        b ^= (T1[5] * ((c + rot64(d, 17)) & M64)) & M64
    rem = n - at
    if rem > 24:
        b = (b + mux64(word(at), T1[4])) & M64
        at += 8
    if rem > 16:
        a = (a + mux64(word(at), T1[3])) & M64
        at += 8
    if rem > 8:
        b = (b + mux64(word(at), T1[2])) & M64
        at += 8
    if rem > 0:
        a = (a + mux64(word(at, n - at), T1[1])) & M64
    x = ((a ^ b) * T1[0]) & M64
    return (mux64(rot64((a + b) & M64, 17), T1[4]) + (x ^ rot64(x, 41))) & M64


def tag(data, key: int, seq: int) -> int:
    return (t1ha(bytes(data), (seq ^ key) & M64) >> 19) & 0xFFFF


def tag_int(key: int, value: int) -> int:
    k0, k1 = key & M32, (key >> 32) & M32
    prod = k0 * ((value ^ k1) & M32)
    return ((prod ^ rot64(prod, 41)) >> 19) & 0xFFFF


def seal(data: np.ndarray, key: int, nonce: int, msg: int) -> np.ndarray:
    """A whole datagram (timestamp and flags in place) sealed; a copy."""
    T = data.size - 6
    out = cipher(data, key, nonce, msg)
    ts24 = int(out[T]) | int(out[T + 1]) << 8 | int(out[T + 2]) << 16
    t = tag(out[:T], key, nonce) ^ tag_int(key, ts24 << 8 | int(out[T + 3]))
    out[T + 4], out[T + 5] = t & 255, t >> 8
    return out


def open_(data: np.ndarray, key: int, nonce: int, msg: int):
    """(rc, datagram after the call)."""
    T = data.size - 6
    ts24 = int(data[T]) | int(data[T + 1]) << 8 | int(data[T + 2]) << 16
    t = tag(data[:T], key, nonce) ^ tag_int(key, ts24 << 8 | int(data[T + 3]))
    if t != (int(data[T + 4]) | int(data[T + 5]) << 8):
        return 2, np.array(data, dtype=np.uint8)
    return 0, cipher(data, key, nonce, msg)


def datagram(nbytes: int, msg: int, ts24: int, flags: int) -> np.ndarray:
    """A D case before it is sealed: the payload rule, then timestamp and flags; tag bytes 0."""
    d = payload(nbytes, msg)
    T = nbytes - 6
    d[T:] = [ts24 & 255, (ts24 >> 8) & 255, ts24 >> 16, flags, 0, 0]
    return d


def fnv1a(b) -> int:
    """oracle_py.fnv1a, vectorised enough for 64 KB cases."""
    h = 1469598103934665603
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & M64
    return h


_kat = None


def kat():
    """The fixture's lines: {"C": [(key, seq, len, msg, tag, fnv)], "I": [(key, data, tag)],
    "D": [(key, seq, bytes, msg, ts24, flags, fnv)]}."""
    global _kat
    if _kat is None:
        out = {"C": [], "I": [], "D": []}
        with gzip.open(KAT, "rt") as f:
            for ln in f:
                p = ln.split()
                out[p[0]].append(tuple(int(x, 0) for x in p[1:]))
        _kat = out
    return _kat


def first_difference(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return "equal" if bad.size == 0 else f"first differing byte {bad[0]}: got {got[bad[0]]:#04x}, want {want[bad[0]]:#04x} ({bad.size} differ)"
