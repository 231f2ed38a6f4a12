"""Helpers of the compression step's tests (test_compress.py, test_decompress.py): the message
generators, the reference codec (oracle/msgcodec_py.py) with the decision to skip when it is not
built, the batch layouts, device memory for the calls that take device pointers, and concurrent
callers."""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np
import pytest

from msgcodec_py import MAX, RefCompressor, RefDecompressor, read_cases, write_streams  # noqa: F401
import msgcodec_py


def ref_lib():
    if not os.path.exists(msgcodec_py.REF):
        pytest.skip("oracle/_ref/libmsgcodec_ref.so not built (needs /root/reference at build time)")
    return msgcodec_py.load()


# ------------------------------------------------------------------------------- generators

class Pcg:
    """siamese::PCGRandom (SiameseTools.h:80-102)."""
    M = (1 << 64) - 1

    def __init__(self, y, x=0):
        self.state, self.inc = 0, ((y << 1) | 1) & self.M
        self.next()
        self.state = (self.state + x) & self.M
        self.next()

    def next(self) -> int:
        old = self.state
        self.state = (old * 6364136223846793005 + self.inc) & self.M
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF


def tonk_unit_messages():
    """TestCompression's stream (TonkUnitTest.cpp:599-700): 100 messages of 400 PCG bytes, seeds
    0..49 then 50..1 (the second half repeats the first in reverse)."""
    out = []
    for i in range(100):
        seed = 100 - i if i >= 50 else i
        p = Pcg(seed)
        out.append(b"".join(p.next().to_bytes(4, "little") for _ in range(100)))
    return out


def mixed_messages(n, seed, max_bytes=MAX):
    """Text-like runs, random bytes and repeats of earlier stretches; lengths 8..max_bytes."""
    rng = np.random.default_rng(seed)
    words = [b"siamese ", b"tonk ", b"packet ", b"recovery ", b"window ", b"lane ", b"sum ", b"ack ", b"0123 "]
    stream = bytearray()
    msgs = []
    for _ in range(n):
        ln = int(rng.integers(8, max_bytes + 1))
        kind = int(rng.integers(0, 4))
        if kind == 3 and len(stream) > 4000:
            start = len(stream) - 1 - int(rng.integers(0, min(len(stream) - 1, 40000)))
            m = bytes(stream[start:start + ln]).ljust(ln, b"x")
        elif kind == 0:
            m = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        else:
            parts = []
            total = 0
            while total < ln:
                parts.append(words[int(rng.integers(0, len(words)))])
                total += len(parts[-1])
            m = b"".join(parts)[:ln]
        stream += m
        msgs.append(m)
    return msgs


def skewed(n, seed, max_bytes):
    """Lengths 64..max, bytes drawn from 64 symbols with probability ~ 2^(-i/3)."""
    rng = np.random.default_rng(seed)
    p = 2.0 ** (-np.arange(64) / 3.0)
    p /= p.sum()
    return [rng.choice(64, size=int(rng.integers(64, max_bytes + 1)), p=p).astype(np.uint8).tobytes() for _ in range(n)]


def edge_case_messages(max_bytes):
    """Tiny messages, runs of one byte, messages of exactly max bytes, messages above 2048 bytes
    and repeats of the one before (test_compress.test_gpu_compressor_edge_cases)."""
    rng = np.random.default_rng(max_bytes)
    top = max_bytes
    msgs = []
    for k in range(300):
        kind = k % 6
        if kind == 0:
            msgs.append(bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8)))
        elif kind == 1:
            msgs.append(bytes([k & 0xFF]) * int(rng.integers(9, top + 1)))
        elif kind == 2:
            msgs.append((b"abc" * top)[:top])
        elif kind == 3:
            msgs.append(bytes(rng.integers(0, 4, top, dtype=np.uint8)))
        elif kind == 4 and max_bytes > 2048:
            msgs.append((b"tonk siamese " * 400)[:int(rng.integers(2049, max_bytes + 1))])
        else:
            msgs.append(msgs[-1] if msgs else b"x" * 20)
    return msgs


def rep_offsets(n, seed, max_bytes=MAX):
    """Records of a fixed stride with a few bytes changed from one to the next: matches separated
    by short (and no) literal runs at the distances just used, the repeat-offset cases."""
    rng = np.random.default_rng(seed)
    msgs = []
    for _ in range(n):
        stride = int(rng.integers(24, 90))
        rec = bytearray(rng.integers(0, 256, stride, dtype=np.uint8).tobytes())
        m = bytearray()
        while len(m) < int(rng.integers(300, max_bytes + 1)):
            kind = int(rng.integers(0, 6))
            if kind == 0:  # a byte changes
                rec[int(rng.integers(0, stride))] = int(rng.integers(0, 256))
                m += rec
            elif kind == 1:  # a byte is left out: the distance shortens by one
                cut = int(rng.integers(1, stride - 1))
                m += rec[:cut] + rec[cut + 1:]
            elif kind == 2:  # two distances alternate
                m += rec + rec[:stride // 2]
            else:
                m += rec
        msgs.append(bytes(m[:max_bytes]))
    return msgs


# ---------------------------------------------------------------------------- batch layouts

def pack_streams(streams):
    """The compress batch's input: every stream's messages end to end in its row of a strided
    host array.  Returns (host, stride, lens per message)."""
    stride = max(sum(map(len, s)) for s in streams) + 64
    host = np.zeros((len(streams), stride), dtype=np.uint8)
    lens = []
    for s, ms in enumerate(streams):
        blob = b"".join(ms)
        host[s, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        lens += [len(m) for m in ms]
    return host, stride, lens


def ref_slots(L, streams, max_bytes):
    """Reference-compressed streams in the batch layout: (slots, in_bytes, is_block)."""
    n_msgs = len(streams[0])
    slots = np.zeros((len(streams) * n_msgs, max_bytes), dtype=np.uint8)
    in_bytes, is_block = [], []
    for s, msgs in enumerate(streams):
        comp = RefCompressor(L, max_bytes)
        for k, m in enumerate(msgs):
            blk = comp.compress(m)
            data = blk if blk else m
            slots[s * n_msgs + k, :len(data)] = np.frombuffer(data, dtype=np.uint8)
            in_bytes.append(len(data))
            is_block.append(1 if blk else 0)
    return slots, in_bytes, is_block


def check_batch(streams, max_bytes, out, restored, status):
    n_msgs = len(streams[0])
    out = np.frombuffer(out, dtype=np.uint8).reshape(-1, max_bytes)
    for s, msgs in enumerate(streams):
        for k, m in enumerate(msgs):
            i = s * n_msgs + k
            assert status[i] == 0 and restored[i] == len(m), (s, k, status[i], restored[i])
            assert out[i, :len(m)].tobytes() == m, (s, k)


class Hip:
    """Device memory through the HIP runtime the library itself uses (the one mapped into this
    process with it), for the tests that hand device pointers to the batch calls."""

    def __init__(self):
        import tonk_amd
        tonk_amd.lib()
        # (the library binds to the runtime already in the process when torch brought one first,
        # else to the system's: the copy outside torch is the library's own whenever there is one)
        with open("/proc/self/maps") as f:
            paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln}, key=lambda p: "/torch/" in p)
        path = paths[0]
        L = self.L = ctypes.CDLL(path)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
        L.hipFree.argtypes = [vp]
        L.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
        L.hipMemset.argtypes = [vp, ctypes.c_int, sz]
        L.hipDeviceSynchronize.argtypes = []
        self.owned = []

    def malloc(self, n, fill=0):
        p = ctypes.c_void_p()
        assert self.L.hipMalloc(ctypes.byref(p), n) == 0
        self.owned.append(p.value)
        assert self.L.hipMemset(p.value, fill, n) == 0
        return p.value

    def upload(self, ptr, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        assert self.L.hipMemcpy(ptr, arr.ctypes.data, arr.size, 1) == 0  # hipMemcpyHostToDevice

    def download(self, ptr, n):
        out = np.empty(n, dtype=np.uint8)
        assert self.L.hipMemcpy(out.ctypes.data, ptr, n, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def copy(self, dst, src, n):
        assert self.L.hipMemcpy(dst, src, n, 3) == 0  # hipMemcpyDeviceToDevice

    def close(self):
        self.L.hipDeviceSynchronize()
        for p in self.owned:
            self.L.hipFree(p)
        self.owned = []


def run_threads(n_threads, worker):
    """worker(t, errors) on n_threads threads at the same time (Tonk's connection threads); every
    call must return.  Returns `errors`: what the workers appended, and any exception's repr."""
    errors = []

    def run(t):
        try:
            worker(t, errors)
        except Exception as e:  # (surfaced by the caller's assertion)
            errors.append(repr(e))

    th = [threading.Thread(target=run, args=(t,)) for t in range(n_threads)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not any(x.is_alive() for x in th), "a call did not return"
    return errors
