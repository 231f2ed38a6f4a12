"""Helpers of the compression step's tests (test_compress.py, test_decompress.py): the message
generators, the reference codec (oracle/msgcodec_py.py) with the decision to skip when it is not
built, the batch layouts, device memory for the calls that take device pointers, and concurrent
callers; and the host checker of compressor output (tests/native/lz_blocks.cpp) with the streams
aimed at the compression kernel's lengths."""
from __future__ import annotations

import ctypes
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from msgcodec_py import MAX, RefCompressor, RefDecompressor, read_cases, write_cases, write_streams  # noqa: F401
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


# ------------------------------------------- streams aimed at the compression kernel (lz.hip)

DICT = 24000  # kCompressionDictBytes: the history ring of both sides (lz.h TAMD_LZ_DICT)
SWEEP_LENGTHS = (8, 9, 11, 12, 15, 16, 17, 19, 20, 63, 64, 65, 191, 192, 193, 575, 576, 577, 1151, 1152, 1153, 1299, 1300,
                 1535, 1536, 1537, 2047, 2048, 2049, 4095, 4096, 4097, 16400, 23999, 24000)


def ring_positions(max_bytes, lens):
    """The history-ring rule (lz.h RingTrack, restated): (linear position, window start) of every
    message of a stream."""
    nxt = lin = seg = prev = 0
    have_prev = False
    out = []
    for n in lens:
        if nxt + max_bytes > DICT:
            if nxt:
                prev, have_prev, seg = seg, True, lin
            nxt = 0
        out.append((lin, min(prev + nxt + n, seg) if have_prev else seg))
        nxt += n
        lin += n
    return out


def lz_key_hash(data):
    """The compression kernel's bucket of every position of `data` with 8 bytes after it
    (lz.hip lz_hash: the top 12 bits of the 8-byte key times a 64-bit constant)."""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    n = len(a) - 7
    key = np.zeros(max(n, 0), dtype=np.uint64)
    for k in range(8):
        key |= a[k:k + n] << np.uint64(8 * k)
    return (key * np.uint64(0x9E3779B185EBCA87)) >> np.uint64(52)


def _random_with_lone_first_key(rng, n):
    """n random bytes; from 16 bytes on, no later position shares the first position's bucket of
    the kernel's hash table, so a repeat of the message finds its first byte's candidate whatever
    the table replaced (what a repeat reaches is still asserted from the record, never assumed)."""
    while True:
        m = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        if n < 16:
            return m
        h = lz_key_hash(m)
        if not (h[1:] == h[0]).any():
            return m


def length_sweep(max_bytes):
    """For every length of SWEEP_LENGTHS up to max_bytes, four messages in a row: random bytes, the
    same again, the same with one middle byte changed, the same with its first and last byte
    changed.  The lengths: the kernel's floor of 8, the 4-byte minimum match, the 16-byte probe,
    the 64-lane groups, the probe batch 3 x 64, the chunk of 576 positions and twice that, both
    sides of 1536 (LDS or scratch) and of 2048, the 2- and 3-byte literals headers, the length
    codes with 14 extra bits, the history size.

    From 64 bytes on two more follow, which carry their match inside themselves (at 24,000 every
    message starts a new history segment over the one before, lz.h RingTrack, so a repeat of an
    equal-length message has no history left to match): a quarter of the message four times over
    (one match of three quarters of the message that overlaps its own output), and three quarters
    of random bytes followed by the first quarter again (one long literal run, then a match)."""
    rng = np.random.default_rng(7000 + max_bytes)
    msgs = []
    for n in SWEEP_LENGTHS:
        if n > max_bytes:
            continue
        m = _random_with_lone_first_key(rng, n)
        mid = bytearray(m)
        mid[n // 2] ^= 0x55
        ends = bytearray(m)
        ends[0] ^= 0x55
        ends[-1] ^= 0x55
        msgs += [m, m, bytes(mid), bytes(ends)]
        if n >= 64:
            q = n // 4
            quarter = rng.integers(0, 256, n - 3 * q, dtype=np.uint8).tobytes()
            msgs.append((quarter * 4)[:n])
            body = rng.integers(0, 256, n - q, dtype=np.uint8).tobytes()
            msgs.append(body + body[:q])
    return msgs


def word_shuffle(k, word, gap, seed=0, jitter=0, filler=0):
    """A message of k distinct random words of `word` bytes (>= 8: the kernel keys candidates by
    8 bytes), then `filler` messages of 1300 random bytes, then a message of the same words in a
    seeded permutation with `gap` fresh random bytes in front of each: about k sequences.  With
    jitter j the words' and gaps' lengths vary over j + 1 values (several length codes); with
    jitter 0 every sequence has the same two length codes, and with a filler much longer than the
    two messages all offsets fall in one power-of-two band."""
    rng = np.random.default_rng(seed)
    words = [rng.integers(0, 256, word + (j % (jitter + 1)), dtype=np.uint8).tobytes() for j in range(k)]
    first = b"".join(words)
    parts = []
    for i, j in enumerate(rng.permutation(k)):
        parts.append(rng.integers(0, 256, gap + (i % (jitter + 1)), dtype=np.uint8).tobytes())
        parts.append(words[int(j)])
    fill = [rng.integers(0, 256, 1300, dtype=np.uint8).tobytes() for _ in range(filler)]
    return [first] + fill + [b"".join(parts)]


RING_EDGE_KS = (1, 7, 8, 15, 16, 63, 64, 65)


def ring_edge(ks=RING_EDGE_KS, max_bytes=MAX, laps=2):
    """For the per-message API, whose 64 KB device ring has a 64-byte mirror: the stream's running
    byte count is brought to c * 65536 - k, for k of `ks` in turn and `laps` times over, and there
    follow a message whose first half repeats the end of the one before (the match's target
    crosses the ring's end) and one that repeats the bytes from 100 before that point to 200 after
    it (the match's source crosses it).  Between them: text, random bytes and repeats."""
    rng = np.random.default_rng(65536)
    words = [b"siamese ", b"tonk ", b"packet ", b"recovery ", b"window ", b"lane "]
    stream = bytearray()
    msgs = []

    def push(m):
        msgs.append(bytes(m))
        stream.extend(m)

    for c in range(len(ks) * laps):
        target = (c + 1) * 65536 - ks[c % len(ks)]
        while target - len(stream) > 2 * max_bytes:
            n = int(rng.integers(200, max_bytes + 1))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                push(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
            elif kind == 1 and len(stream) > 3000:
                at = len(stream) - int(rng.integers(n, 3000))
                push(stream[at:at + n])
            else:
                push(b"".join(words[int(i)] for i in rng.integers(0, len(words), n // 5 + 1))[:n])
        left = target - len(stream)  # in (max, 2 max]: two messages of at least 8 bytes
        a = left // 2
        push(rng.integers(0, 256, a, dtype=np.uint8).tobytes())
        push(rng.integers(0, 256, left - a, dtype=np.uint8).tobytes())
        assert len(stream) == target
        h = 300
        push(bytes(stream[-h:]) + rng.integers(0, 256, h, dtype=np.uint8).tobytes())
        push(bytes(stream[target - 100:target + 200]) + rng.integers(0, 256, 100, dtype=np.uint8).tobytes())
    return msgs


# ------------------------------------------- the host checker of compressor output (lz_blocks)

def lz_blocks_exe(which="lz_blocks"):
    """tests/native/_build/lz_blocks, made on demand where it is not there (the build makes the
    plain program; the sanitizer build is made by the CPU test that runs it)."""
    from conftest import NATIVE, _make
    exe = os.path.join(NATIVE, "_build", which)
    if which != "lz_blocks" or not os.path.exists(exe):
        _make(NATIVE, f"_build/{which}")
    return exe


def lz_blocks_check(path, which="lz_blocks"):
    """The checker over a case file: (exit status, the per-stream records, the total, stderr)."""
    r = subprocess.run([lz_blocks_exe(which), "check", path], capture_output=True, text=True, timeout=600)
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    total = [x for x in recs if x.get("total")]
    return r.returncode, [x for x in recs if not x.get("total")], total[0] if total else None, r.stdout[-2000:] + r.stderr[-4000:]


def checked_record(tmp_path, streams, name="cases.bin"):
    """Hands [(max, [(message, block)])] to the checker, asserts that it accepts every block, and
    returns the reach record of the whole file."""
    path = str(tmp_path / name)
    write_cases(path, streams)
    rc, recs, total, text = lz_blocks_check(path)
    bad = [(x["stream"], x["failed_message"], x["reason"]) for x in recs if not x["ok"]]
    assert rc == 0 and not bad and total and total["ok"], (bad, text)
    return total


def batch_cases(streams, max_bytes, raw, written):
    """The output of a compress batch as the checker's cases: [(max, [(message, block)])]."""
    n_msgs = len(streams[0])
    out = np.frombuffer(raw, dtype=np.uint8)
    cases = []
    for s, msgs in enumerate(streams):
        row = []
        for k, m in enumerate(msgs):
            i = s * n_msgs + k
            row.append((m, out[i * max_bytes:i * max_bytes + written[i]].tobytes()))
        cases.append((max_bytes, row))
    return cases


def pad_streams(streams, pad=b"p"):
    """Streams of one batch have the same number of messages: the shorter ones get one-byte
    messages (below the kernel's floor: sent as is) at their end."""
    n = max(len(s) for s in streams)
    return [list(s) + [pad] * (n - len(s)) for s in streams]


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
