"""The receive side of the compression step: tonk::MessageDecompressor on the GPU
(include/tonk_compress.h tamd_decompress*, tonk_amd/csrc/unlz.h / unlz.hip / decompress.cpp).

Parity is the reference's own pair (oracle/_ref/libmsgcodec_ref.so): its compressor's blocks are
the input, its decompressor's bytes the expected output.  The CPU tests run the block reader as a
serial host walk (tests/native/unlz_check.cpp) over every format path, and over malformed blocks
under the address and undefined-behaviour sanitizers; the GPU tests run the kernel through the
per-message API, the batch and the device-resident chain.
"""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

from conftest import NATIVE, ROOT, _make
from test_compress import MAX, RefCompressor, RefDecompressor, mixed_messages, ref_lib, tonk_unit_messages

STATUS_FAILED = -13  # TAMD_UNLZ_E_FAILED (tonk_amd/csrc/unlz.h)


# ------------------------------------------------------------------------------- generators

def mixed_messages_max(n, seed, max_bytes):
    """test_compress.mixed_messages with the lengths' upper end as a parameter."""
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
    """The list of test_compress.test_gpu_compressor_edge_cases."""
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


def cpu_streams():
    """(max, messages) of every stream the walk is checked on."""
    out = [(1300, tonk_unit_messages()), (1300, mixed_messages(300, 5)), (4000, mixed_messages_max(300, 5, 4000)),
           (24000, mixed_messages_max(48, 5, 24000)), (1300, skewed(120, 9, 1300)), (8000, skewed(40, 9, 8000)),
           (1300, rep_offsets(60, 3))]
    out += [(m, edge_case_messages(m)) for m in (1300, 4000, 24000)]
    return out


def write_streams(path, streams):
    """The stream file of unlz_check: raw messages (is_block 0)."""
    with open(path, "wb") as f:
        f.write(b"UNLZ" + struct.pack("<I", len(streams)))
        for max_bytes, msgs in streams:
            f.write(struct.pack("<II", max_bytes, len(msgs)))
            for m in msgs:
                f.write(struct.pack("<II", 0, len(m)) + m)


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


def unlz_check(which="unlz_check"):
    ref_lib()
    _make(NATIVE, "-f", "unlz.mk", f"_build/{which}")
    return os.path.join(NATIVE, "_build", which)


@pytest.fixture(scope="module")
def stream_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("unlz") / "streams.bin")
    write_streams(path, cpu_streams())
    return path


@pytest.fixture(scope="module")
def mutant_cases(stream_file, tmp_path_factory):
    """The malformed corpus through the plain build of the host walk: its 64 chosen cases, with
    the walk's verdicts, for the device.  (The sanitizer build runs the same corpus in the CPU
    suite only: test_malformed_blocks_under_sanitizers.)"""
    exe = unlz_check()
    out = str(tmp_path_factory.mktemp("unlz") / "cases.bin")
    r = subprocess.run([exe, "mutants", stream_file, out], capture_output=True, text=True, timeout=120)
    return r, out


# --------------------------------------------------------------------------------------- CPU

def test_block_reader_walk_matches_reference(stream_file, tmp_path):
    """Every stream at 1300 / 4000 / 8000 / 24000: the reference's blocks restored by the host
    walk equal the messages and the reference decompressor's bytes; the Repeat rewrites and the
    hand-made blocks equal the reference's bytes; the GPU compressor's format too; every path of
    the reader ran."""
    exe = unlz_check()
    r = subprocess.run([exe, "check", stream_file, str(tmp_path / "rewrites.bin")], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    paths = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("path ")]
    assert len(paths) == 32
    assert all(int(p[2]) > 0 for p in paths), paths
    assert len(read_cases(str(tmp_path / "rewrites.bin"), False)) > 4


def test_fse_tables_built_by_64_lanes():
    """The decode-table build's phases run for 64 lanes, phase by phase, equal the table built by
    one lane and the table built state by state, over 4,000 count distributions (the predefined
    ones, "less than one" symbols, up to 256 symbols, logs 5..9)."""
    exe = unlz_check()
    r = subprocess.run([exe, "tables"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_malformed_blocks_under_sanitizers(stream_file, mutant_cases, tmp_path):
    """Truncations, bit flips, an offset too far, a capacity too small: no sanitizer report, every
    unmutated block accepted, and whatever the walk accepts the reference restores the same.  The
    sanitizer build is made and run here only (a CPU test); it chooses the same 64 cases with the
    same verdicts as the plain build that the device test takes them from."""
    exe = unlz_check("unlz_check_san")
    out = str(tmp_path / "cases.bin")
    r = subprocess.run([exe, "mutants", stream_file, out], capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert len(read_cases(out, True)) == 64
    plain, plain_out = mutant_cases
    assert plain.returncode == 0 and plain.stdout == r.stdout
    with open(out, "rb") as a, open(plain_out, "rb") as b:
        assert a.read() == b.read()


def test_decompress_abi_exports_and_no_cpu_fallback():
    import tonk_amd
    path = tonk_amd.LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for sym in ("tamd_decompressor_create", "tamd_decompressor_insert_uncompressed", "tamd_decompressor_decompress",
                "tamd_decompressor_destroy", "tamd_decompress_batch", "tamd_decompress_batch_host"):
        assert f" T {sym}" in out, sym
    import torch
    if torch.cuda.is_available():
        return
    from tonk_amd.compress import MessageDecompressor
    with pytest.raises(RuntimeError):
        MessageDecompressor(MAX)


# --------------------------------------------------------------------------------------- GPU

def gpu_streams():
    return [(1300, tonk_unit_messages()), (1300, mixed_messages(300, 5)), (1300, skewed(120, 9, 1300))] + \
           [(m, edge_case_messages(m)) for m in (1300, 4000, 24000)]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6))
def test_gpu_decompressor_reference_blocks(which):
    """The per-message API on the reference compressor's blocks: the output equals the message
    every time (uncompressed messages go through insert_uncompressed)."""
    from tonk_amd.compress import MessageDecompressor
    L = ref_lib()
    max_bytes, msgs = gpu_streams()[which]
    comp, dec = RefCompressor(L, max_bytes), MessageDecompressor(max_bytes)
    n_blocks = 0
    for k, m in enumerate(msgs):
        blk = comp.compress(m)
        if blk:
            assert dec.decompress(blk) == m, k
            n_blocks += 1
        else:
            dec.insert_uncompressed(m)
    dec.close()
    assert n_blocks > len(msgs) // 4


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6))
def test_gpu_decompressor_gpu_blocks(which):
    """MessageCompressor's blocks restored by MessageDecompressor; the reference decompressor
    beside it as the tie-breaker."""
    from tonk_amd.compress import MessageCompressor, MessageDecompressor
    L = ref_lib()
    max_bytes, msgs = gpu_streams()[which]
    comp, dec, rdec = MessageCompressor(max_bytes), MessageDecompressor(max_bytes), RefDecompressor(L, max_bytes)
    n_blocks = 0
    for k, m in enumerate(msgs):
        blk = comp.compress(m)
        assert rdec.feed(blk, m) == m, k
        if blk:
            assert dec.decompress(blk) == m, k
            n_blocks += 1
        else:
            dec.insert_uncompressed(m)
    comp.close()
    dec.close()
    assert n_blocks > 0


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


@pytest.mark.gpu
def test_gpu_decompress_batch_streams():
    """16 streams x 120 messages of the mixed format in one decompress_batch_host call."""
    from tonk_amd.compress import decompress_batch_host
    L = ref_lib()
    streams = [mixed_messages(120, 100 + s) for s in range(16)]
    slots, in_bytes, is_block = ref_slots(L, streams, MAX)
    assert 0 < sum(is_block) < len(is_block)
    out, restored, status, ms = decompress_batch_host(slots.tobytes(), 16, 120, in_bytes, is_block, MAX)
    print(f"batch: kernel {ms:.3f} ms")
    check_batch(streams, MAX, out, restored, status)


@pytest.mark.gpu
def test_gpu_decompress_batch_large_messages():
    """4 streams x 24 messages at 24,000: Treeless literals, four Huffman streams, literals in
    global scratch, sequences in several chunks."""
    from tonk_amd.compress import decompress_batch_host
    L = ref_lib()
    max_bytes = 24000
    streams = [mixed_messages_max(24, 5, max_bytes), mixed_messages_max(24, 6, max_bytes),
               skewed(24, 9, max_bytes), skewed(24, 10, max_bytes)]
    slots, in_bytes, is_block = ref_slots(L, streams, max_bytes)
    types = {int(slots[i, 0]) & 3 for i in range(len(in_bytes)) if is_block[i]}
    assert {2, 3} <= types, types  # Compressed and Treeless literals are in the input
    out, restored, status, _ = decompress_batch_host(slots.tobytes(), 4, 24, in_bytes, is_block, max_bytes)
    check_batch(streams, max_bytes, out, restored, status)


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


@pytest.mark.gpu
def test_gpu_compress_then_decompress_on_device():
    """compress_batch then decompress_batch on device memory: the blocks never leave the device.
    Device pointers come from the HIP runtime the library uses, not from torch: by the time this
    test runs the library has initialised its runtime, and torch's own copy of the runtime,
    initialised second in one process, finds no device.  With torch first both use
    torch's: test_gpu_chain_on_torch_tensors runs that order in a process of its own."""
    from tonk_amd.compress import compress_batch, decompress_batch
    hip = Hip()
    n_streams, n_msgs = 8, 60
    streams = [mixed_messages(n_msgs, 200 + s) for s in range(n_streams)]
    stride = max(sum(map(len, s)) for s in streams) + 64
    host = np.zeros((n_streams, stride), dtype=np.uint8)
    lens = []
    for s, ms in enumerate(streams):
        blob = b"".join(ms)
        host[s, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        lens += [len(m) for m in ms]
    total = n_streams * n_msgs
    d_in = hip.malloc(host.size)
    hip.upload(d_in, host.reshape(-1))
    d_blocks = hip.malloc(total * MAX + 32)
    written, _ = compress_batch(d_in, stride, n_streams, n_msgs, lens, MAX, d_blocks)
    assert (written > 0).sum() > total // 4
    # the caller copies the messages sent uncompressed into their slots (device to device)
    for s in range(n_streams):
        at = 0
        for k in range(n_msgs):
            i = s * n_msgs + k
            if written[i] == 0:
                hip.copy(d_blocks + i * MAX, d_in + s * stride + at, lens[i])
            at += lens[i]
    in_bytes = np.where(written > 0, written, np.asarray(lens, dtype=np.uint32))
    d_out = hip.malloc(total * MAX)
    restored, status, ms = decompress_batch(d_blocks, n_streams, n_msgs, in_bytes, written > 0, MAX, d_out)
    out = hip.download(d_out, total * MAX)
    hip.close()
    check_batch(streams, MAX, out.tobytes(), restored, status)


TORCH_CHAIN = r"""
import sys
import numpy as np
import torch
torch.cuda.init()
root, path, max_bytes = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, root)
from tonk_amd.compress import compress_batch, decompress_batch
z = np.load(path + ".in.npz")
host, lens = z["host"], z["lens"]
n_streams, stride = host.shape
n_msgs = lens.size // n_streams
total = n_streams * n_msgs
d_in = torch.from_numpy(host).cuda()
d_blocks = torch.zeros(total * max_bytes + 32, dtype=torch.uint8, device="cuda")
written, _ = compress_batch(d_in.data_ptr(), stride, n_streams, n_msgs, lens, max_bytes, d_blocks.data_ptr())
flat = d_in.reshape(-1)
for s in range(n_streams):  # the messages sent uncompressed go into their slots, device to device
    at = 0
    for k in range(n_msgs):
        i, n = s * n_msgs + k, int(lens[s * n_msgs + k])
        if written[i] == 0:
            d_blocks[i * max_bytes:i * max_bytes + n] = flat[s * stride + at:s * stride + at + n]
        at += n
torch.cuda.synchronize()
in_bytes = np.where(written > 0, written, lens).astype(np.uint32)
d_out = torch.zeros(total * max_bytes, dtype=torch.uint8, device="cuda")
restored, status, ms = decompress_batch(d_blocks.data_ptr(), n_streams, n_msgs, in_bytes, written > 0, max_bytes,
                                        d_out.data_ptr())
torch.cuda.synchronize()
np.savez(path + ".out.npz", out=d_out.cpu().numpy(), restored=restored, status=status, written=written)
print("chain ok")
"""


@pytest.mark.gpu
def test_gpu_chain_on_torch_tensors(tmp_path):
    """compress_batch then decompress_batch on torch tensors (data_ptr()), as README, INTEGRATION
    and tools/decompress_time.py use them, in a process where torch initialises the GPU first."""
    import sys
    n_streams, n_msgs = 8, 60
    streams = [mixed_messages(n_msgs, 200 + s) for s in range(n_streams)]
    stride = max(sum(map(len, s)) for s in streams) + 64
    host = np.zeros((n_streams, stride), dtype=np.uint8)
    lens = []
    for s, ms in enumerate(streams):
        blob = b"".join(ms)
        host[s, :len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        lens += [len(m) for m in ms]
    path = str(tmp_path / "chain")
    np.savez(path + ".in.npz", host=host, lens=np.asarray(lens, dtype=np.uint32))
    r = subprocess.run([sys.executable, "-c", TORCH_CHAIN, ROOT, path, str(MAX)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "chain ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(path + ".out.npz")
    assert (z["written"] > 0).sum() > n_streams * n_msgs // 4
    check_batch(streams, MAX, z["out"].tobytes(), z["restored"], z["status"])


@pytest.mark.gpu
def test_gpu_decompressor_failure_contract():
    """dest_cap below the restored size: -4 and nothing written; a rejected block: negative with
    the reader's reason; after either the decompressor stays failed."""
    from tonk_amd.compress import MessageDecompressor, _lib
    L = ref_lib()
    msgs = mixed_messages(40, 5)
    comp = RefCompressor(L, MAX)
    blocks = [comp.compress(m) for m in msgs]
    first = next(k for k, b in enumerate(blocks) if b and len(msgs[k]) > 8)
    later = next(k for k in range(first + 1, len(blocks)) if blocks[k])

    def fed(dec, upto):
        for k in range(upto):
            if blocks[k]:
                assert dec.decompress(blocks[k]) == msgs[k]
            else:
                dec.insert_uncompressed(msgs[k])

    # one byte short
    dec = MessageDecompressor(MAX)
    fed(dec, first)
    cap = len(msgs[first]) - 1
    dest = ctypes.create_string_buffer(b"\xa5" * MAX, MAX)
    got = ctypes.c_uint(77)
    rc = _lib().tamd_decompressor_decompress(dec._h, blocks[first], len(blocks[first]), dest, cap, ctypes.byref(got))
    assert rc == -4 and got.value == 0
    assert dest.raw == b"\xa5" * MAX
    with pytest.raises(RuntimeError):
        dec.decompress(blocks[first])
    dec.close()
    # a block cut to two bytes (shorter than any block: TAMD_UNLZ_E_SHORT), then a good one
    dec = MessageDecompressor(MAX)
    fed(dec, first)
    rc = _lib().tamd_decompressor_decompress(dec._h, blocks[first][:2], 2, dest, MAX, ctypes.byref(got))
    assert rc == -17 and got.value == 0
    assert dest.raw == b"\xa5" * MAX
    with pytest.raises(RuntimeError):
        dec.decompress(blocks[first])
    with pytest.raises(RuntimeError):
        dec.decompress(blocks[later])
    dec.close()


@pytest.mark.gpu
def test_gpu_decompressor_flushes_queued_messages():
    """More uncompressed messages between two blocks than the queue holds (four ring sizes): they
    are flushed without a block, and the next block's matches find them in the history."""
    from tonk_amd.compress import MessageDecompressor
    L = ref_lib()
    rng = np.random.default_rng(11)
    comp, dec = RefCompressor(L, MAX), MessageDecompressor(MAX)
    noise = [rng.integers(0, 256, MAX, dtype=np.uint8).tobytes() for _ in range(80)]  # 104,000 bytes
    for m in noise:
        assert comp.compress(m) == b""  # (random bytes: sent as they are)
        dec.insert_uncompressed(m)
    again = noise[-2][100:700] + noise[-1][:600]  # repeats of the last two: matches into the history
    blk = comp.compress(again)
    assert blk and len(blk) < 100
    assert dec.decompress(blk) == again
    dec.close()


@pytest.mark.gpu
def test_gpu_repeat_rewrites_and_hand_made_blocks(stream_file, tmp_path):
    """Streams "first k+1 messages, then the block rewritten to Repeat modes", and the hand-made
    RLE / raw blocks: the device restores what the reference decompressor restores."""
    from tonk_amd.compress import decompress_batch_host
    L = ref_lib()
    exe = unlz_check()
    path = str(tmp_path / "rewrites.bin")
    r = subprocess.run([exe, "check", stream_file, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    cases = read_cases(path, False)
    assert len(cases) > 4
    for max_bytes, msgs in cases:
        rdec = RefDecompressor(L, max_bytes)
        want = []
        for isb, data, _, _ in msgs:
            want.append(rdec.feed(data if isb else b"", data))
        slots = np.zeros((len(msgs), max_bytes), dtype=np.uint8)
        for k, (_, data, _, _) in enumerate(msgs):
            slots[k, :len(data)] = np.frombuffer(data, dtype=np.uint8)
        out, restored, status, _ = decompress_batch_host(slots.tobytes(), 1, len(msgs), [len(m[1]) for m in msgs],
                                                         [int(m[0]) for m in msgs], max_bytes)
        out = np.frombuffer(out, dtype=np.uint8).reshape(-1, max_bytes)
        for k, w in enumerate(want):
            assert status[k] == 0 and restored[k] == len(w), (k, status[k])
            assert out[k, :len(w)].tobytes() == w, k


@pytest.mark.gpu
def test_gpu_rejects_malformed_blocks_like_the_host_walk(mutant_cases):
    """64 streams, each a valid prefix, one block of the malformed corpus and one more message:
    per-message status and restored bytes equal the host walk's, accepted outputs are equal,
    later messages of a failed stream are untouched, and the canaries around every output slot
    and around the ring allocation are intact."""
    from tonk_amd.compress import decompress_batch
    hip = Hip()
    r, path = mutant_cases
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    cases = read_cases(path, True)
    assert len(cases) == 64
    for max_bytes in sorted({c[0] for c in cases}):
        group = [c[1] for c in cases if c[0] == max_bytes]
        n_msgs = max(len(g) for g in group)
        # shorter streams are padded at the end, behind everything the host walk saw, with
        # uncompressed messages: restored as they are, or not decoded when the stream has failed
        def padded(g):
            dead = any(st != 0 for _, _, st, _ in g)
            pad = (False, b"p" * 16, STATUS_FAILED, b"") if dead else (False, b"p" * 16, 0, b"p" * 16)
            return g + [pad] * (n_msgs - len(g))
        group = [padded(g) for g in group]
        n_streams, total = len(group), len(group) * n_msgs
        slots = np.zeros((total, max_bytes), dtype=np.uint8)
        in_bytes, is_block = [], []
        for s, g in enumerate(group):
            for k, (isb, data, _, _) in enumerate(g):
                slots[s * n_msgs + k, :len(data)] = np.frombuffer(data, dtype=np.uint8)
                in_bytes.append(len(data))
                is_block.append(int(isb))
        d_in = hip.malloc(total * max_bytes + 32)
        hip.upload(d_in, slots.reshape(-1))
        # output slots with 64-byte canaries: the batch's stride is the slot size, so the canaries
        # sit before the first and after the last slot, and every slot's unused tail is one too
        d_out = hip.malloc(64 + total * max_bytes + 64, fill=0xA5)
        restored, status, _ = decompress_batch(d_in, n_streams, n_msgs, in_bytes, is_block, max_bytes, d_out + 64)
        out = hip.download(d_out, 64 + total * max_bytes + 64)
        assert (out[:64] == 0xA5).all() and (out[-64:] == 0xA5).all()
        body = out[64:-64].reshape(total, max_bytes)
        for s, g in enumerate(group):
            for k, (_, _, want_status, want) in enumerate(g):
                i = s * n_msgs + k
                assert status[i] == want_status and restored[i] == len(want), (s, k, status[i], want_status)
                if want_status == 0:
                    assert body[i, :len(want)].tobytes() == want, (s, k)
                    assert (body[i, len(want):] == 0xA5).all(), (s, k)
                elif want_status == STATUS_FAILED:
                    assert (body[i] == 0xA5).all(), (s, k)  # a later message of a failed stream
        assert any(st == STATUS_FAILED for st in status) and any(st not in (0, STATUS_FAILED) for st in status)
    hip.close()


@pytest.mark.gpu
def test_gpu_decompressor_concurrent_callers():
    """8 threads x 150 messages, each thread with its own compressor-decompressor pair calling
    the synchronous per-message API at the same time."""
    from tonk_amd.compress import MessageCompressor, MessageDecompressor
    n_threads, n_msgs = 8, 150
    streams = [mixed_messages(n_msgs, 300 + t) for t in range(n_threads)]
    errors = []

    def worker(t):
        try:
            comp, dec = MessageCompressor(MAX), MessageDecompressor(MAX)
            for k, m in enumerate(streams[t]):
                blk = comp.compress(m)
                if blk:
                    if dec.decompress(blk) != m:
                        errors.append((t, k))
                        return
                else:
                    dec.insert_uncompressed(m)
            comp.close()
            dec.close()
        except Exception as e:  # (surfaced below)
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(n_threads)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not any(x.is_alive() for x in th), "a call did not return"
    assert not errors, errors
