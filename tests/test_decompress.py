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
import subprocess

import numpy as np
import pytest

from conftest import NATIVE, ROOT, _make
from lz_streams import (MAX, Hip, RefCompressor, RefDecompressor, check_batch, edge_case_messages, mixed_messages,
                        pack_streams, read_cases, ref_lib, ref_slots, rep_offsets, run_threads, skewed, tonk_unit_messages,
                        write_streams)

STATUS_FAILED = -13  # TAMD_UNLZ_E_FAILED (tonk_amd/csrc/unlz.h)


def cpu_streams():
    """(max, messages) of every stream the walk is checked on."""
    out = [(1300, tonk_unit_messages()), (1300, mixed_messages(300, 5)), (4000, mixed_messages(300, 5, 4000)),
           (24000, mixed_messages(48, 5, 24000)), (1300, skewed(120, 9, 1300)), (8000, skewed(40, 9, 8000)),
           (1300, rep_offsets(60, 3))]
    out += [(m, edge_case_messages(m)) for m in (1300, 4000, 24000)]
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


def test_ring_rule_of_compressor_and_decoder_agree():
    """The history-ring rule in its two forms, the compressor's linear positions (lz.h RingTrack)
    and the decoder's ring offset and dictionary length (unlz.h tamd_unlz_place), stepped side by
    side over 10 maximum sizes x 200 seeded streams x 400 lengths: every position is the running
    byte count, every message fits the ring, and the compressor's window starts exactly where the
    decoder's history does.  Restarts and partly overwritten dictionaries both occurred."""
    exe = unlz_check()
    r = subprocess.run([exe, "ring"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    counts = [int(w.rstrip(",")) for w in r.stdout.splitlines()[0].split() if w.rstrip(",").isdigit()]
    assert len(counts) == 3 and counts[0] == 10 * 200 * 400
    assert counts[1] > 0 and counts[2] > 0, counts


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
    streams = [mixed_messages(24, 5, max_bytes), mixed_messages(24, 6, max_bytes),
               skewed(24, 9, max_bytes), skewed(24, 10, max_bytes)]
    slots, in_bytes, is_block = ref_slots(L, streams, max_bytes)
    types = {int(slots[i, 0]) & 3 for i in range(len(in_bytes)) if is_block[i]}
    assert {2, 3} <= types, types  # Compressed and Treeless literals are in the input
    out, restored, status, _ = decompress_batch_host(slots.tobytes(), 4, 24, in_bytes, is_block, max_bytes)
    check_batch(streams, max_bytes, out, restored, status)


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
    host, stride, lens = pack_streams(streams)
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
    host, stride, lens = pack_streams(streams)
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

    def worker(t, errors):
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

    errors = run_threads(n_threads, worker)
    assert not errors, errors


@pytest.mark.gpu
def test_gpu_recycled_device_memory():
    """The device memory of a closed compressor and decompressor goes to the next ones, stale
    bytes included (lz_host.h DevicePool); at 24,000 the messages go through the scratch path.
    First generation: a stream through a compressor-decompressor pair, the reference decompressor
    beside it; both closed.  Second generation: a block of the first stream whose match reaches
    into history, given as the first block to a new decompressor, fails or restores exactly what
    the reference restores from a fresh state: the old history is not visible.  That block has a
    decompressor of its own, since a rejected block leaves a decompressor failed for good and an
    accepted one would put bytes into the history that the new compressor does not have.  Then a
    different stream through a new pair: every message restored.  Once at 1300 with 40 messages
    a stream, once at 24,000 with 12."""
    L = ref_lib()
    for max_bytes, first, second in ((1300, (40, 7), (40, 8)), (24000, (12, 5), (12, 6))):
        _two_generations(L, max_bytes, first, second)


def _two_generations(L, max_bytes, first, second):
    from tonk_amd.compress import MessageCompressor, MessageDecompressor, _lib

    def generation(msgs):
        comp, dec, rdec = MessageCompressor(max_bytes), MessageDecompressor(max_bytes), RefDecompressor(L, max_bytes)
        blocks = []
        for k, m in enumerate(msgs):
            blk = comp.compress(m)
            assert rdec.feed(blk, m) == m, k
            if blk:
                assert dec.decompress(blk) == m, k
            else:
                dec.insert_uncompressed(m)
            blocks.append(blk)
        comp.close()
        dec.close()
        return blocks

    msgs = mixed_messages(first[0], first[1], max_bytes)
    blocks = generation(msgs)
    assert any(blocks)

    # what a fresh reference decompressor makes of each block alone: the first one it rejects or
    # restores differently from the message reaches into history
    def fresh_reference(blk):
        return RefDecompressor(L, max_bytes).decompress(blk)

    stale = next(k for k, b in enumerate(blocks) if k and b and fresh_reference(b) != msgs[k])
    want = fresh_reference(blocks[stale])
    dec = MessageDecompressor(max_bytes)
    dest = ctypes.create_string_buffer(max_bytes)
    got = ctypes.c_uint(0)
    rc = _lib().tamd_decompressor_decompress(dec._h, blocks[stale], len(blocks[stale]), dest, max_bytes, ctypes.byref(got))
    print(f"block {stale} of the first stream on a fresh decompressor: rc {rc}, reference "
          f"{'rejects' if want is None else 'restores %d bytes' % len(want)}")
    assert rc < 0 or (rc == 0 and want is not None and dest.raw[:got.value] == want)
    dec.close()

    blocks = generation(mixed_messages(second[0], second[1], max_bytes))
    assert any(blocks)
