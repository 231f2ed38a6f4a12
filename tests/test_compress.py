"""The compression step (Tonk's MessageCompressor, PacketCompression.h:92).

Parity here is the reference's own receive side: every block the GPU writes must be restored
byte for byte by tonk::MessageDecompressor (PacketCompression.cpp:120-216, restated over the
reference's zstd in oracle/msgcodec_ref.cpp and compiled from /root/reference into oracle/_ref),
with uncompressed messages fed to InsertUncompressed as Tonk does.  The blocks themselves differ
from zstd level 1's (raw literals, predefined FSE tables, our own parse); their sizes are
reported beside the reference compressor's.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import NATIVE, _make
from lz_streams import (MAX, RefCompressor, RefDecompressor, edge_case_messages, mixed_messages, pack_streams, ref_lib,
                        run_threads, tonk_unit_messages)


# --------------------------------------------------------------------------------------- CPU

def test_reference_msgcodec_roundtrip():
    """Pins the oracle: the reference compressor's blocks restore through the restated
    decompressor over Tonk's own unit-test stream and a long mixed stream (ring wraps)."""
    L = ref_lib()
    for msgs in (tonk_unit_messages(), mixed_messages(300, 5)):
        comp, dec = RefCompressor(L), RefDecompressor(L)
        n_comp = 0
        for m in msgs:
            blk = comp.compress(m)
            n_comp += bool(blk)
            assert dec.feed(blk, m) == m
        assert n_comp > 0


def test_block_writer_decodes_with_reference_zstd():
    """The block writer shared by the kernel (lz.h) against the reference's zstd decoder: with
    block-fitted / RLE sequence tables (tamd_seq_choose, the kernel's choice), and with the
    predefined tables only (where the table writer must also equal the packed-map writer)."""
    ref_lib()
    _make(NATIVE, "_build/lz_check")
    exe = os.path.join(NATIVE, "_build", "lz_check")
    for seed in (1, 2, 3):
        for extra in ([], ["0", "4", "0"]):
            r = subprocess.run([exe, "300", str(seed)] + extra, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
            if not extra:
                assert "fitted tables LL/ML/OF 0/0/0," not in r.stderr, r.stderr


def test_compress_abi_exports_and_no_cpu_fallback():
    import tonk_amd
    path = tonk_amd.LIB_PATH
    if not os.path.exists(path):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for sym in ("tamd_compressor_create", "tamd_compressor_compress", "tamd_compressor_destroy",
                "tamd_compress_batch", "tamd_compress_batch_host"):
        assert f" T {sym}" in out, sym
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tonk_amd.compress import MessageCompressor
    with pytest.raises(RuntimeError):
        MessageCompressor(MAX)


# --------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_gpu_compressor_tonk_unit_stream():
    """TonkUnitTest.cpp TestCompression through the GPU compressor: every message restored, and
    the repeated second half compresses wherever the decompressor still holds its source."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    msgs = tonk_unit_messages()
    comp, dec = MessageCompressor(MAX), RefDecompressor(L)
    rcomp = RefCompressor(L)
    ours = theirs = 0
    for m in msgs:
        blk = comp.compress(m)
        assert len(blk) < len(m)
        ours += bool(blk)
        assert dec.feed(blk, m) == m
        theirs += bool(rcomp.compress(m))
    print(f"compressed messages: gpu {ours}, reference zstd-1 {theirs}")
    assert ours >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [5, 6])
def test_gpu_compressor_mixed_stream(seed):
    """A long mixed stream (several ring wraps, external-dictionary matches) through the GPU
    compressor, restored by the reference decompressor; sizes beside zstd level 1."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    msgs = mixed_messages(400, seed)
    comp, dec, rcomp = MessageCompressor(MAX), RefDecompressor(L), RefCompressor(L)
    out_gpu = out_ref = inp = 0
    for m in msgs:
        blk = comp.compress(m)
        assert dec.feed(blk, m) == m
        out_gpu += len(blk) if blk else len(m)
        r = rcomp.compress(m)
        out_ref += len(r) if r else len(m)
        inp += len(m)
    print(f"bytes in {inp}: gpu {out_gpu} ({inp / out_gpu:.2f}x), zstd-1 {out_ref} ({inp / out_ref:.2f}x)")
    assert out_gpu < 0.75 * inp


@pytest.mark.gpu
def test_gpu_compress_batch_streams():
    """The device-resident batch: 16 streams x 120 messages in one launch; every stream restored
    in order by its own reference decompressor."""
    from tonk_amd.compress import compress_batch_host
    L = ref_lib()
    n_streams, n_msgs = 16, 120
    streams = [mixed_messages(n_msgs, 100 + s) for s in range(n_streams)]
    host, stride, lens = pack_streams(streams)
    raw, written, ms = compress_batch_host(host.tobytes(), stride, n_streams, n_msgs, lens, MAX, msgs_per_job=8)
    out_h = np.frombuffer(raw, dtype=np.uint8)
    total_in = total_out = 0
    for s, msgs in enumerate(streams):
        dec = RefDecompressor(L)
        for k, m in enumerate(msgs):
            i = s * n_msgs + k
            w = written[i]
            assert w < len(m)
            blk = out_h[i * MAX:i * MAX + w].tobytes() if w else b""
            assert dec.feed(blk, m) == m, (s, k)
            total_in += len(m)
            total_out += w if w else len(m)
    print(f"batch: {total_in} -> {total_out} bytes, kernel {ms:.3f} ms")
    assert total_out < 0.8 * total_in


@pytest.mark.gpu
@pytest.mark.parametrize("max_bytes", [1300, 4000, 24000])
def test_gpu_compressor_edge_cases(max_bytes):
    """Tiny messages (below the kernel's 8-byte floor: sent as is), runs of one byte (matches that
    overlap their own output, distance 1), messages of exactly max bytes, messages above 2048
    bytes (compressed through global scratch instead of LDS) up to the 24,000-byte history, and
    enough of them to restart the ring many times; every one restored by the reference
    decompressor."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    msgs = edge_case_messages(max_bytes)
    comp, dec = MessageCompressor(max_bytes), RefDecompressor(L, max_bytes)
    n_comp = 0
    for m in msgs:
        blk = comp.compress(m)
        assert len(blk) < len(m) or not blk
        if len(m) < 8:
            assert blk == b""
        n_comp += bool(blk)
        if len(m) > 2048 and len(set(m)) <= 3:
            assert blk, len(m)  # (repetitive text and one-byte runs compress at any size)
        assert dec.feed(blk, m) == m
    assert n_comp > 100


@pytest.mark.gpu
@pytest.mark.parametrize("per_job", [4, 0])
def test_gpu_compress_batch_large_messages(per_job):
    """The batch API with messages of 64 B .. 24,000 B (the history size) mixed in one launch:
    the large ones go through global scratch, jobs longer than 64 KB move their hash table's base;
    per_job 0: the library's job size (one round of jobs over the wave slots: here one message
    per job); every stream restored by the reference."""
    from tonk_amd.compress import compress_batch_host
    L = ref_lib()
    max_bytes, n_streams, n_msgs = 24000, 4, 24
    rng = np.random.default_rng(11)
    text = b"".join(rng.choice([b"siamese ", b"tonk ", b"window ", b"lane "], 6000))
    streams = []
    for s in range(n_streams):
        ms = []
        for k in range(n_msgs):
            n = int(rng.integers(64, 2049)) if k % 3 else int(rng.integers(2049, max_bytes + 1))
            if k % 4 == 3:
                ms.append(bytes(rng.integers(0, 256, n, dtype=np.uint8)))
            else:
                o = int(rng.integers(0, len(text) - n))
                ms.append(text[o:o + n])
        streams.append(ms)
    host, stride, lens = pack_streams(streams)
    raw, written, _ = compress_batch_host(host.tobytes(), stride, n_streams, n_msgs, lens, max_bytes, msgs_per_job=per_job)
    out_h = np.frombuffer(raw, dtype=np.uint8)
    big = 0
    for s, msgs in enumerate(streams):
        dec = RefDecompressor(L, max_bytes)
        for k, m in enumerate(msgs):
            i = s * n_msgs + k
            w = written[i]
            assert w < len(m)
            big += bool(w) and len(m) > 2048
            blk = out_h[i * max_bytes:i * max_bytes + w].tobytes() if w else b""
            assert dec.feed(blk, m) == m, (s, k)
    assert big >= n_streams * n_msgs // 6


@pytest.mark.gpu
def test_gpu_compressor_concurrent_callers():
    """Several threads, each with its own compressor, call the synchronous per-message API at the
    same time (Tonk's connection threads): the calls are combined into shared launches, a leader
    hands leadership on once its own message is done, and every stream is restored in order by
    its own reference decompressor."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    n_threads, n_msgs = 8, 150
    streams = [mixed_messages(n_msgs, 300 + t) for t in range(n_threads)]
    blocks = [[None] * n_msgs for _ in range(n_threads)]

    def worker(t, errors):
        comp = MessageCompressor(MAX)
        for k, m in enumerate(streams[t]):
            blocks[t][k] = comp.compress(m)

    errors = run_threads(n_threads, worker)
    assert not errors, errors
    for t in range(n_threads):
        dec = RefDecompressor(L)
        for k, m in enumerate(streams[t]):
            assert dec.feed(blocks[t][k], m) == m, (t, k)
