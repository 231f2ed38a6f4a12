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
from lz_streams import (MAX, RING_EDGE_KS, Hip, RefCompressor, RefDecompressor, batch_cases, checked_record,
                        edge_case_messages, length_sweep, lz_blocks_check, lz_blocks_exe, mixed_messages, pack_streams,
                        pad_streams, read_cases, ref_lib, rep_offsets, ring_edge, ring_positions, run_threads, skewed,
                        tonk_unit_messages, word_shuffle, write_cases, write_streams)


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


# ---- the checker of compressor output (tests/native/lz_blocks.cpp) on the host writer's blocks

def _host_cases(tmp_path, streams, *opts, name="host"):
    """The host compressor of lz_host.h (raw literals; `opts` as lz_blocks takes them) over
    [(max, messages)]: the case file's path."""
    src, out = str(tmp_path / f"{name}_streams.bin"), str(tmp_path / f"{name}_cases.bin")
    write_streams(src, streams)
    subprocess.run([lz_blocks_exe(), "host", src, out, *opts], check=True, timeout=120)
    return out


def _cases_of(path):
    return [(mx, [(restored, data) if isb else (data, b"") for isb, data, _, restored in msgs])
            for mx, msgs in read_cases(path, True)]


def test_checker_accepts_host_writer_blocks(tmp_path):
    """Blocks of lz_host_block with raw literals over every stream of test_decompress.cpu_streams():
    the checker accepts every one, in the plain build and under the address and undefined-behaviour
    sanitizers (no report, the same record), and the host writer's record shows predefined, RLE
    and fitted tables for each of LL, ML and OF, so the GPU tests' reach assertions are attainable."""
    from test_decompress import cpu_streams
    path = _host_cases(tmp_path, cpu_streams())
    rc, recs, total, text = lz_blocks_check(path)
    assert rc == 0 and total["ok"] and all(r["ok"] for r in recs) and len(recs) == 10, text
    assert total["blocks_small"] > 500 and total["blocks_big"] > 500 and total["as_is_small"] and total["as_is_big"]
    for t in ("ll_modes", "ml_modes", "of_modes"):
        assert all(total[t][m] > 0 for m in ("predefined", "rle", "fitted")), (t, total[t])
    assert total["seq_header_1"] and total["seq_header_2"] and total["overlap"] and total["ext_match"] and total["ext_cross"]
    san = subprocess.run([lz_blocks_exe("lz_blocks_san"), "check", path], capture_output=True, text=True, timeout=600)
    assert san.returncode == 0, san.stdout[-2000:] + san.stderr[-4000:]
    assert "ERROR" not in san.stderr and "runtime error" not in san.stderr, san.stderr[-4000:]
    plain = subprocess.run([lz_blocks_exe(), "check", path], capture_output=True, text=True, timeout=600)
    assert plain.stdout == san.stdout


def _window_mutant_stream():
    """A stream with a ring restart whose last message repeats the previous segment from one byte
    before its window start (lz.h RingTrack): with the window moved back by one the host parse
    takes that byte as the first external match's source.  The rest of the history is zeros, so
    that the parse's hash table still holds the position."""
    rng = np.random.default_rng(1)
    msgs = [bytes(1300) for _ in range(19)]
    msgs[1] = rng.integers(0, 256, 1300, dtype=np.uint8).tobytes()
    pos, win = ring_positions(1300, [1300] * 19 + [600])[-1]
    assert pos == 19 * 1300 and 1300 < win < 2600  # (after the restart; the window starts inside the random message)
    msgs.append(b"".join(msgs)[win - 1:win - 1 + 600])
    return (1300, msgs)


def _size_mutant_stream():
    """Short messages of 8 random bytes, their first 4..14 bytes again and 0..3 more: some blocks
    of theirs are exactly as long as the message."""
    rng = np.random.default_rng(2)
    msgs = []
    for ml in range(4, 15):
        for tail in range(4):
            a = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
            msgs.append(a + a[:ml] + rng.integers(0, 256, tail, dtype=np.uint8).tobytes())
    return (1300, msgs)


@pytest.mark.parametrize("what, opts, reason", [
    ("tables", ["fitted=0"], "tables differ from tamd_seq_choose"),
    ("maximal", ["len_cap=20"], "match not maximal"),
    ("minmatch", ["minmatch=3", "len_cap=3"], "match below 4"),  # (the host parse finds 3-byte matches only when cut)
    ("huffman", ["huffman=1"], "literals not raw"),
    ("flip", ["flip=1"], None),
    ("size", ["slack=1"], "block above min(len - 1, max)"),
    ("window", ["win_back=1"], "match source before the window start"),
])
def test_checker_rejects_one_thing_wrong(tmp_path, what, opts, reason):
    """The checker is no rubber stamp: the host writer with one thing wrong each time (predefined
    tables where tamd_seq_choose picks others, matches cut short, a 3-byte match, Huffman literals,
    one bit of a fitted table's description flipped, a block as long as its message, a match
    source one byte before the window start).  Every stream written wrong is rejected with the
    reason that belongs to it, and the same streams written right are accepted in the same run."""
    from test_decompress import cpu_streams
    if what == "huffman":
        streams = [(1300, skewed(120, 9, 1300))]
    elif what == "size":
        streams = [_size_mutant_stream()]
    elif what == "window":
        streams = [_window_mutant_stream()]
    else:
        streams = cpu_streams()[1:4]
    right = _cases_of(_host_cases(tmp_path, streams, name="right"))
    wrong = _cases_of(_host_cases(tmp_path, streams, *opts, name="wrong"))
    assert right != wrong
    path = str(tmp_path / "both.bin")
    write_cases(path, right + wrong)
    rc, recs, total, text = lz_blocks_check(path)
    assert rc == 1 and len(recs) == 2 * len(streams), text
    assert all(r["ok"] and r["blocks_small"] + r["blocks_big"] > 0 for r in recs[:len(streams)]), text
    for r in recs[len(streams):]:
        assert not r["ok"] and r["failed_message"] >= 0, r
        if reason is None:  # (a flipped bit: whichever check meets it first)
            assert r["reason"] in ("block rejected by the reader", "block does not restore the message",
                                   "tables differ from tamd_seq_choose", "match not maximal",
                                   "match source before the window start", "match below 4",
                                   "lengths do not sum to the message", "match source before the stream"), r
        else:
            assert r["reason"] == reason, r


# --------------------------------------------------------------------------------------- GPU

# The GPU compressor's total output over the reference compressor's (zstd level 1) on the same
# stream, measured on an MI355X; the size tests allow this quotient plus 0.05 (the output is
# deterministic: the margin is room for deliberate changes of the parse).
GPU_OVER_REFERENCE = {"mixed_5": 0.9559, "mixed_6": 0.9686, "batch_16x120": 0.9734}


def lz_max_message(tmp_path):
    """TAMD_LZ_MAX_MESSAGE as the checker prints it: the largest message compressed in LDS."""
    return checked_record(tmp_path, [(MAX, [(b"12345678", b"")])], name="constant.bin")["lz_max_message"]


@pytest.mark.gpu
def test_gpu_compressor_tonk_unit_stream(tmp_path):
    """TonkUnitTest.cpp TestCompression through the GPU compressor: every message restored, and
    the repeated second half compresses wherever the decompressor still holds its source; every
    block accepted by the checker (tests/native/lz_blocks.cpp)."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    msgs = tonk_unit_messages()
    comp, dec = MessageCompressor(MAX), RefDecompressor(L)
    rcomp = RefCompressor(L)
    ours = theirs = 0
    cases = []
    for m in msgs:
        blk = comp.compress(m)
        cases.append((m, blk))
        assert len(blk) < len(m)
        ours += bool(blk)
        assert dec.feed(blk, m) == m
        theirs += bool(rcomp.compress(m))
    print(f"compressed messages: gpu {ours}, reference zstd-1 {theirs}")
    assert ours >= 20
    rec = checked_record(tmp_path, [(MAX, cases)])
    assert rec["blocks_small"] == ours and rec["ml_over_16"] >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [5, 6])
def test_gpu_compressor_mixed_stream(seed, tmp_path):
    """A long mixed stream (several ring wraps, external-dictionary matches: both asserted from
    the checker's record) through the GPU compressor, restored by the reference decompressor and
    accepted block by block by the checker; the total size is bounded by the reference
    compressor's (zstd level 1) on the same stream times the quotient measured on an MI355X
    (GPU_OVER_REFERENCE: 0.9559 for seed 5, 0.9686 for seed 6) plus 0.05."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    msgs = mixed_messages(400, seed)
    comp, dec, rcomp = MessageCompressor(MAX), RefDecompressor(L), RefCompressor(L)
    out_gpu = out_ref = inp = 0
    cases = []
    for m in msgs:
        blk = comp.compress(m)
        cases.append((m, blk))
        assert dec.feed(blk, m) == m
        out_gpu += len(blk) if blk else len(m)
        r = rcomp.compress(m)
        out_ref += len(r) if r else len(m)
        inp += len(m)
    print(f"bytes in {inp}: gpu {out_gpu} ({inp / out_gpu:.2f}x), zstd-1 {out_ref} ({inp / out_ref:.2f}x), "
          f"gpu / zstd-1 = {out_gpu / out_ref:.4f}")
    assert out_gpu < 0.75 * inp
    assert out_gpu <= (GPU_OVER_REFERENCE[f"mixed_{seed}"] + 0.05) * out_ref
    rec = checked_record(tmp_path, [(MAX, cases)])
    assert rec["ring_restarts"] >= 5 and rec["ext_match"] > 0 and rec["ext_cross"] > 0 and rec["overlap"] > 0
    assert rec["in_bytes"] == inp and rec["out_bytes"] == out_gpu


@pytest.mark.gpu
def test_gpu_compress_batch_streams(tmp_path):
    """The device-resident batch: 16 streams x 120 messages in one launch; every stream restored
    in order by its own reference decompressor and accepted by the checker; the total size bounded
    by the reference compressor's on the same streams (GPU_OVER_REFERENCE: measured 0.9734)."""
    from tonk_amd.compress import compress_batch_host
    L = ref_lib()
    n_streams, n_msgs = 16, 120
    streams = [mixed_messages(n_msgs, 100 + s) for s in range(n_streams)]
    host, stride, lens = pack_streams(streams)
    raw, written, ms = compress_batch_host(host.tobytes(), stride, n_streams, n_msgs, lens, MAX, msgs_per_job=8)
    out_h = np.frombuffer(raw, dtype=np.uint8)
    total_in = total_out = total_ref = 0
    for s, msgs in enumerate(streams):
        dec, rcomp = RefDecompressor(L), RefCompressor(L)
        for k, m in enumerate(msgs):
            total_ref += len(rcomp.compress(m)) or len(m)
            i = s * n_msgs + k
            w = written[i]
            assert w < len(m)
            blk = out_h[i * MAX:i * MAX + w].tobytes() if w else b""
            assert dec.feed(blk, m) == m, (s, k)
            total_in += len(m)
            total_out += w if w else len(m)
    print(f"batch: {total_in} -> {total_out} bytes, kernel {ms:.3f} ms; zstd-1 {total_ref}, "
          f"gpu / zstd-1 = {total_out / total_ref:.4f}")
    assert total_out < 0.8 * total_in
    assert total_out <= (GPU_OVER_REFERENCE["batch_16x120"] + 0.05) * total_ref
    rec = checked_record(tmp_path, batch_cases(streams, MAX, raw, written))
    assert rec["out_bytes"] == total_out and rec["ext_match"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("max_bytes", [1300, 4000, 24000])
def test_gpu_compressor_edge_cases(max_bytes, tmp_path):
    """Tiny messages (below the kernel's 8-byte floor: sent as is), runs of one byte (matches that
    overlap their own output, distance 1), messages of exactly max bytes, messages above
    TAMD_LZ_MAX_MESSAGE (the constant the checker prints: compressed through global scratch
    instead of LDS) up to the 24,000-byte history, and enough of them to restart the ring many
    times; every one restored by the reference decompressor and accepted by the checker, whose
    record shows the overlapping matches, the distance 1 and the restarts."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    msgs = edge_case_messages(max_bytes)
    comp, dec = MessageCompressor(max_bytes), RefDecompressor(L, max_bytes)
    n_comp = 0
    lz_max = lz_max_message(tmp_path)
    cases = []
    for m in msgs:
        blk = comp.compress(m)
        cases.append((m, blk))
        assert len(blk) < len(m) or not blk
        if len(m) < 8:
            assert blk == b""
        n_comp += bool(blk)
        if len(m) > lz_max and len(set(m)) <= 3:
            assert blk, len(m)  # (repetitive text and one-byte runs compress at any size)
        assert dec.feed(blk, m) == m
    assert n_comp > 100
    rec = checked_record(tmp_path, [(max_bytes, cases)])
    assert rec["overlap"] > 0 and rec["dist1"] > 0 and rec["ring_restarts"] > 10
    assert rec["blocks_small"] + rec["blocks_big"] == n_comp
    if max_bytes > lz_max:
        assert rec["blocks_big"] > 100


@pytest.mark.gpu
@pytest.mark.parametrize("per_job", [4, 0])
def test_gpu_compress_batch_large_messages(per_job, tmp_path):
    """The batch API with messages of 64 B .. 24,000 B (the history size) mixed in one launch:
    the large ones (above TAMD_LZ_MAX_MESSAGE, the constant the checker prints) go through global
    scratch, jobs longer than 64 KB move their hash table's base (with 4 messages per job: the
    record shows sequences of messages past 64 KB); per_job 0: the library's job size (one round
    of jobs over the wave slots: here one message per job); every stream restored by the reference
    and accepted by the checker."""
    from tonk_amd.compress import compress_batch_host
    L = ref_lib()
    max_bytes, n_streams, n_msgs = 24000, 4, 24
    lz_max = lz_max_message(tmp_path)
    rng = np.random.default_rng(11)
    text = b"".join(rng.choice([b"siamese ", b"tonk ", b"window ", b"lane "], 6000))
    streams = []
    for s in range(n_streams):
        ms = []
        for k in range(n_msgs):
            n = int(rng.integers(64, lz_max + 1)) if k % 3 else int(rng.integers(lz_max + 1, max_bytes + 1))
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
            big += bool(w) and len(m) > lz_max
            blk = out_h[i * max_bytes:i * max_bytes + w].tobytes() if w else b""
            assert dec.feed(blk, m) == m, (s, k)
    assert big >= n_streams * n_msgs // 6
    rec = checked_record(tmp_path, batch_cases(streams, max_bytes, raw, written))
    assert rec["blocks_big"] == big and rec["msg_pos_max"] > 65535 and rec["sequences_past_64k"] > 0


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


def _batch(streams, max_bytes, per_job):
    """compress_batch_host over streams of equally many messages: (raw output, written)."""
    from tonk_amd.compress import compress_batch_host
    host, stride, lens = pack_streams(streams)
    raw, written, _ = compress_batch_host(host.tobytes(), stride, len(streams), len(streams[0]), lens, max_bytes,
                                          msgs_per_job=per_job)
    return raw, written


def _roundtrip(L, max_bytes, cases):
    """The reference decompressor beside the checker: every stream restored in order."""
    for (_, row) in cases:
        dec = RefDecompressor(L, max_bytes)
        for m, blk in row:
            assert dec.feed(blk, m) == m


@pytest.mark.gpu
def test_gpu_compressor_skewed_and_strided_streams(tmp_path):
    """Two generators the GPU compressor had never been given: skewed literals (the host writer
    would code them with Huffman; the kernel's literals stay raw) and strided records (the
    repeat-offset cases: the kernel writes every offset anew).  Per-message API, restored by the
    reference and accepted by the checker."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    cases = []
    for msgs in (skewed(120, 9, 1300), rep_offsets(60, 3)):
        comp = MessageCompressor(MAX)
        cases.append((MAX, [(m, comp.compress(m)) for m in msgs]))
        comp.close()
    _roundtrip(L, MAX, cases)
    rec = checked_record(tmp_path, cases)
    print({k: rec[k] for k in ("blocks_small", "as_is_small", "sequences")})
    assert rec["blocks_small"] >= 50 and rec["sequences"] > 300


@pytest.mark.gpu
@pytest.mark.parametrize("per_job", [1, 4, 0])
@pytest.mark.parametrize("max_bytes", [1300, 4100, 24000])
def test_gpu_compress_length_sweep(max_bytes, per_job, tmp_path):
    """lz_streams.length_sweep through the batch: lengths at the kernel's floor, minimum match,
    probe, lane groups, probe batch, chunk, both sides of TAMD_LZ_MAX_MESSAGE, the literals
    headers' widths and the 14-bit length codes, with 1 and 4 messages per job and the library's
    own job size.  The checker accepts every block, and its record shows what the ring rule lets
    each maximum reach:
      - every repeat of n >= 64 bytes whose earlier copy lies inside its window (lz.h RingTrack,
        restated in lz_streams.ring_positions) comes back as a block.  At 24,000 every message
        starts a new history segment over the one before, so no repeat of an equal length has its
        copy left: there the self-matching messages of the sweep carry the assertions;
      - a match equal to the whole message: below TAMD_LZ_MAX_MESSAGE at 1300 and 4100, above it
        at 4100 (the hash table keeps the first position's candidate: the generator sees to it);
      - a match longer than 16 + 512 (the wave's extension took more than one step);
      - 1- and 2-byte literals headers below 24,000 (there only the self-matching messages
        compress, and a match inside a message starts in its second group of 64 positions at the
        earliest, a group's positions entering the table after it is scanned: 64 literals or
        more, a 2-byte header); at 24,000 the 3-byte one (4096 literals and a match need a message
        above 4100), the match-length code of 16387 and above (50) and the literal-length code of
        16384 and above (33).
    Sizes of repeats below 64 bytes are printed, not asserted: whether they beat len - 1 depends
    on what the table replaced."""
    L = ref_lib()
    msgs = length_sweep(max_bytes)
    raw, written = _batch([msgs], max_bytes, per_job)
    cases = batch_cases([msgs], max_bytes, raw, written)
    _roundtrip(L, max_bytes, cases)
    rec = checked_record(tmp_path, cases)
    lz_max = rec["lz_max_message"]
    place = ring_positions(max_bytes, [len(m) for m in msgs])
    reachable = 0
    for i in range(1, len(msgs)):
        n = len(msgs[i])
        is_repeat = len(msgs[i - 1]) == n and sum(a != b for a, b in zip(msgs[i], msgs[i - 1])) <= 3
        if not is_repeat:
            continue
        pos, win = place[i]
        if n < 64:
            print(f"repeat of {n} bytes: written {written[i]}")
        elif win <= pos - n:
            reachable += 1
            assert written[i] > 0, (i, n)
    print(f"max {max_bytes} per_job {per_job}: repeats inside their window {reachable}; "
          + ", ".join(f"{k} {rec[k]}" for k in ("blocks_small", "blocks_big", "ml_whole_small", "ml_whole_big", "ml_over_528",
                                              "lit_header_1", "lit_header_2", "lit_header_3", "ml_code_max", "ll_code_max")))
    assert rec["ml_over_528"] > 0 and rec["lit_header_2"] > 0 and rec["overlap"] > 0
    if max_bytes < 24000:
        assert rec["lit_header_1"] > 0
        assert reachable >= 3 * sum(1 for n in set(map(len, msgs)) if n >= 64) - 6
        assert rec["ml_whole_small"] > 0
    if max_bytes == 4100:
        assert rec["ml_whole_big"] > 0
    if max_bytes > lz_max:
        assert rec["blocks_big"] > 0
    if max_bytes == 24000:
        assert rec["lit_header_3"] > 0 and rec["ml_code_max"] >= 50 and rec["ll_code_max"] >= 33


@pytest.mark.gpu
def test_gpu_compress_word_shuffle(tmp_path):
    """lz_streams.word_shuffle through the batch, a stream per configuration: k words give k
    sequences, so the sequence counts sit at 1, around 64 and 128 (the 64-sequence store groups
    and their tail, lz.hip lz_message: `(nseq & 63u) == 0` and `lane < (nseq & 63u)`), and, with
    192 words of 8 bytes and no gap, at the most a 1536-byte message yields: candidates are
    keyed by 8 bytes (lz.hip lz_hash of msg_dword), so matches effectively begin with 8 equal
    bytes and LZ_MAX_SEQS (384) is never approached.  The record shows each of predefined, RLE
    and fitted on each of LL, ML and OF (RLE on all three: equal words and gaps far enough from
    their source that the offsets share a power-of-two band), nseq mod 64 of 0, 1 and 63 with
    nseq below and above 64, and sequence-count headers of both widths."""
    L = ref_lib()
    max_bytes = 4100
    streams = [word_shuffle(k, 12, 4, seed=k) for k in (1, 2, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130)]
    streams += [word_shuffle(192, 8, 0, seed=192)]
    streams += [word_shuffle(k, 12, 4, seed=1000 + k, jitter=2) for k in (3, 4, 5, 40, 100)]   # several length codes
    streams += [word_shuffle(k, 8, 4, seed=2000 + k, filler=2) for k in (10, 20)]               # one code per table
    streams = pad_streams(streams)
    raw, written = _batch(streams, max_bytes, 0)
    cases = batch_cases(streams, max_bytes, raw, written)
    _roundtrip(L, max_bytes, cases)
    rec = checked_record(tmp_path, cases)
    print({k: rec[k] for k in ("ll_modes", "ml_modes", "of_modes", "nseq_seen", "seq_header_1", "seq_header_2")})
    for t in ("ll_modes", "ml_modes", "of_modes"):
        assert all(rec[t][m] > 0 for m in ("predefined", "rle", "fitted")), (t, rec[t])
    seen = rec["nseq_seen"]
    assert {0, 1, 63} <= {v % 64 for v in seen}, seen
    assert any(1 < v < 64 for v in seen) and any(v > 64 for v in seen), seen
    assert rec["seq_header_1"] > 0 and rec["seq_header_2"] > 0 and rec["nseq_max"] >= 128


@pytest.mark.gpu
def test_gpu_compress_one_job_past_64k(tmp_path):
    """4 streams x 120 mixed messages of up to 1300 bytes, each stream one job: the job runs past
    64 KB with every message in LDS, so the hash table's base moves (lz.hip lz_rebase, from
    lz_message's chunk loop) in the LDS path too.  The record's highest message position is above
    65535 and the messages past that point still carry sequences."""
    L = ref_lib()
    streams = [mixed_messages(120, 500 + s) for s in range(4)]
    raw, written = _batch(streams, MAX, 120)
    cases = batch_cases(streams, MAX, raw, written)
    _roundtrip(L, MAX, cases)
    rec = checked_record(tmp_path, cases)
    assert rec["blocks_big"] == 0 and rec["msg_pos_max"] > 65535 and rec["sequences_past_64k"] > 100, rec
    assert rec["src_pos_max"] > 65535


@pytest.mark.gpu
def test_gpu_compressor_ring_edge(tmp_path):
    """lz_streams.ring_edge through the per-message API: the running byte count lands 1 .. 65 bytes
    before the end of the 64 KB device ring, sixteen times over, and the next messages repeat the
    bytes on both sides of it, so probes, extension loads and 8-byte keys straddle the ring's end
    and its 64-byte mirror.  The checker accepts every block (a stale mirror byte would cut a match
    short of the linear stream's: not maximal, or restore another byte); the record shows matches
    whose source and whose target cross a multiple of 65536, and, the history restarting many
    times at 1300, external matches and ones that cross into the current segment."""
    from tonk_amd.compress import MessageCompressor
    L = ref_lib()
    msgs = ring_edge()
    comp = MessageCompressor(MAX)
    cases = [(MAX, [(m, comp.compress(m)) for m in msgs])]
    comp.close()
    _roundtrip(L, MAX, cases)
    rec = checked_record(tmp_path, cases)
    print({k: rec[k] for k in ("src_cross_64k", "dst_cross_64k", "ext_match", "ext_cross", "ring_restarts", "msg_pos_max")})
    n_edges = 2 * len(RING_EDGE_KS)
    assert rec["msg_pos_max"] > n_edges * 65536
    # (a target crosses only when the match starts at the message's first bytes, which the table's
    # replacement may deny now and then: half of the sixteen edges at least)
    assert rec["dst_cross_64k"] >= n_edges // 2 and rec["src_cross_64k"] >= n_edges // 2, rec
    assert rec["ext_match"] > 0 and rec["ext_cross"] > 0 and rec["ring_restarts"] > 30


@pytest.mark.gpu
@pytest.mark.parametrize("max_bytes", [1300, 24000])
def test_gpu_compress_batch_canaries(max_bytes):
    """compress_batch on device memory with 64 bytes of 0xA5 in front of and behind the output and
    the output itself filled with 0xA5: the guards stay, every slot is 0xA5 from written[i] to its
    end (a slot with written[i] = 0 is untouched), and the input buffer is unchanged."""
    from tonk_amd.compress import compress_batch
    streams = [mixed_messages(24, 700 + s, max_bytes) for s in range(4)]
    host, stride, lens = pack_streams(streams)
    total = len(lens)
    hip = Hip()
    try:
        d_in = hip.malloc(host.size)
        hip.upload(d_in, host)
        d_out = hip.malloc(64 + total * max_bytes + 64, fill=0xA5)
        written, _ = compress_batch(d_in, stride, len(streams), len(streams[0]), lens, max_bytes, d_out + 64)
        out = hip.download(d_out, 64 + total * max_bytes + 64)
        back = hip.download(d_in, host.size)
    finally:
        hip.close()
    assert (back == host.reshape(-1)).all()
    assert (out[:64] == 0xA5).all() and (out[-64:] == 0xA5).all()
    slots = out[64:-64].reshape(total, max_bytes)
    assert 0 < (written == 0).sum() < total
    for i in range(total):
        assert written[i] < lens[i]
        assert (slots[i, written[i]:] == 0xA5).all(), i
    used = np.arange(max_bytes)[None, :] < written[:, None]
    assert (slots[used] != 0xA5).any()


@pytest.mark.gpu
def test_gpu_compress_batch_is_deterministic():
    """The same batch twice in one process: written and every output byte are equal (lanes of one
    store that share a hash bucket leave one of theirs in a fixed order, lz.hip lz_insert)."""
    streams = [mixed_messages(120, 100 + s) for s in range(16)]
    raw1, written1 = _batch(streams, MAX, 8)
    raw2, written2 = _batch(streams, MAX, 8)
    assert written1 == written2 and sum(written1) > 0
    for i, w in enumerate(written1):  # (past written[i] a slot holds whatever the allocation held)
        assert raw1[i * MAX:i * MAX + w] == raw2[i * MAX:i * MAX + w], i
