"""The receive side of the compression step: tonk::MessageDecompressor on the GPU
(include/tonk_compress.h tamd_decompress*, tonk_amd/csrc/unlz.h / unlz.hip / decompress.cpp).

Parity is the reference's own pair (oracle/_ref/libmsgcodec_ref.so): its compressor's blocks are
the input, its decompressor's bytes the expected output.  What is checked where
(tests/native/unlz_check.cpp is the host program of all CPU tests):

  one lane (the serial host walk)  every format path against the reference (check); malformed
      blocks and the directed corpus under the address and undefined-behaviour sanitizers
      (mutants, directed); the directed corpus reaches its targets; the ring rule; which paths
      the device's inputs reach (reach).
  64 emulated lanes  the lane protocol without a GPU: where the syncs stand, the rule that
      decides when a match waits for bytes just written, the lane strides, the chunks of 64
      sequences (lanes); every sync site shown necessary or listed with the reason why no valid
      block can show it (sens); the decode-table build phase by phase (tables).
  device  the kernel through the per-message API, the batch and the device-resident chain: the
      reference's and the GPU compressor's blocks of gpu_streams(), the Repeat rewrites and
      hand-made blocks, the directed corpus (batch with canaries, and per message), malformed
      blocks with the walk's verdicts, concurrent callers, recycled device memory.
"""
from __future__ import annotations

import ctypes
import json
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


def test_malformed_blocks_under_sanitizers(stream_file, mutant_cases, directed_cases, tmp_path):
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
    # the directed corpus once under the same build: generator, block writer and walk
    plain, plain_out = directed_cases
    out = str(tmp_path / "directed.bin")
    r = subprocess.run([exe, "directed", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert plain.stdout == r.stdout
    with open(out, "rb") as a, open(plain_out, "rb") as b:
        assert a.read() == b.read()


@pytest.fixture(scope="module")
def rewrites_file(stream_file, tmp_path_factory):
    """The Repeat rewrites and the hand-made blocks of `check`, as blocks (no verdicts)."""
    exe = unlz_check()
    out = str(tmp_path_factory.mktemp("unlz") / "rewrites.bin")
    r = subprocess.run([exe, "check", stream_file, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def directed_cases(tmp_path_factory):
    """The directed corpus (unlz_check directed): the run and its case file.  Generated from
    seeds every time; the generator itself requires of every block that the walk and the
    reference decompressor restore the message."""
    exe = unlz_check()
    out = str(tmp_path_factory.mktemp("unlz") / "directed.bin")
    r = subprocess.run([exe, "directed", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]
    return r, out


WAITS = ("ext_wait", "ext_no_wait", "cross_rest", "cross_none", "match_wait", "match_no_wait")


def test_directed_blocks_reach_their_targets(directed_cases):
    """Each group of the directed corpus reached what it aims at, by the reader's own counters
    and facts: chunks 1..4 chunks of sequences with every count around the multiples of 64;
    hazards both outcomes of each of the three decisions to wait; external the matches into and
    across the previous segment; overlap the overlapping match; sizes both literal buffers, one
    and four Huffman streams, a symbol with and without a long table run, both sides of 1536
    block bytes and the exact block sizes."""
    r, path = directed_cases
    rec = {x["group"]: x for x in map(json.loads, (ln for ln in r.stdout.splitlines() if ln.startswith("{")))}
    assert set(rec) == {"chunks", "hazards", "overlap", "external", "sizes"}
    assert rec["chunks"]["nseq"] == [1, 63, 64, 65, 127, 128, 129, 191, 192, 193]
    assert rec["chunks"]["chunks"] == [1, 2, 3, 4]
    for k in ("ll_predefined", "ml_predefined", "of_predefined"):  # predefined and fitted tables
        assert 0 < rec["chunks"]["paths"][k] < rec["chunks"]["blocks"], k
    assert all(rec["hazards"]["waits"][k] > 0 for k in WAITS), rec["hazards"]["waits"]
    ext = rec["external"]
    assert ext["paths"]["ext_dict_match"] > 0 and ext["paths"]["ext_dict_cross"] > 0 and ext["paths"]["ring_restart"] == 2
    assert ext["waits"]["cross_rest"] > 0 and ext["waits"]["cross_none"] > 0
    assert rec["overlap"]["paths"]["overlap_match"] >= 81
    sz = rec["sizes"]
    assert sz["lit_sel"] == [0, 1] and sz["huf_streams"] == [1, 4] and sz["huf_big_symbol"] == [0, 1] and sz["lit_type"] == [0, 2]
    assert {255, 256, 257, 259, 1535, 1536, 1537} <= set(sz["block_bytes"])
    assert min(sz["block_bytes"]) < 1536 < max(sz["block_bytes"])
    cases = read_cases(path, True)
    assert sum(x["streams"] for x in rec.values()) == len(cases)
    assert 100 < sum(len(m) for _, m in cases) < 1000
    assert all(st == 0 and len(want) <= mx for mx, msgs in cases for _, _, st, want in msgs)


def test_reader_on_64_emulated_lanes(stream_file, rewrites_file, directed_cases):
    """unlz_check lanes: the whole reader on 64 lanes run as fibres inside the kernel's message
    loop, every sync a barrier, one lane at a time between two barriers, in ascending, descending
    and shuffled order: bytes, status, repeat offsets, ring offset and dictionary length after
    every message equal the one-lane walk's, over every stream of cpu_streams() as the reference
    compresses it, the Repeat rewrites, the hand-made blocks and the directed corpus."""
    exe = unlz_check()
    r = subprocess.run([exe, "lanes", stream_file, "blocks=" + rewrites_file, "cases=" + directed_cases[1]],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]
    assert ", 3 orders" in r.stdout


def sync_ordinals():
    """(function, line) -> the ordinal of that TAMD_UNLZ_SYNC() within its function of unlz.h."""
    import re
    out, func, n = {}, None, 0
    with open(os.path.join(ROOT, "tonk_amd", "csrc", "unlz.h")) as f:
        for no, ln in enumerate(f, 1):
            m = re.match(r"TAMD_HD static inline .*?\b(tamd_\w+)\(", ln)
            if m:
                func, n = m.group(1), 0
            if "TAMD_UNLZ_SYNC();" in ln and not ln.startswith("#"):
                n += 1
                out[(func, no)] = n
    return out


# Sync sites that must be shown necessary: skipping one changes an output under some lane order.
NECESSARY_SYNCS = {
    ("tamd_unlz_block", 2): "the chunk arrays are free: lane 0 may decode the next chunk into them",
    ("tamd_unlz_block", 3): "the chunk is decoded: all lanes may execute it",
    ("tamd_unlz_block", 4): "an external match reads ring bytes written since the last sync",
    ("tamd_unlz_block", 5): "the rest of a crossing match reads its own first part",
    ("tamd_unlz_block", 6): "a match reads bytes written since the last sync",
    ("tamd_unlz_literals", 2): "the Huffman table is filled: the stream lanes may read it",
    ("tamd_unlz_literals", 3): "the streams' verdicts are written: every lane returns the same one",
    ("tamd_unlz_fse_table", 1): "cum / nxt / the low symbols' places are written: the spread may read them",
    ("tamd_unlz_fse_table", 2): "the spread is complete: the states may be numbered",
    ("tamd_unlz_fse_table", 3): "every lane has read nxt: the entries may move it on",
    ("tamd_unlz_fse_table", 4): "nxt has moved on: the next group of states may read it",
}
# Sites that no valid block can show necessary, each with the reason.  Any other reached site
# must be shown necessary as well (message_loop: the kernel's loop in unlz.hip, restated in
# unlz_check.cpp; its syncs are numbered in the order of the kernel's source).
UNNEEDED_SYNCS = {
    ("tamd_unlz_block", 1): "lane 0's reset of the block's counters; their first readers stand behind tamd_unlz_seq_header's first sync too",
    ("tamd_unlz_block", 7): "before lane 0 moves S->rep / S->next on: the other lanes hold q0 in a register and read neither before the loop's sync",
    ("tamd_unlz_block", 8): "the message loop's sync follows at once",
    ("tamd_unlz_seq_header", 3): "W->norm free again: tamd_unlz_fse_table's last sync already stands behind its last reader",
    ("tamd_unlz_seq_header", 4): "S->have_pre is next read behind the sync of the next table's description",
    ("tamd_unlz_seq_header", 5): "the chunk loop's first sync follows at once",
    ("tamd_unlz_insert", 2): "the message loop's sync follows at once",
    ("message_loop", 4): "guards S->failed and the status, which only a rejected block changes",
}


def test_sync_sites_are_each_necessary(stream_file, rewrites_file, directed_cases):
    """unlz_check sens: for every sync site the lanes reach, the lanes run through that one site
    without waiting (all alike), and the outputs are compared under the three orders.  Every site
    of NECESSARY_SYNCS is reached and changes an output when skipped, so the emulation would see
    it missing; every other reached site does as well or is listed in UNNEEDED_SYNCS."""
    exe = unlz_check()
    r = subprocess.run([exe, "sens", stream_file, "blocks=" + rewrites_file, "cases=" + directed_cases[1]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]
    ordinal = sync_ordinals()
    verdict = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("site "):
            _, func, line, what = ln.split(None, 3)
            key = (func, int(line)) if func == "message_loop" else (func, ordinal[(func, int(line))])
            verdict[key] = what
            print(key, what)
    for key in NECESSARY_SYNCS:
        assert verdict.get(key, "not reached").startswith("necessary"), (key, verdict.get(key))
    for key, what in verdict.items():
        assert what.startswith("necessary") or key in UNNEEDED_SYNCS, (key, what)
    for key in UNNEEDED_SYNCS:  # (the list holds nothing that has become necessary or is gone)
        assert verdict.get(key) == "unneeded", (key, verdict.get(key))


def test_gpu_inputs_reach_every_reader_path(rewrites_file, directed_cases, tmp_path):
    """What the device is given reaches what the walk's streams reach: the one-lane walk with
    counters over exactly gpu_streams() as the reference compresses them, the directed corpus and
    the block file of test_gpu_repeat_rewrites_and_hand_made_blocks (the only source of the
    Repeat modes, RLE literals and the repeat codes no level-1 compressor writes) runs all 32
    paths and both outcomes of every wait."""
    exe = unlz_check()
    path = str(tmp_path / "gpu_streams.bin")
    write_streams(path, gpu_streams())
    def reach(*more):
        r = subprocess.run([exe, "reach", path, "cases=" + directed_cases[1], *more], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]
        counts = {ln.split()[1]: int(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith(("path ", "wait "))}
        assert len(counts) == 32 + len(WAITS)
        return {k for k, v in counts.items() if v == 0}

    # (the block file holds prefixes of cpu_streams() too: it is asked only for what nothing else has)
    assert reach() <= {"lit_rle", "ll_repeat", "ml_repeat", "of_repeat", "rep1", "rep2", "rep_ll0_2", "rep_ll0_minus1"}
    assert reach("blocks=" + rewrites_file) == set()


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
    """(test_gpu_inputs_reach_every_reader_path: with the directed corpus and the rewrites these
    reach every path of the reader; the last two are there for the repeat offsets and for
    Huffman literals in the job's scratch)"""
    return [(1300, tonk_unit_messages()), (1300, mixed_messages(300, 5)), (1300, skewed(120, 9, 1300))] + \
           [(m, edge_case_messages(m)) for m in (1300, 4000, 24000)] + \
           [(1300, rep_offsets(60, 3)), (8000, skewed(40, 9, 8000))]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(8))
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
@pytest.mark.parametrize("which", range(8))
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
def test_gpu_directed_blocks_batch(directed_cases):
    """The directed corpus through decompress_batch on device memory, one call per maximum size,
    the output slots between 64-byte canaries and filled with the canary byte: every status is 0,
    every restored length and byte is the case file's, and nothing is written behind a message's
    last byte."""
    from tonk_amd.compress import decompress_batch
    hip = Hip()
    cases = read_cases(directed_cases[1], True)
    n_blocks = 0
    for max_bytes in sorted({c[0] for c in cases}):
        group = [c[1] for c in cases if c[0] == max_bytes]
        n_msgs = max(len(g) for g in group)
        pad = (False, b"p" * 16, 0, b"p" * 16)  # (uncompressed, behind everything the generator made)
        group = [g + [pad] * (n_msgs - len(g)) for g in group]
        n_streams, total = len(group), len(group) * n_msgs
        slots = np.zeros((total, max_bytes), dtype=np.uint8)
        in_bytes, is_block = [], []
        for s, g in enumerate(group):
            for k, (isb, data, _, _) in enumerate(g):
                slots[s * n_msgs + k, :len(data)] = np.frombuffer(data, dtype=np.uint8)
                in_bytes.append(len(data))
                is_block.append(int(isb))
        n_blocks += sum(is_block)
        d_in = hip.malloc(total * max_bytes + 32)
        hip.upload(d_in, slots.reshape(-1))
        d_out = hip.malloc(64 + total * max_bytes + 64, fill=0xA5)
        restored, status, _ = decompress_batch(d_in, n_streams, n_msgs, in_bytes, is_block, max_bytes, d_out + 64)
        out = hip.download(d_out, 64 + total * max_bytes + 64)
        assert (out[:64] == 0xA5).all() and (out[-64:] == 0xA5).all()
        body = out[64:-64].reshape(total, max_bytes)
        for s, g in enumerate(group):
            for k, (_, _, _, want) in enumerate(g):
                i = s * n_msgs + k
                assert status[i] == 0 and restored[i] == len(want), (max_bytes, s, k, status[i], restored[i])
                assert body[i, :len(want)].tobytes() == want, (max_bytes, s, k)
                assert (body[i, len(want):] == 0xA5).all(), (max_bytes, s, k)
    hip.close()
    assert n_blocks > 100


@pytest.mark.gpu
def test_gpu_directed_blocks_per_message(directed_cases):
    """The same streams through MessageDecompressor.decompress / insert_uncompressed: the state
    leaves and re-enters LDS at every message, and large literal sections go to the handle's own
    scratch."""
    from tonk_amd.compress import MessageDecompressor
    cases = read_cases(directed_cases[1], True)
    n_blocks = 0
    for s, (max_bytes, msgs) in enumerate(cases):
        dec = MessageDecompressor(max_bytes)
        for k, (isb, data, _, want) in enumerate(msgs):
            if isb:
                assert dec.decompress(data) == want, (s, k)
                n_blocks += 1
            else:
                dec.insert_uncompressed(data)
        dec.close()
    assert n_blocks > 100


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
