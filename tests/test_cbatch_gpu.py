"""The stateful batched compressor and decompressor (include/tonk_compress_batch.h,
tonk_amd.BatchCompressor) on an MI355X against its three yardsticks: the per-message drop-in
(tonk_amd.compress.MessageCompressor) for the blocks, the reference MessageDecompressor for their
restoration, and the reference decompressor's output for what `decompress` returns -- with the
messages spread unevenly over calls, sources at every address offset, canaries in every output
slot, failures that stay with their stream, the refusals, and the chain compress -> build -> parse
-> decompress joined on the device.  The drop-in's blocks and the reference's are computed once
and shared."""
from __future__ import annotations

import numpy as np
import pytest

from batch_ref import Guarded
from lz_streams import (Hip, RefCompressor, RefDecompressor, checked_record, edge_case_messages, mixed_messages, ref_lib,
                        tonk_unit_messages)

pytestmark = [pytest.mark.gpu]

FILL = Guarded.FILL
MAX = 1300
TAMD_LZ_RING = 65536
COMPRESSED, RELIABLE = 5, 6  # TonkineseProtocol.h MessageType_Compressed, MessageType_Reliable


@pytest.fixture(scope="module")
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def L():
    return ref_lib()


def priming(maxb):
    """One lap of the 64 KB ring in random messages of the maximum size, fed to the handle and to
    the drop-ins alike ahead of the streams that are compared.  The compression kernel lets up to
    four bytes behind a message's end into the hash keys of its last positions,
    and during a connection's first 64 KB those are whatever the drop-in's ring held when it was
    allocated or recycled -- the handle's is zeroed.  After one lap both rings hold the same bytes
    in every slot, and the identity is one between defined things."""
    rng = np.random.default_rng(maxb)
    return [rng.integers(0, 256, maxb, dtype=np.uint8).tobytes() for _ in range(TAMD_LZ_RING // maxb + 2)]


def streams_small():
    """Five streams of maximum 1300 behind the priming lap.  A mixed message has about 650 bytes,
    so 80 of them cross the 24,000-byte restart twice and stay below the 64 KB ring; the third mixed
    stream therefore goes on to 120 messages (its first 80 are mixed_messages(80, 13)) and wraps the
    ring again, as the edge cases' 300 messages do several times."""
    return [priming(MAX) + s for s in (tonk_unit_messages(), mixed_messages(80, 11), mixed_messages(80, 12), mixed_messages(120, 13),
                                       edge_case_messages(MAX))]


def streams_large():
    """Two streams of maximum 24000 with messages above TAMD_LZ_MAX_MESSAGE (1536: the scratch path)."""
    return [priming(24000) + s for s in (mixed_messages(12, 21, 24000), edge_case_messages(24000)[:12])]


def streams_sealed():
    """Three mixed streams whose every message ends in seven random bytes: no four bytes that start
    in a message's last seven have occurred before, so no match can begin there and the blocks do
    not depend on what lies behind a message -- not on a new drop-in's uninitialised ring, and not
    on the next message of an abutting pass.  These compare from a connection's first message on."""
    rng = np.random.default_rng(77)
    return [[m[:MAX - 7] + rng.integers(0, 256, 7, dtype=np.uint8).tobytes() for m in mixed_messages(60, 14 + s)] for s in range(3)]


STREAMS = {"small": (streams_small, MAX), "large": (streams_large, 24000), "sealed": (streams_sealed, MAX)}


def skip_of(which):
    """The messages of the priming lap, which are fed and restored but not compared."""
    return 0 if which == "sealed" else len(priming(STREAMS[which][1]))


_cache = {}


def dropin_blocks(which):
    """What MessageCompressor drop-ins, one per stream, return for the streams, b"" for "send as is"."""
    key = ("dropin", which)
    if key not in _cache:
        from tonk_amd.compress import MessageCompressor
        streams, maxb = STREAMS[which][0](), STREAMS[which][1]
        # (all alive at once: a closed drop-in's ring, stale bytes and all, goes to the next one made)
        comps = [MessageCompressor(maxb) for _ in streams]
        out = [[c.compress(m) for m in msgs] for c, msgs in zip(comps, streams)]
        for c in comps:
            c.close()
        _cache[key] = (streams, maxb, out)
    return _cache[key]


def calls_of(n_msgs, pattern):
    """The streams' messages spread over calls: in call c stream s contributes pattern[(c + s) %
    len(pattern)] of its next messages, and the streams' items alternate in the call's array.
    Yields lists of (stream, message index)."""
    done, c = [0] * len(n_msgs), 0
    while any(d < n for d, n in zip(done, n_msgs)):
        take = [min(pattern[(c + s) % len(pattern)], n_msgs[s] - done[s]) for s in range(len(n_msgs))]
        items, k = [], 0
        while any(k < t for t in take):
            items += [(s, done[s] + k) for s in range(len(n_msgs)) if k < take[s]]
            k += 1
        done = [d + t for d, t in zip(done, take)]
        c += 1
        if items:
            yield items


class Scattered:
    """Byte strings in one guarded device buffer, string k at an address whose low four bits are
    (first + k) & 15, `gap` bytes of 0xA5 behind each (none behind the last)."""

    def __init__(self, hip, blobs, first=0, gap=1):
        total = sum(len(b) + gap + 16 for b in blobs) + 16
        self.buf = Guarded(hip, total)
        self.image = np.full(total, FILL, dtype=np.uint8)
        self.addr, at = [], 0
        for k, b in enumerate(blobs):
            at += ((first + k) - (self.buf.ptr + at)) & 15
            self.addr.append(self.buf.ptr + at)
            self.image[at:at + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
            at += len(b) + gap
        self.buf.upload(self.image)

    def check(self):
        self.buf.check()
        assert (self.buf.download() == self.image).all(), "a source buffer was written"


def compress_call(hip, h, streams, items, pitch, first=0):
    """One compress call over `items`; returns the blocks (b"" = send as is) after checking that
    nothing but a block's bytes was written."""
    msgs = [streams[s][k] for s, k in items]
    src = Scattered(hip, msgs, first=first)
    out = Guarded(hip, len(items) * pitch, skew=3)
    written = h.compress([s for s, _ in items], src.addr, [len(m) for m in msgs], out.ptr, pitch)
    got = out.download().reshape(len(items), pitch)
    out.check()
    src.check()
    blocks = []
    for i, m in enumerate(msgs):
        w = int(written[i])
        assert w < max(len(m), 1) and (got[i, w:] == FILL).all(), (i, w, len(m))
        blocks.append(got[i, :w].tobytes())
    return blocks


def compressed(hip, which, abut):
    """The handle's blocks of the streams, per stream in message order, fed in uneven calls."""
    key = ("handle", which, abut)
    if key not in _cache:
        import tonk_amd
        from tonk_amd import cbatch
        streams, maxb, _ = dropin_blocks(which)
        h = tonk_amd.BatchCompressor(len(streams), maxb, sides=cbatch.COMPRESS, abut=abut)
        h.set_timing(True)
        out = [[None] * len(m) for m in streams]
        pattern = [1, 3, 0, 5] if which == "large" else [0, 1, 50, 7, 3]
        n_calls = 0
        for c, items in enumerate(calls_of([len(m) for m in streams], pattern)):
            for (s, k), b in zip(items, compress_call(hip, h, streams, items, maxb + 3, first=c)):
                out[s][k] = b
            n_calls += 1
        ms = h.kernel_ms()
        h.close()
        _cache[key] = (out, n_calls, ms)
    return _cache[key]


def restores(L, maxb, msgs, blocks):
    d = RefDecompressor(L, maxb)
    for k, (m, b) in enumerate(zip(msgs, blocks)):
        assert d.feed(b, m) == m, k


def accepted_by_the_host_checker(tmp_path, maxb, streams, blocks):
    """tests/native/lz_blocks.cpp: every block decodes to its message from matches inside the window."""
    checked_record(tmp_path, [(maxb, list(zip(msgs, bs))) for msgs, bs in zip(streams, blocks)])


# ---- 1, 2. the blocks are the drop-in's, and the reference restores them ----

@pytest.mark.parametrize("which", ["small", "large"])
def test_blocks_equal_the_dropins_and_the_reference_restores_them(hip, L, which, tmp_path):
    """Contract (1) and (2): five streams of maximum 1300 (two of 24000, with messages on the scratch
    path) fed in calls of uneven shape -- in every call one stream is absent, one has a single item
    and, for the small maximum, one has 50 (more than a pass's ring budget), interleaved in the
    item array, sources at every offset 0..15 -- give, per stream, the written values and blocks of
    a MessageCompressor drop-in fed the same messages one by one; tonk::MessageDecompressor
    restores them.  Both sides take the priming lap first (see priming)."""
    streams, maxb, want = dropin_blocks(which)
    got, n_calls, ms = compressed(hip, which, False)
    assert n_calls >= 4 and ms["place_launches"] == ms["compress_launches"] >= n_calls
    skip = skip_of(which)
    for s, msgs in enumerate(streams):
        for k in range(skip, len(msgs)):
            assert len(got[s][k]) == len(want[s][k]), (s, k, len(msgs[k]), len(got[s][k]), len(want[s][k]))
            assert got[s][k] == want[s][k], (s, k, len(msgs[k]))
        restores(L, maxb, msgs, got[s])
    accepted_by_the_host_checker(tmp_path, maxb, streams, got)
    # not vacuous: at least half of the mixed streams' messages of 64 bytes or more are blocks
    mixed = [1, 2, 3] if which == "small" else [0]
    sized = [(len(m), len(b)) for s in mixed for m, b in zip(streams[s][skip:], got[s][skip:]) if len(m) >= 64]
    share = sum(1 for _, b in sized if b) / len(sized)
    print(f"{which}: {n_calls} calls, {share:.2f} of {len(sized)} mixed messages are blocks, "
          f"{sum(n for n, _ in sized) / sum(b if b else n for n, b in sized):.2f}:1")
    assert share >= 0.5
    if which == "large":
        assert any(len(m) > 1536 and b for s in (0, 1) for m, b in zip(streams[s][skip:], got[s][skip:])), "no block from the scratch path"


@pytest.mark.parametrize("which", ["small", "large", "sealed"])
def test_abutting_passes_give_blocks_the_reference_restores(hip, L, which, tmp_path):
    """A handle created with abut takes several messages of a stream per pass (fewer launches for the same
    calls).  Its blocks may differ from the drop-in's in their last sequence (the header says
    why), so the yardsticks are contract (2) and the host checker: the reference restores every
    block, and every match lies inside its message's window.  How many blocks equal the drop-in's
    is printed, not asserted -- except on the sealed streams, whose blocks cannot depend on the
    bytes behind a message: there every block of either handle equals a new drop-in's from the
    first message on."""
    streams, maxb, want = dropin_blocks(which)
    got, n_calls, ms = compressed(hip, which, True)
    _, _, ms_exact = compressed(hip, which, False)
    assert ms["place_launches"] == ms["compress_launches"] < ms_exact["compress_launches"]
    for s, msgs in enumerate(streams):
        restores(L, maxb, msgs, got[s])
    accepted_by_the_host_checker(tmp_path, maxb, streams, got)
    skip = skip_of(which)
    total = sum(len(m) - skip for m in streams)
    same = sum(g == w for gs, ws in zip(got, want) for g, w in zip(gs[skip:], ws[skip:]))
    if which == "sealed":
        assert same == total and compressed(hip, which, False)[0] == want and sum(1 for bs in want for b in bs if b) >= total // 2
    print(f"{which}: {same} of {total} blocks equal the drop-in's; compression launches {ms['compress_launches']:.0f} "
          f"against {ms_exact['compress_launches']:.0f}")


# ---- 3. decompression ----

def ref_inputs(L, streams, maxb):
    key = ("ref", maxb, len(streams))
    if key not in _cache:
        out = []
        for msgs in streams:
            c = RefCompressor(L, maxb)
            out.append([c.compress(m) for m in msgs])
        _cache[key] = out
    return _cache[key]


def decompress_call(hip, h, items, pitch, first=0):
    """One decompress call over items (stream, is_block, bytes): inputs at odd offsets inside a
    larger buffer with 33 bytes between them.  Returns per item (status, restored bytes or None for
    an item that is no block), after checking the canaries: a slot is written only as far as a
    block restores."""
    src = Scattered(hip, [d for _, _, d in items], first=first, gap=33)
    out = Guarded(hip, len(items) * pitch, skew=5)
    restored, status = h.decompress([s for s, _, _ in items], src.addr, [len(d) for _, _, d in items], [b for _, b, _ in items],
                                    out.ptr, pitch)
    got = out.download().reshape(len(items), pitch)
    out.check()
    src.check()
    res = []
    for i, (s, isb, d) in enumerate(items):
        r = int(restored[i])
        if status[i] == 0 and not isb:
            assert r == len(d)
            r = 0
        if status[i] != 0:
            assert r == 0
        # (a rejected block may have written what it restored before the error: only its slot)
        keep = got[i, r:] if status[i] == 0 else got[i, h.max_message_bytes:]
        assert (keep == FILL).all(), (i, s, isb, int(status[i]), r)
        res.append((int(status[i]), got[i, :r].tobytes() if isb and status[i] == 0 else None))
    return res


@pytest.mark.parametrize("source", ["reference", "handle"])
def test_decompress_returns_what_the_reference_decompressor_returns(hip, L, source):
    """Contract (3): the reference compressor's blocks and the handle's own (made in other call
    splits), in place at odd offsets, give item by item the bytes of tonk::MessageDecompressor;
    messages sent as is never write their slot."""
    import tonk_amd
    from tonk_amd import cbatch
    streams, maxb, _ = dropin_blocks("small")
    blocks = ref_inputs(L, streams, maxb) if source == "reference" else compressed(hip, "small", False)[0]
    assert sum(1 for bs in blocks for b in bs if b) > 100 and sum(1 for bs in blocks for b in bs if not b) > 20
    refs = [RefDecompressor(L, maxb) for _ in streams]
    h = tonk_amd.BatchCompressor(len(streams), maxb, sides=cbatch.DECOMPRESS)
    try:
        for c, call in enumerate(calls_of([len(m) for m in streams], [3, 0, 1, 20, 2, 64])):
            items = [(s, 1 if blocks[s][k] else 0, blocks[s][k] or streams[s][k]) for s, k in call]
            res = decompress_call(hip, h, items, maxb + 5, first=c + 1)
            for (s, k), (_, isb, d), (status, out) in zip(call, items, res):
                want = refs[s].feed(blocks[s][k], streams[s][k])
                assert status == 0, (s, k, status)
                if isb:
                    assert out == want == streams[s][k], (s, k)
    finally:
        h.close()


def test_decompress_large_maximum(hip, L):
    """The same for maximum 24000 (blocks above 1536 bytes are read in place, literals in scratch)."""
    import tonk_amd
    from tonk_amd import cbatch
    streams, maxb, _ = dropin_blocks("large")
    blocks = ref_inputs(L, streams, maxb)
    h = tonk_amd.BatchCompressor(len(streams), maxb, sides=cbatch.DECOMPRESS)
    try:
        for c, call in enumerate(calls_of([len(m) for m in streams], [2, 5, 0, 1])):
            items = [(s, 1 if blocks[s][k] else 0, blocks[s][k] or streams[s][k]) for s, k in call]
            for (s, k), (_, isb, _d), (status, out) in zip(call, items, decompress_call(hip, h, items, maxb + 5, first=c)):
                assert status == 0 and (not isb or out == streams[s][k]), (s, k, status)
    finally:
        h.close()


# ---- 4. failure is per stream and sticky; reset ----

def test_failure_stays_with_its_stream_until_reset(hip, L):
    import tonk_amd
    from tonk_amd import cbatch
    streams = [mixed_messages(14, 31 + s) for s in range(3)]
    fresh = mixed_messages(5, 40)
    blocks = []
    for msgs in streams:
        c = RefCompressor(L, MAX)
        blocks.append([c.compress(m) for m in msgs])
    k_bad = next(k for k, b in enumerate(blocks[1]) if b and 1 <= k <= 5)
    truncated = blocks[1][k_bad][:-3]
    d = RefDecompressor(L, MAX)
    for k in range(k_bad):
        d.feed(blocks[1][k], streams[1][k])
    assert d.decompress(truncated) is None, "the reference accepts the truncated block"

    def item(s, k):
        b = truncated if (s, k) == (1, k_bad) else blocks[s][k]
        return (s, 1 if b else 0, b or streams[s][k])

    h = tonk_amd.BatchCompressor(3, MAX, sides=cbatch.DECOMPRESS)
    try:
        first = [(s, k) for k in range(6) for s in range(3)]
        res = decompress_call(hip, h, [item(s, k) for s, k in first], MAX)
        for (s, k), (status, out) in zip(first, res):
            if s == 1 and k == k_bad:
                assert -12 <= status <= -1, status  # the walk's reason
            elif s == 1 and k > k_bad:
                assert status == cbatch.STREAM_FAILED, (k, status)
            else:
                assert status == 0 and (out is None or out == streams[s][k]), (s, k, status)
        second = [(s, k) for k in range(6, 9) for s in range(3)]
        res = decompress_call(hip, h, [item(s, k) for s, k in second], MAX)
        for (s, k), (status, out) in zip(second, res):
            if s == 1:
                assert status == cbatch.STREAM_FAILED, (k, status)
            else:
                assert status == 0 and (out is None or out == streams[s][k]), (s, k, status)
        # a size no message can have fails its stream (2) and does not refuse the call
        third = [(2, 1, bytes(MAX + 1)), item(2, 9), item(0, 9)]
        res = decompress_call(hip, h, third, MAX)
        assert [st for st, _ in res[:2]] == [cbatch.BAD_SIZE, cbatch.STREAM_FAILED], res[:2]
        assert res[2][0] == 0 and (res[2][1] is None or res[2][1] == streams[0][9])
        # reset of stream 1 alone: a fresh reference stream restores there, stream 0 goes on with
        # its history, stream 2 stays failed
        h.reset([1], cbatch.DECOMPRESS)
        c = RefCompressor(L, MAX)
        again = [c.compress(m) for m in fresh]
        items = [(1, 1 if b else 0, b or m) for b, m in zip(again, fresh)] + [item(0, k) for k in range(10, 14)] + [item(2, 10)]
        want = fresh + streams[0][10:14] + [None]
        assert sum(1 for s, isb, _ in items if s == 0 and isb) >= 2 and sum(1 for s, isb, _ in items if s == 1 and isb) >= 2
        for (s, _, _), m, (status, out) in zip(items, want, decompress_call(hip, h, items, MAX)):
            if s == 2:
                assert status == cbatch.STREAM_FAILED, status
            else:
                assert status == 0 and (out is None or out == m), (s, status)
    finally:
        h.close()


def test_reset_of_the_compress_side_starts_a_new_stream(hip):
    import tonk_amd
    from tonk_amd import cbatch
    streams, maxb, want = dropin_blocks("sealed")
    h = tonk_amd.BatchCompressor(3, maxb, sides=cbatch.COMPRESS)
    try:
        # stream 1 takes 30 messages of another stream first, stream 2 is never reset
        compress_call(hip, h, [None, streams[0], streams[2]], [(1, k) for k in range(30)] + [(2, k) for k in range(4)], maxb)
        h.reset([1], cbatch.COMPRESS)
        items = [(1, k) for k in range(12)] + [(2, k) for k in range(4, 12)]
        got = compress_call(hip, h, streams, items, maxb)
        for (s, k), b in zip(items, got):
            assert b == want[s][k], (s, k)
        with pytest.raises(RuntimeError, match="rc=-1"):
            h.reset([1], cbatch.DECOMPRESS)  # a side the handle was not created with
    finally:
        h.close()


# ---- 5. refusals move no state ----

def test_refused_calls_move_no_state(hip, L):
    import tonk_amd
    from tonk_amd import cbatch
    from tonk_amd._handle import arr, ptr, u32p, u64p
    streams, maxb, want = dropin_blocks("sealed")
    h = tonk_amd.BatchCompressor(2, maxb)
    try:
        msgs = streams[1][:6]
        src = Scattered(hip, msgs)
        out = Guarded(hip, 6 * maxb)
        lens = [len(m) for m in msgs]
        for args, rc in ((([0, 2, 1, 0, 1, 0], src.addr, lens, out.ptr, maxb), -2),
                         (([0] * 6, src.addr, lens, out.ptr, maxb - 1), -3),
                         (([0] * 6, src.addr, lens[:5] + [0], out.ptr, maxb), -1),
                         (([0] * 6, src.addr, lens[:5] + [maxb + 1], out.ptr, maxb), -1),
                         (([0] * 6, src.addr[:5] + [0], lens, out.ptr, maxb), -1),
                         (([0] * 6, src.addr, lens, 0, maxb), -1)):
            with pytest.raises(RuntimeError, match=f"rc={rc}:"):
                h.compress(*args)
        S, A, B = arr([0] * 6, "uint32"), arr(src.addr, "uint64"), arr(lens, "uint32")
        assert h._c.compress(h._h, 6, ptr(S, u32p), ptr(A, u64p), ptr(B, u32p), out.ptr, maxb, None) == -1
        assert h._c.compress(h._h, 6, None, ptr(A, u64p), ptr(B, u32p), out.ptr, maxb, None) == -1
        assert h._c.compress(None, 0, None, None, None, None, maxb, None) == -1
        assert (out.download() == FILL).all()
        # stream 0 is still fresh: its blocks are a new drop-in's first ones
        got = compress_call(hip, h, [streams[1]], [(0, k) for k in range(6)], maxb)
        assert got == want[1][:6] and any(got)
        # the same on the other side
        c = RefCompressor(L, maxb)
        blocks = [c.compress(m) for m in msgs]
        items = [(0, 1 if b else 0, b or m) for b, m in zip(blocks, msgs)]
        ins = Scattered(hip, [d for _, _, d in items], gap=33)
        n = len(items)
        for args, rc in ((([0] * 5 + [2], ins.addr, [len(d) for _, _, d in items], [b for _, b, _ in items], out.ptr, maxb), -2),
                         (([0] * n, ins.addr, [len(d) for _, _, d in items], [b for _, b, _ in items], out.ptr, maxb - 1), -3),
                         (([0] * n, ins.addr, [len(d) for _, _, d in items], [b for _, b, _ in items], 0, maxb), -1)):
            with pytest.raises(RuntimeError, match=f"rc={rc}:"):
                h.decompress(*args)
        for m, (status, got1) in zip(msgs, decompress_call(hip, h, items, maxb)):
            assert status == 0 and (got1 is None or got1 == m)
    finally:
        h.close()


# ---- 6. the chain: compress -> build -> parse -> decompress, in place ----

def test_chain_compress_build_parse_decompress(hip):
    import tonk_amd
    n_streams, per_tick, pitch_d = 3, 4, 8192
    streams = [mixed_messages(8, 50 + s) for s in range(n_streams)]
    sender = tonk_amd.BatchCompressor(n_streams, MAX, sides=tonk_amd.cbatch.COMPRESS)
    receiver = tonk_amd.BatchCompressor(n_streams, MAX, sides=tonk_amd.cbatch.DECOMPRESS)
    framer = tonk_amd.DatagramFramer(65535)
    try:
        blocks_seen = plain_seen = 0
        for tick in range(2):
            items = [(s, tick * per_tick + k) for k in range(per_tick) for s in range(n_streams)]
            msgs = [streams[s][k] for s, k in items]
            src = Scattered(hip, msgs, first=tick + 3)
            comp = Guarded(hip, len(items) * MAX)
            written = sender.compress([s for s, _ in items], src.addr, [len(m) for m in msgs], comp.ptr, MAX)
            # one datagram per stream: its messages in order, the block where there is one, else the original
            order = sorted(range(len(items)), key=lambda i: items[i])
            dg = [items[i][0] for i in order]
            mt = [COMPRESSED if written[i] else RELIABLE for i in order]
            mb = [int(written[i]) if written[i] else len(msgs[i]) for i in order]
            ms = [comp.ptr + i * MAX if written[i] else src.addr[i] for i in order]
            dgrams = Guarded(hip, n_streams * pitch_d)
            ones, zeros = [1] * n_streams, [0] * n_streams
            out_bytes, message_bytes, _, _, rc = framer.build(dg, mt, mb, ms, [tick + 1] * n_streams, ones, [7] * n_streams, ones, zeros,
                                                              zeros, dgrams.ptr, pitch_d)
            assert (rc == 0).all() and (out_bytes + 32 <= pitch_d).all()
            status, count, _, _, table = framer.parse(message_bytes, dgrams.ptr, pitch_d, mode=0, cap=per_tick)
            assert (status == 0).all() and (count == per_tick).all()
            # decompress in place from the positions the parse returned
            d_stream, d_src, d_bytes, d_isb = [], [], [], []
            for d in range(n_streams):
                for e in table[d]:
                    t, nb, off = int(e) >> 27, (int(e) >> 16) & 2047, int(e) & 0xFFFF
                    assert t in (COMPRESSED, RELIABLE)
                    d_stream.append(d)
                    d_src.append(dgrams.ptr + d * pitch_d + off)
                    d_bytes.append(nb)
                    d_isb.append(1 if t == COMPRESSED else 0)
            out = Guarded(hip, len(d_src) * MAX)
            restored, st = receiver.decompress(d_stream, d_src, d_bytes, d_isb, out.ptr, MAX)
            assert (st == 0).all()
            got = out.download().reshape(len(d_src), MAX)
            image = dgrams.download()
            for j, i in enumerate(order):
                if d_isb[j]:
                    assert got[j, :restored[j]].tobytes() == msgs[i], (tick, j)
                    blocks_seen += 1
                else:
                    at = d_src[j] - dgrams.ptr
                    assert restored[j] == len(msgs[i]) and image[at:at + d_bytes[j]].tobytes() == msgs[i], (tick, j)
                    assert (got[j] == FILL).all()
                    plain_seen += 1
            for g in (comp, dgrams, out):
                g.check()
            src.check()
        assert blocks_seen >= 6 and plain_seen >= 2, (blocks_seen, plain_seen)
    finally:
        for x in (sender, receiver, framer):
            x.close()


# ---- 7. calls larger than one launch's scratch ----

LARGE = 24000
LZ_MAX_MESSAGE = 1536        # lz.h `#define TAMD_LZ_MAX_MESSAGE 1536u`: larger messages take scratch
SCRATCH_BUDGET = 64 << 20    # cbatch.cpp `const size_t kScratchBudget = (size_t)64 << 20`


def lz_scratch_bytes(n):
    """lz.h tamd_lz_scratch_bytes: `(8u * S + 4u * ((n + 64u) / 4u + 4u) + 6u * S + 15u) & ~15u` with
    S = tamd_lz_big_seqs(n) = `n / 4u + 1u`."""
    S = n // 4 + 1
    return (8 * S + 4 * ((n + 64) // 4 + 4) + 6 * S + 15) & ~15


# cbatch.cpp tamd_cbatch_compress cuts a pass at `big && scr + big > kScratchBudget`: 620 messages of
# 24000 bytes (108,096 bytes of scratch each) fit one launch, the 621st starts the next
COMPRESS_FIT = SCRATCH_BUDGET // lz_scratch_bytes(LARGE)
# cbatch.cpp tamd_cbatch_decompress: `per_launch = kScratchBudget / scratch_each` with scratch_each =
# align16(maxb) streams in a launch, stream job k in slot `k % per_launch`: 2796, so job 2796 reuses slot 0
DECOMPRESS_FIT = SCRATCH_BUDGET // ((LARGE + 15) & ~15)
EXTRA = 3  # streams beyond the large call's, for the small calls around it


def large_templates():
    """Nine streams of two messages of 24000 bytes in the style of streams_sealed: stretches of
    words, of random bytes and repeats of earlier stretches (the second message's reach into the
    first), the last seven bytes random.  The ninth stream's first message is random throughout:
    it is sent as is."""
    if "templates" not in _cache:
        words = [b"siamese ", b"tonk ", b"packet ", b"recovery ", b"window ", b"lane ", b"sum ", b"ack ", b"0123 "]
        out = []
        for t in range(9):
            rng = np.random.default_rng(900 + t)
            stream, msgs = bytearray(), []
            for k in range(2):
                m = bytearray()
                while len(m) < LARGE - 7:
                    kind, ln = int(rng.integers(0, 3)), int(rng.integers(200, 2500))
                    if t == 8 and k == 0:
                        kind, ln = 1, LARGE
                    if kind == 0:
                        piece = b"".join(words[int(i)] for i in rng.integers(0, len(words), ln // 4))[:ln]
                    elif kind == 1 or len(stream) + len(m) < 4000:
                        piece = rng.integers(0, 256, min(ln, 700) if t < 8 else ln, dtype=np.uint8).tobytes()
                    else:
                        whole = bytes(stream) + bytes(m)
                        start = int(rng.integers(max(0, len(whole) - 30000), len(whole) - 100))
                        piece = whole[start:start + ln]
                    m += piece
                m = bytes(m[:LARGE - 7]) + rng.integers(0, 256, 7, dtype=np.uint8).tobytes()
                stream += m
                msgs.append(m)
            out.append(msgs)
        _cache["templates"] = out
    return _cache["templates"]


def test_compress_call_larger_than_one_launchs_scratch(hip, L):
    """One call with a 24000-byte message for each of COMPRESS_FIT + 2 = 622 fresh streams of one
    pass takes two compression launches (asserted); a call of three streams before it and one of
    four after it on the same handle make the staging and the scratch grow and be used again.
    Every block is the first (after: the second) block of a MessageCompressor drop-in for the
    stream's template, and the reference decompressor restores it."""
    import tonk_amd
    from tonk_amd import cbatch
    from tonk_amd.compress import MessageCompressor
    assert lz_scratch_bytes(LARGE) == 108096 and COMPRESS_FIT == 620 and LARGE > LZ_MAX_MESSAGE
    n_big = COMPRESS_FIT + 2
    templates = large_templates()[:8]
    comps = [MessageCompressor(LARGE) for _ in templates]
    want = [[c.compress(m) for m in msgs] for c, msgs in zip(comps, templates)]
    for c in comps:
        c.close()
    assert all(0 < len(b) < LARGE for bs in want for b in bs), [[len(b) for b in bs] for bs in want]
    for msgs, bs in zip(templates, want):
        restores(L, LARGE, msgs, bs)
    streams = [templates[s % 8] for s in range(n_big + EXTRA)]
    h = tonk_amd.BatchCompressor(n_big + EXTRA, LARGE, sides=cbatch.COMPRESS, abut=False)
    h.set_timing(True)
    try:
        def call(items, first):
            h.kernel_ms()
            got = compress_call(hip, h, streams, items, LARGE + 3, first=first)
            for (s, k), b in zip(items, got):
                assert len(b) > 0 and b == want[s % 8][k], (s, k, len(b), len(want[s % 8][k]))
            return h.kernel_ms()["compress_launches"]

        assert call([(n_big + e, 0) for e in range(EXTRA)], 1) == 1
        assert call([(s, 0) for s in range(n_big)], 2) == -(-n_big // COMPRESS_FIT) == 2
        assert call([(n_big, 1), (n_big + 1, 1), (0, 1), (n_big - 1, 1)], 3) == 1
    finally:
        h.close()


def test_decompress_call_larger_than_one_launchs_scratch(hip, L):
    """One call with one item for each of DECOMPRESS_FIT + 1 = 2797 streams takes two launches
    (asserted) whose jobs reuse the scratch slots: streams 0 and 2796 share slot 0.  The items are
    the reference compressor's blocks of the templates (all restore to 24000 bytes: literals in
    scratch) and, every 97th, a message sent as is.  A second call gives a subset of the streams
    their second message: each kept its own history.  Small calls on three more streams before and
    after."""
    import tonk_amd
    from tonk_amd import cbatch
    assert DECOMPRESS_FIT == 2796
    n_big = DECOMPRESS_FIT + 1
    templates = large_templates()
    blocks = []
    for msgs in templates:
        c = RefCompressor(L, LARGE)
        blocks.append([c.compress(m) for m in msgs])
    assert all(b for bs in blocks[:8] for b in bs) and not blocks[8][0] and blocks[8][1]
    template_of = lambda s: 8 if s % 97 == 5 else s % 8
    as_is = [s for s in range(n_big) if template_of(s) == 8]
    assert 3 <= len(as_is) <= n_big // 20 and 0 not in as_is and DECOMPRESS_FIT not in as_is
    assert sum(1 for s in range(n_big) if len(templates[template_of(s)][0]) > LZ_MAX_MESSAGE and blocks[template_of(s)][0]) >= n_big // 2

    def item(s, k):
        b = blocks[template_of(s)][k]
        return (s, 1 if b else 0, b or templates[template_of(s)][k])

    h = tonk_amd.BatchCompressor(n_big + EXTRA, LARGE, sides=cbatch.DECOMPRESS)
    h.set_timing(True)
    try:
        def call(entries, first):
            h.kernel_ms()
            res = decompress_call(hip, h, [item(s, k) for s, k in entries], LARGE + 5, first=first)
            for (s, k), (status, out) in zip(entries, res):
                assert status == 0, (s, k, status)
                if blocks[template_of(s)][k]:
                    assert out == templates[template_of(s)][k], (s, k)
                else:
                    assert out is None
            return h.kernel_ms()["decompress_launches"], res

        assert call([(n_big + e, 0) for e in range(EXTRA)], 1)[0] == 1
        launches, res = call([(s, 0) for s in range(n_big)], 2)
        assert launches == -(-n_big // DECOMPRESS_FIT) == 2
        # slot 0's two users: the streams are listed in order, so job k is stream k
        assert res[0][1] == templates[template_of(0)][0] and res[DECOMPRESS_FIT][1] == templates[template_of(DECOMPRESS_FIT)][0]
        again = sorted({0, DECOMPRESS_FIT, DECOMPRESS_FIT - 1, 1} | set(as_is[:2]) | set(range(7, n_big, 131)))
        assert call([(s, 1) for s in again], 3)[0] == 1
        assert call([(n_big + e, 1) for e in range(EXTRA)] + [(2, 1)], 4)[0] == 1
    finally:
        h.close()
