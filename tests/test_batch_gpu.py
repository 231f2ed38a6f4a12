"""The batched codecs over the caller's device packets (include/tonk_batch.h, tonk_amd.BatchCodec)
on an MI355X against the reference codec (oracle/_ref/libsiamese_ref.so) driven through ctypes with
the same calls in the same per-stream order: packet numbers, result codes, recovery packets,
acknowledgements and recovered payloads must be equal.  Every caller buffer has 64 guard bytes of
0xA5 on each side, checked after every call."""
from __future__ import annotations

import os

import numpy as np
import pytest

from batch_ref import (DISABLED, DUPLICATE, INVALID, LENGTHS, NEED_MORE, REF, SUCCESS, Guarded, RefDecoder, RefEncoder,
                       slots)
from lz_streams import Hip

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not os.path.exists(REF), reason="reference codec not built (oracle/Makefile)")]

MAXB = 4000
OVER = 11  # TAMD_BATCH_RECOVERY_OVERHEAD
LENS18 = LENGTHS[:18]
N_STREAMS, N_ORIG, PER_CALL = 3, 72, 9
ENCODE_LIST = [0, 1, 1, 2]  # every stream, stream 1 twice


def stream_lengths(s):
    rot = LENS18[s % 18:] + LENS18[:s % 18]
    return (rot * 4)[:N_ORIG]


def make_payloads(n_streams, lengths_of, seed):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths_of(s)] for s in range(n_streams)]


@pytest.fixture(scope="module")
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def payloads():
    return make_payloads(N_STREAMS, stream_lengths, 7)


def reference_traffic(payloads, n_orig):
    """The reference encoders' traffic for the three streams: per round and stream the recovery
    packets of ENCODE_LIST, then six more per stream at the end."""
    encs = [RefEncoder() for _ in range(N_STREAMS)]
    rounds = []
    for r in range(n_orig // PER_CALL):
        for s in range(N_STREAMS):
            for k in range(PER_CALL):
                rc, pn = encs[s].add(payloads[s][r * PER_CALL + k])
                assert rc == 0 and pn == r * PER_CALL + k
        recs = []
        for s in ENCODE_LIST:
            rc, data = encs[s].encode()
            assert rc == 0
            recs.append((s, data))
        rounds.append(recs)
    tail = []
    for k in range(6):
        for s in range(N_STREAMS):
            rc, data = encs[s].encode()
            assert rc == 0
            tail.append((s, data))
    rounds.append(tail)
    for e in encs:
        e.close()
    return rounds


@pytest.fixture(scope="module")
def ref_traffic(payloads):
    """(computed once)"""
    return reference_traffic(payloads, N_ORIG)


def new_codec(n_streams=N_STREAMS, maxb=MAXB, arena=96 << 20):
    import tonk_amd
    return tonk_amd.BatchCodec(n_streams, maxb, arena)


def check_all(*bufs):
    for b in bufs:
        b.check()


def recovery_slots(out, pitch, nbytes):
    """Recovery packets of an encode's output buffer; bytes past each packet must keep the fill."""
    raw = out.download()
    got = []
    for i, n in enumerate(nbytes):
        slot = raw[i * pitch:(i + 1) * pitch]
        assert (slot[n:] == Guarded.FILL).all(), f"slot {i} written past its {n} bytes"
        got.append(slot[:n].tobytes())
    return got


@pytest.mark.parametrize("pitch,skew", [(4001, 0), (4096, 0), (4001, 5)])
def test_encoder_matches_reference(hip, payloads, pitch, skew):
    out_pitch = pitch + OVER if pitch == 4001 else pitch  # 4012 (odd slots) / 4096
    bc = new_codec()
    refs = [RefEncoder() for _ in range(N_STREAMS)]
    ref_dec = [RefDecoder() for _ in range(N_STREAMS)]
    src = Guarded(hip, N_STREAMS * PER_CALL * pitch, skew)
    out = Guarded(hip, len(ENCODE_LIST) * out_pitch, skew)
    try:
        # nothing added yet: NeedMoreData on both
        out.fill()
        nb, rc = bc.encode(ENCODE_LIST, out.ptr, out_pitch)
        assert [r.encode()[0] for r in (refs[0], refs[1], refs[1], refs[2])] == [NEED_MORE] * 4
        assert list(rc) == [NEED_MORE] * 4 and list(nb) == [0] * 4
        check_all(src, out)
        assert (out.download() == Guarded.FILL).all()
        for r in range(N_ORIG // PER_CALL):
            # the call's packets, streams interleaved (list order inside a stream is the add order)
            stream = [s for k in range(PER_CALL) for s in range(N_STREAMS)]
            index = [r * PER_CALL + k for k in range(PER_CALL) for s in range(N_STREAMS)]
            pk = [payloads[s][i] for s, i in zip(stream, index)]
            src.upload(slots(pk, pitch))
            pn, rc = bc.encoder_add(stream, [len(p) for p in pk], src.ptr, pitch)
            want = [refs[s].add(p) for s, p in zip(stream, pk)]
            assert list(rc) == [w[0] for w in want] and list(pn) == [w[1] for w in want]
            check_all(src, out)
            out.fill()
            nb, rc = bc.encode(ENCODE_LIST, out.ptr, out_pitch)
            want = [refs[s].encode() for s in ENCODE_LIST]
            assert list(rc) == [w[0] for w in want], r
            assert list(nb) == [len(w[1]) for w in want], r
            got = recovery_slots(out, out_pitch, nb)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w[1], f"round {r} recovery packet {i} (stream {ENCODE_LIST[i]}) differs"
            check_all(src, out)
            for s, w in zip(ENCODE_LIST, want):
                assert ref_dec[s].add_recovery(w[1]) == 0
            for s in range(N_STREAMS):
                for k in range(PER_CALL):
                    i = r * PER_CALL + k
                    if i not in (5, 20):
                        assert ref_dec[s].add_original(i, payloads[s][i]) == 0
            if r == 3:  # after the fourth add call: the receivers' acknowledgements
                for s in range(N_STREAMS):
                    arc, ack = ref_dec[s].ack()
                    assert arc == 0 and ack
                    assert bc.encoder_ack(s, ack) == refs[s].ack(ack)
    finally:
        bc.close()
        for x in refs + ref_dec:
            x.close()


def test_encode_of_a_single_packet(hip):
    """A stream holding one packet gets the single-packet row; its neighbour holds nothing."""
    bc = new_codec(2, 1300, 16 << 20)
    ref = RefEncoder()
    src, out = Guarded(hip, 1300), Guarded(hip, 2 * 1311, 3)
    try:
        data = bytes(range(256)) * 5 + b"xyz"
        src.upload(slots([data[:1283]], 1300))
        pn, rc = bc.encoder_add([0], [1283], src.ptr, 1300)
        assert (list(pn), list(rc)) == ([0], [0]) and ref.add(data[:1283]) == (0, 0)
        out.fill()
        nb, rc = bc.encode([0, 1], out.ptr, 1311)
        want = ref.encode()
        assert list(rc) == [want[0], NEED_MORE] and list(nb) == [len(want[1]), 0]
        assert recovery_slots(out, 1311, nb)[0] == want[1]
        check_all(src, out)
    finally:
        bc.close()
        ref.close()


def lost_original(i):
    return i % 11 == 3 or 40 <= i <= 44


def decode_and_compare(bc, ref_dec, out, pitch, cap, tag):
    out.fill()
    rc, o_s, o_n, o_b = bc.decode(list(range(len(ref_dec))), out.ptr, pitch, cap)
    want = [d.decode_if_ready() for d in ref_dec]
    assert list(rc) == [w[0] for w in want], tag
    flat = [(s, num, data) for s, w in enumerate(want) for num, data in w[1]]
    assert list(o_s) == [f[0] for f in flat] and list(o_n) == [f[1] for f in flat], tag
    assert list(o_b) == [len(f[2]) for f in flat], tag
    raw = out.download()
    for j, f in enumerate(flat):
        slot = raw[j * pitch:(j + 1) * pitch]
        assert slot[:len(f[2])].tobytes() == f[2], f"{tag}: recovered packet {f[1]} of stream {f[0]} differs"
        assert (slot[len(f[2]):] == Guarded.FILL).all(), f"{tag}: slot {j} written past its payload"
    assert (raw[len(flat) * pitch:] == Guarded.FILL).all(), tag
    out.check()
    return flat


@pytest.mark.parametrize("pitch", [4001, 4096])
def test_decoder_matches_reference(hip, payloads, ref_traffic, pitch):
    rec_pitch = pitch + OVER if pitch == 4001 else pitch
    bc = new_codec()
    ref_dec = [RefDecoder() for _ in range(N_STREAMS)]
    src = Guarded(hip, N_STREAMS * PER_CALL * pitch, 1)
    rec = Guarded(hip, 18 * rec_pitch, 2)
    out = Guarded(hip, 32 * pitch, 7)
    recovered = 0
    try:
        for r, recs in enumerate(ref_traffic):
            if r < N_ORIG // PER_CALL:
                ent = [(s, r * PER_CALL + k) for k in range(PER_CALL) for s in range(N_STREAMS)
                       if not lost_original(r * PER_CALL + k)]
                pk = [payloads[s][i] for s, i in ent]
                src.upload(slots(pk, pitch))
                rc = bc.decoder_add_original([e[0] for e in ent], [e[1] for e in ent], [len(p) for p in pk], src.ptr, pitch)
                assert list(rc) == [ref_dec[s].add_original(i, p) for (s, i), p in zip(ent, pk)]
                check_all(src, rec, out)
                recovered += len(decode_and_compare(bc, ref_dec, out, pitch, 32, f"round {r} originals"))
            rec.upload(slots([d for _, d in recs], rec_pitch))
            rc = bc.decoder_add_recovery([s for s, _ in recs], [len(d) for _, d in recs], rec.ptr, rec_pitch)
            assert list(rc) == [ref_dec[s].add_recovery(d) for s, d in recs], r
            check_all(src, rec, out)
            recovered += len(decode_and_compare(bc, ref_dec, out, pitch, 32, f"round {r} recovery"))
            for s in range(N_STREAMS):
                assert bc.decoder_ack(s) == ref_dec[s].ack(), (r, s)
        assert recovered >= 20  # (the losses are mostly recovered: the comparison is not vacuous)
    finally:
        bc.close()
        for x in ref_dec:
            x.close()


def test_round_trip_on_the_device(hip):
    """16 streams x 192 originals through both sides of one handle: the encode output buffer is the
    add_recovery input (lost entries get 0 bytes and are skipped with rc 1), 3 % seeded loss on
    originals and recovery packets alike, acknowledgements every second tick.  The reference codec,
    driven on the CPU with the same calls and deliveries, says what must be recovered."""
    n_streams, n_orig, tick, n_rec, pitch = 16, 192, 16, 2, 1311
    rng = np.random.default_rng(99)
    odd_lens = rng.integers(1, 1301, (n_streams, n_orig))
    pay = make_payloads(n_streams, lambda s: [1300] * n_orig if s % 2 == 0 else list(odd_lens[s]), 5)
    lost_o = rng.random((n_streams, n_orig)) < 0.03
    lost_r = rng.random((n_streams, n_orig // tick * n_rec)) < 0.03
    bc = new_codec(n_streams, 1300, 256 << 20)
    r_enc = [RefEncoder() for _ in range(n_streams)]
    r_dec = [RefDecoder() for _ in range(n_streams)]
    src = Guarded(hip, n_streams * tick * pitch, 9)
    rec = Guarded(hip, n_streams * n_rec * pitch, 1)
    out = Guarded(hip, 64 * pitch, 0)
    want_all, got_all = [], []
    try:
        for t in range(n_orig // tick):
            ent = [(s, t * tick + k) for s in range(n_streams) for k in range(tick)]
            pk = [pay[s][i] for s, i in ent]
            src.upload(slots(pk, pitch))
            streams, lens = [e[0] for e in ent], [len(p) for p in pk]
            pn, rc = bc.encoder_add(streams, lens, src.ptr, pitch)
            assert list(rc) == [0] * len(ent) and list(pn) == [e[1] for e in ent]
            for (s, i), p in zip(ent, pk):
                assert r_enc[s].add(p) == (0, i)
            # the same buffer into the receivers, lost originals skipped
            dl = [0 if lost_o[s, i] else n for (s, i), n in zip(ent, lens)]
            rc = bc.decoder_add_original(streams, [e[1] for e in ent], dl, src.ptr, pitch)
            assert list(rc) == [INVALID if n == 0 else SUCCESS for n in dl]
            for (s, i), p, n in zip(ent, pk, dl):
                if n:
                    assert r_dec[s].add_original(i, p) == 0
            elist = [s for s in range(n_streams) for _ in range(n_rec)]
            rec.fill()
            nb, rc = bc.encode(elist, rec.ptr, pitch)
            assert list(rc) == [0] * len(elist)
            rl = [0 if lost_r[s, t * n_rec + (j % n_rec)] else int(n) for j, (s, n) in enumerate(zip(elist, nb))]
            rc = bc.decoder_add_recovery(elist, rl, rec.ptr, pitch)
            ref_rc = []
            for s, n in zip(elist, rl):
                erc, data = r_enc[s].encode()
                assert erc == 0
                ref_rc.append(r_dec[s].add_recovery(data) if n else INVALID)
            assert list(rc) == ref_rc, t
            out.fill()
            rc, o_s, o_n, o_b = bc.decode(list(range(n_streams)), out.ptr, pitch, 64)
            raw = out.download()
            for j in range(len(o_s)):
                got_all.append((t, int(o_s[j]), int(o_n[j]), raw[j * pitch:j * pitch + int(o_b[j])].tobytes()))
            for s in range(n_streams):
                wrc, wp = r_dec[s].decode_if_ready()
                assert rc[s] == wrc, (t, s)
                want_all += [(t, s, num, data) for num, data in wp]
            check_all(src, rec, out)
            if t % 2 == 1:
                for s in range(n_streams):
                    arc, ack = bc.decoder_ack(s)
                    assert (arc, ack) == r_dec[s].ack()
                    assert bc.encoder_ack(s, ack) == r_enc[s].ack(ack)
        assert got_all == want_all
        assert len(want_all) >= 30 and all(d == pay[s][num] for _, s, num, d in want_all)
    finally:
        bc.close()
        for x in r_enc + r_dec:
            x.close()


def test_refusals(hip):
    import tonk_amd
    pitch = 1311
    bc = new_codec(2, 1300, 32 << 20)
    refs = [RefEncoder(), RefEncoder()]
    ref_dec = RefDecoder()
    rng = np.random.default_rng(3)
    pk = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (700, 700, 700, 1300, 33, 700, 700, 700)]
    src, out = Guarded(hip, 8 * pitch, 3), Guarded(hip, 8 * pitch, 0)
    try:
        src.upload(slots(pk, pitch))
        # len 0 and len = max + 1 between good neighbours of the same stretch
        lens = [700, 0, 700, 1301, 33, 700, 700, 700]
        pn, rc = bc.encoder_add([0] * 8, lens, src.ptr, pitch)
        assert list(rc) == [0, INVALID, 0, INVALID, 0, 0, 0, 0]
        good = [i for i in range(8) if rc[i] == 0]
        assert [int(pn[i]) for i in good] == list(range(6))
        for i in good:
            assert refs[0].add(pk[i])[0] == 0
        # refused as a whole, nothing changed: a stream id out of range, a pitch below the largest len
        with pytest.raises(RuntimeError, match="stream id out of range"):
            bc.encoder_add([0, 2], [700, 700], src.ptr, pitch)
        with pytest.raises(RuntimeError, match="pitch"):
            bc.encoder_add([0, 0], [700, 1300], src.ptr, 1299)
        with pytest.raises(RuntimeError, match="pitch"):
            bc.encode([0], out.ptr, 1310)
        with pytest.raises(RuntimeError, match="stream id out of range"):
            bc.encode([0, 7], out.ptr, pitch)
        check_all(src, out)
        out.fill()
        nb, rc = bc.encode([0, 0], out.ptr, pitch)
        want = [refs[0].encode(), refs[0].encode()]
        assert list(rc) == [0, 0] and recovery_slots(out, pitch, nb) == [w[1] for w in want]
        # a duplicate original; the receiver lacks originals 1 and 3 (pk[2] and pk[5]); nums -> their index in pk
        nums = [0, 2, 4, 5, 0]
        idx = [0, 4, 6, 7, 0]
        src.upload(slots([pk[i] for i in idx], pitch))
        rc = bc.decoder_add_original([1] * 5, nums, [len(pk[i]) for i in idx], src.ptr, pitch)
        assert list(rc) == [0, 0, 0, 0, DUPLICATE]
        assert [ref_dec.add_original(n, pk[i]) for n, i in zip(nums, idx)] == [0, 0, 0, 0, DUPLICATE]
        # two recovery packets recover two losses: cap 1 leaves the stream for the next call
        src.upload(slots([w[1] for w in want], pitch))
        rc = bc.decoder_add_recovery([1, 1], [len(w[1]) for w in want], src.ptr, pitch)
        assert list(rc) == [ref_dec.add_recovery(w[1]) for w in want] == [0, 0]
        out.fill()
        rc, o_s, o_n, o_b = bc.decode([0, 1], out.ptr, pitch, 1)
        assert list(rc) == [NEED_MORE, NEED_MORE] and len(o_s) == 0
        assert (out.download() == Guarded.FILL).all()
        rc, o_s, o_n, o_b = bc.decode([0, 1], out.ptr, pitch, 2)
        wrc, wp = ref_dec.decode_if_ready()
        assert list(rc) == [NEED_MORE, wrc] and wrc == 0
        assert [(int(n), int(b)) for n, b in zip(o_n, o_b)] == [(n, len(d)) for n, d in wp] == [(1, 700), (3, 700)]
        raw = out.download()
        for j, (n, d) in enumerate(wp):
            assert raw[j * pitch:j * pitch + len(d)].tobytes() == d
        with pytest.raises(RuntimeError, match="pitch"):
            bc.decode([1], out.ptr, 1299, 4)
        check_all(src, out)
        assert isinstance(bc, tonk_amd.BatchCodec)
    finally:
        bc.close()
        for x in refs + [ref_dec]:
            x.close()


@pytest.mark.parametrize("length", [100, 1300])
def test_damaged_recovery_packet(hip, length):
    """Byte 0 of stream 1's recovery packet is XORed with 0xFF on its way to both decoders: the
    recovered row's length header is wrong (length 100: it announces more than the row holds, the
    kernel's bounds check; 1300: a shorter packet of garbage).  Whatever the reference returns is
    expected; streams 0 and 2 of the same calls recover their packet."""
    pitch = length + OVER
    bc = new_codec(3, length, 32 << 20)
    encs = [RefEncoder() for _ in range(3)]
    decs = [RefDecoder() for _ in range(3)]
    pay = make_payloads(3, lambda s: [length] * 10, 11)
    src, out = Guarded(hip, 27 * pitch, 5), Guarded(hip, 8 * pitch, 6)
    try:
        recs = []
        for s in range(3):
            for p in pay[s]:
                assert encs[s].add(p)[0] == 0
            rc, data = encs[s].encode()
            assert rc == 0
            if s == 1:
                data = bytes([data[0] ^ 0xFF]) + data[1:]
            recs.append(data)
        ent = [(s, i) for s in range(3) for i in range(10) if i != 4]
        src.upload(slots([pay[s][i] for s, i in ent], pitch))
        rc = bc.decoder_add_original([e[0] for e in ent], [e[1] for e in ent], [length] * len(ent), src.ptr, pitch)
        assert list(rc) == [decs[s].add_original(i, pay[s][i]) for s, i in ent] == [0] * len(ent)
        src.upload(slots(recs, pitch))
        rc = bc.decoder_add_recovery([0, 1, 2], [len(d) for d in recs], src.ptr, pitch)
        assert list(rc) == [decs[s].add_recovery(recs[s]) for s in range(3)]
        check_all(src, out)
        flat = decode_and_compare(bc, decs, out, pitch, 8, f"damaged, length {length}")
        assert [f[:2] for f in flat if f[0] != 1] == [(0, 4), (2, 4)]
        assert all(f[2] == pay[f[0]][4] for f in flat if f[0] != 1)
        check_all(src, out)
        # afterwards the three streams answer as the reference's do
        assert [bc.decoder_ack(s)[0] for s in range(3)] == [decs[s].ack()[0] for s in range(3)]
    finally:
        bc.close()
        for x in encs + decs:
            x.close()


def test_full_arena_disables_one_stream(hip):
    """A stream whose share of the arena is full is disabled (result 5 for the packets that did not
    fit and for every later call on it), as a codec of the C ABI is; its neighbour goes on and still
    equals the reference."""
    share = 88 << 10  # 65 rows of a 1300-byte original
    bc = new_codec(2, 1300, 2 * share)
    ref = RefEncoder()
    rng = np.random.default_rng(17)
    pk = [rng.integers(0, 256, 1300, dtype=np.uint8).tobytes() for _ in range(64)]
    src, out = Guarded(hip, 64 * 1300, 1), Guarded(hip, 2 * 1311, 2)
    try:
        src.upload(slots(pk, 1300))
        pn, rc = bc.encoder_add([0] * 64, [1300] * 64, src.ptr, 1300)
        assert list(rc) == [SUCCESS] * 64 and list(pn) == list(range(64))
        pn, rc = bc.encoder_add([0] * 64, [1300] * 64, src.ptr, 1300)
        assert list(rc) == [DISABLED] * 64
        pn, rc = bc.encoder_add([0, 1, 0, 1], [1300] * 4, src.ptr, 1300)
        assert list(rc) == [DISABLED, SUCCESS, DISABLED, SUCCESS] and [int(pn[1]), int(pn[3])] == [0, 1]
        assert ref.add(pk[1]) == (0, 0) and ref.add(pk[3]) == (0, 1)
        out.fill()
        nb, rc = bc.encode([0, 1], out.ptr, 1311)
        want = ref.encode()
        assert list(rc) == [DISABLED, want[0]] and list(nb) == [0, len(want[1])]
        raw = out.download()
        assert (raw[:1311] == Guarded.FILL).all() and raw[1311:1311 + nb[1]].tobytes() == want[1]
        check_all(src, out)
    finally:
        bc.close()
        ref.close()


# ---- reordering, duplicates and stale acknowledgements ----

IMP_ORIG, IMP_TICK, IMP_REC = 96, 8, 2


def impaired_lengths(s):
    """1300 for even streams, LENS18 rotated for odd ones."""
    return [1300] * IMP_ORIG if s % 2 == 0 else ((LENS18[s % 18:] + LENS18[:s % 18]) * 6)[:IMP_ORIG]


_scripts = {}


def impaired_decoder_script(n_streams):
    """The reference's side of test_decoder_under_impairment, computed once per stream count: the
    calls of a seeded delivery plan in order, each with what RefDecoder returned.  5 % of the
    originals are lost; 25 % of the delivered packets of either kind are held for 1-3 ticks; 10 %
    are delivered twice (the second copy 0-2 ticks after the first); stream 0's whole first tick of
    originals is held, so its first recovery packet meets an empty decoder.  The senders
    (RefEncoder) get their receiver's acknowledgement every third tick.
    Steps: ("orig", [(stream, num, payload)], rcs), ("rec", [(stream, packet)], rcs),
    ("decode", [(rc, [(num, payload)])] per stream), ("ack", [(rc, bytes)] per stream)."""
    if n_streams in _scripts:
        return _scripts[n_streams]
    rng = np.random.default_rng(4100 + n_streams)
    pay = make_payloads(n_streams, impaired_lengths, 21)
    encs = [RefEncoder() for _ in range(n_streams)]
    decs = [RefDecoder() for _ in range(n_streams)]
    n_ticks = IMP_ORIG // IMP_TICK
    arrive_o = [[] for _ in range(n_ticks + 8)]
    arrive_r = [[] for _ in range(n_ticks + 8)]
    steps, stats = [], {"duplicate": 0, "recovered": 0, "behind": 0, "late_originals": 0}
    newest = [-1] * n_streams  # encode sequence of the newest recovery packet delivered
    n_encoded = [0] * n_streams

    def fate(force_hold=False, never_hold=False):
        u = rng.random(5)
        hold = 1 + int(u[2] * 3) if u[1] < 0.25 else 0
        if force_hold:
            hold = max(hold, 1)
        if never_hold:
            hold = 0
        return u[0] < 0.05, hold, (hold + int(u[4] * 3) if u[3] < 0.10 else None)

    def decode_step():
        want = [d.decode_if_ready() for d in decs]
        stats["recovered"] += sum(len(w[1]) for w in want)
        steps.append(("decode", want))

    def deliver(t):
        if arrive_o[t]:
            ent = arrive_o[t]
            rcs = [decs[s].add_original(i, pay[s][i]) for s, i in ent]
            stats["duplicate"] += rcs.count(DUPLICATE)
            steps.append(("orig", [(s, i, pay[s][i]) for s, i in ent], rcs))
            decode_step()
        if arrive_r[t]:
            ent = arrive_r[t]
            rcs = []
            for s, seq, data in ent:
                if seq < newest[s]:
                    stats["behind"] += 1
                newest[s] = max(newest[s], seq)
                rcs.append(decs[s].add_recovery(data))
            steps.append(("rec", [(s, data) for s, _, data in ent], rcs))
            decode_step()
        acks = [d.ack() for d in decs]
        steps.append(("ack", acks))
        if t % 3 == 2:
            for s, (arc, ack) in enumerate(acks):
                if arc == 0 and ack:
                    assert encs[s].ack(ack)[0] == 0

    def send_recovery(s, t, in_order):
        rc, data = encs[s].encode()
        _, hold, dup = fate(never_hold=in_order)
        if rc != 0:  # (everything acknowledged: the sender has nothing to protect)
            assert rc == NEED_MORE and t >= n_ticks
            return
        arrive_r[t + hold].append((s, n_encoded[s], data))
        if dup is not None and not in_order:
            arrive_r[t + dup].append((s, n_encoded[s], data))
        n_encoded[s] += 1

    for t in range(n_ticks):
        for k in range(IMP_TICK):
            for s in range(n_streams):
                i = t * IMP_TICK + k
                assert encs[s].add(pay[s][i]) == (0, i)
                lost, hold, dup = fate(force_hold=(s == 0 and t == 0))
                if lost:
                    continue
                stats["late_originals"] += hold > 0
                arrive_o[t + hold].append((s, i))
                if dup is not None:
                    arrive_o[t + dup].append((s, i))
        for s in range(n_streams):
            for _ in range(IMP_REC):
                send_recovery(s, t, in_order=(s == 0 and t == 0))
        deliver(t)
    for t in range(n_ticks, n_ticks + 6):  # what is still held, then recovery packets in order
        for s in range(n_streams):
            for _ in range(IMP_REC):
                send_recovery(s, t, in_order=True)
        deliver(t)
    for x in encs + decs:
        x.close()
    _scripts[n_streams] = (steps, stats)
    return _scripts[n_streams]


class Recorded:
    """A RefDecoder's recorded answer, for decode_and_compare."""

    def __init__(self, result):
        self.result = result

    def decode_if_ready(self):
        return self.result


@pytest.mark.parametrize("n_streams", [3, 8])
def test_decoder_under_impairment(hip, n_streams):
    """The batched decoder at 3 and at 8 streams (the two configurations of tamd_batch_create: back
    substitution over materialized rows and short scans up to 4 streams, split dense ranges above)
    under reordering and duplication: every decoder_add_original, decoder_add_recovery, decode and
    decoder_ack equals RefDecoder's, call by call, recovered payloads byte for byte."""
    steps, stats = impaired_decoder_script(n_streams)
    # (from the reference's returns: the comparison is not vacuous)
    assert stats["duplicate"] >= 1 and stats["recovered"] >= 10 and stats["behind"] >= 1 and stats["late_originals"] >= 1
    pitch = 4001
    rec_pitch = pitch + OVER
    most_o = max(len(st[1]) for st in steps if st[0] == "orig")
    most_r = max(len(st[1]) for st in steps if st[0] == "rec")
    bc = new_codec(n_streams, MAXB, n_streams * (32 << 20))
    src = Guarded(hip, most_o * pitch, 1)
    rec = Guarded(hip, most_r * rec_pitch, 2)
    out = Guarded(hip, 64 * pitch, 7)
    try:
        for n, st in enumerate(steps):
            if st[0] == "orig":
                ent = st[1]
                src.upload(slots([e[2] for e in ent], pitch))
                rc = bc.decoder_add_original([e[0] for e in ent], [e[1] for e in ent], [len(e[2]) for e in ent], src.ptr, pitch)
                assert list(rc) == st[2], f"step {n}"
            elif st[0] == "rec":
                ent = st[1]
                rec.upload(slots([e[1] for e in ent], rec_pitch))
                rc = bc.decoder_add_recovery([e[0] for e in ent], [len(e[1]) for e in ent], rec.ptr, rec_pitch)
                assert list(rc) == st[2], f"step {n}"
            elif st[0] == "decode":
                decode_and_compare(bc, [Recorded(w) for w in st[1]], out, pitch, 64, f"step {n}")
            else:
                assert [bc.decoder_ack(s) for s in range(n_streams)] == st[1], f"step {n}"
            check_all(src, rec, out)
    finally:
        bc.close()


def test_encoder_under_impairment(hip):
    """One batched encoder per stream beside a RefEncoder, fed the same originals and the same
    acknowledgements out of a seeded plan: 30 % dropped, 30 % held for one or two ticks (delivered
    oldest-due first, so a held one arrives after a newer one: the stale acknowledgement), 20 %
    delivered twice in succession.  The acknowledgements are a RefDecoder's that lost 5 % of the
    originals.  encoder_ack's results and the bytes of every later encode must be equal."""
    n_streams, pitch = 2, 4001
    out_pitch = pitch + OVER
    rng = np.random.default_rng(77)
    pay = make_payloads(n_streams, impaired_lengths, 31)
    bc = new_codec(n_streams, MAXB, 64 << 20)
    encs = [RefEncoder() for _ in range(n_streams)]
    decs = [RefDecoder() for _ in range(n_streams)]
    src = Guarded(hip, n_streams * IMP_TICK * pitch, 3)
    out = Guarded(hip, n_streams * IMP_REC * out_pitch, 5)
    pending, newest = [], [-1] * n_streams
    dropped = stale = repeated = 0
    try:
        for t in range(IMP_ORIG // IMP_TICK):
            ent = [(s, t * IMP_TICK + k) for k in range(IMP_TICK) for s in range(n_streams)]
            pk = [pay[s][i] for s, i in ent]
            src.upload(slots(pk, pitch))
            pn, rc = bc.encoder_add([e[0] for e in ent], [len(p) for p in pk], src.ptr, pitch)
            want = [encs[s].add(p) for (s, _), p in zip(ent, pk)]
            assert list(rc) == [w[0] for w in want] and list(pn) == [w[1] for w in want], t
            elist = [s for s in range(n_streams) for _ in range(IMP_REC)]
            out.fill()
            nb, rc = bc.encode(elist, out.ptr, out_pitch)
            want = [encs[s].encode() for s in elist]
            assert list(rc) == [w[0] for w in want] == [0] * len(elist), t
            assert list(nb) == [len(w[1]) for w in want], t
            for j, (g, w) in enumerate(zip(recovery_slots(out, out_pitch, nb), want)):
                assert g == w[1], f"tick {t}: recovery packet {j} (stream {elist[j]}) differs"
            check_all(src, out)
            # the receivers (reference only), and their acknowledgements' way back
            for (s, i), p in zip(ent, pk):
                if rng.random() >= 0.05:
                    assert decs[s].add_original(i, p) == 0
            for s, w in zip(elist, want):
                assert decs[s].add_recovery(w[1]) == 0
            for d in decs:
                d.decode_if_ready()
            for s in range(n_streams):
                arc, ack = decs[s].ack()
                u = rng.random(4)
                if arc != 0 or not ack:
                    continue
                if u[0] < 0.30:
                    dropped += 1
                    continue
                hold = 1 + int(u[2] * 2) if u[1] < 0.30 else 0
                pending.append((t + hold, t, s, ack, bool(u[3] < 0.20)))
            due = sorted(x for x in pending if x[0] <= t)
            pending = [x for x in pending if x[0] > t]
            for _, seq, s, ack, twice in due:
                if seq < newest[s]:
                    stale += 1
                newest[s] = max(newest[s], seq)
                for _ in range(2 if twice else 1):
                    assert bc.encoder_ack(s, ack) == encs[s].ack(ack), (t, s, seq)
                repeated += twice
        assert dropped >= 1 and stale >= 1 and repeated >= 1
    finally:
        bc.close()
        for x in encs + decs:
            x.close()


# ---- packets above 4096 bytes: two and four waves per packet, the 3-byte length header ----

LONG_MAXB = 65535
LONG_LENS = [1, 4093, 4094, 4097, 9000, 16381, 16382, 16383, 16384, 16385, 40000, 65534, 65535]
LONG_ORIG = 36
STREAM_ARENA = 64 << 20  # a stream's share: no codec disables itself for lack of rows
# (payload slots, recovery slots): odd and minimal, then a multiple of 64 that holds either
LONG_PITCHES = [(LONG_MAXB, LONG_MAXB + OVER), (65600, 65600)]


def waves_per_packet(largest):
    """batch.cpp Batch::waves_per_packet (frame.h tamd_frame_waves), restated:
    `bytes <= 4096u ? 1u : bytes <= 16384u ? 2u : 4u`."""
    return 1 if largest <= 4096 else 2 if largest <= 16384 else 4


def add_waves(lens):
    """An add call's shape (batch.cpp add_packets: `b->frame(nd, largest + 3)`)."""
    return waves_per_packet(max(lens) + 3)


def packet_waves(nbytes):
    """The shape of an encode's output and of add_recovery (batch.cpp: the largest `o.total()`,
    `largest_within(bytes, n, maxb)`): by the largest recovery packet as it is."""
    return waves_per_packet(max(nbytes))


def size_class(n):
    """0: one wave when added (n + 3 <= 4096), 1: two waves, 2: four (n + 3 > 16384)."""
    return add_waves([n]).bit_length() - 1


def long_lengths(s):
    rot = LONG_LENS[4 * s % 13:] + LONG_LENS[:4 * s % 13]
    return (rot * 3)[:LONG_ORIG]


def lost_long(s, i):
    """Three sizes of each stream's first pass through LONG_LENS and three of its second: one or more of
    every size class, 16384 and 65535 (3-byte headers) among them."""
    return long_lengths(s)[i] in ((4093, 9000, 16384), (1, 16381, 65535), ())[i // 13]


@pytest.fixture(scope="module")
def long_payloads():
    return make_payloads(N_STREAMS, long_lengths, 8)


_long_script = []


def long_decoder_script(long_payloads):
    """The reference's side of test_decoder_matches_reference_on_long_packets, computed once on the
    CPU: the reference encoders' traffic delivered round by round without the originals of
    lost_long, each call with what RefDecoder returned (steps as in impaired_decoder_script), and
    the originals the reference decoders recovered, (stream, number, bytes)."""
    if not _long_script:
        decs = [RefDecoder() for _ in range(N_STREAMS)]
        steps, recovered = [], []

        def decode_step():
            want = [d.decode_if_ready() for d in decs]
            recovered.extend((s, num, len(data)) for s, w in enumerate(want) for num, data in w[1])
            steps.append(("decode", want))

        for r, recs in enumerate(reference_traffic(long_payloads, LONG_ORIG)):
            if r < LONG_ORIG // PER_CALL:
                ent = [(s, r * PER_CALL + k) for k in range(PER_CALL) for s in range(N_STREAMS) if not lost_long(s, r * PER_CALL + k)]
                rcs = [decs[s].add_original(i, long_payloads[s][i]) for s, i in ent]
                assert rcs == [SUCCESS] * len(ent)
                steps.append(("orig", [(s, i, long_payloads[s][i]) for s, i in ent], rcs))
                decode_step()
            steps.append(("rec", recs, [decs[s].add_recovery(d) for s, d in recs]))
            decode_step()
            steps.append(("ack", [d.ack() for d in decs]))
        for d in decs:
            d.close()
        _long_script.append((steps, recovered))
    return _long_script[0]


@pytest.mark.parametrize("skew", [0, 5])
@pytest.mark.parametrize("pitch,out_pitch", LONG_PITCHES)
def test_encoder_matches_reference_on_long_packets(hip, long_payloads, pitch, out_pitch, skew):
    """test_encoder_matches_reference at max_packet_bytes 65535 over LONG_LENS: every add call and
    every encode runs four waves per packet (asserted from the call's sizes), short packets beside
    long ones in every call."""
    bc = new_codec(N_STREAMS, LONG_MAXB, N_STREAMS * STREAM_ARENA)
    refs = [RefEncoder() for _ in range(N_STREAMS)]
    ref_dec = [RefDecoder() for _ in range(N_STREAMS)]
    src = Guarded(hip, N_STREAMS * PER_CALL * pitch, skew)
    out = Guarded(hip, len(ENCODE_LIST) * out_pitch, skew)
    try:
        for r in range(LONG_ORIG // PER_CALL):
            stream = [s for k in range(PER_CALL) for s in range(N_STREAMS)]
            index = [r * PER_CALL + k for k in range(PER_CALL) for s in range(N_STREAMS)]
            pk = [long_payloads[s][i] for s, i in zip(stream, index)]
            assert add_waves([len(p) for p in pk]) == 4 and min(len(p) for p in pk) <= 4093
            src.upload(slots(pk, pitch))
            pn, rc = bc.encoder_add(stream, [len(p) for p in pk], src.ptr, pitch)
            want = [refs[s].add(p) for s, p in zip(stream, pk)]
            assert [w[0] for w in want] == [SUCCESS] * len(pk)
            assert list(rc) == [w[0] for w in want] and list(pn) == [w[1] for w in want]
            check_all(src, out)
            out.fill()
            nb, rc = bc.encode(ENCODE_LIST, out.ptr, out_pitch)
            want = [refs[s].encode() for s in ENCODE_LIST]
            assert [w[0] for w in want] == [SUCCESS] * len(want)
            assert list(rc) == [w[0] for w in want], r
            assert list(nb) == [len(w[1]) for w in want], r
            assert packet_waves(nb) == 4 and (r == 0 or max(nb) > LONG_MAXB)
            got = recovery_slots(out, out_pitch, nb)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w[1], f"round {r} recovery packet {i} (stream {ENCODE_LIST[i]}) differs"
            check_all(src, out)
            for s, w in zip(ENCODE_LIST, want):
                assert ref_dec[s].add_recovery(w[1]) == 0
            for s in range(N_STREAMS):
                for k in range(PER_CALL):
                    i = r * PER_CALL + k
                    if i not in (5, 20):
                        assert ref_dec[s].add_original(i, long_payloads[s][i]) == 0
            if r == 1:  # after the second add call: the receivers' acknowledgements
                for s in range(N_STREAMS):
                    arc, ack = ref_dec[s].ack()
                    assert arc == 0 and ack
                    assert bc.encoder_ack(s, ack) == refs[s].ack(ack)
    finally:
        bc.close()
        for x in refs + ref_dec:
            x.close()


def replay_decoder_script(hip, bc, steps, n_streams, pitch, rec_pitch, skew, cap):
    """The calls of a decoder script on the handle, each against the reference's recorded answer."""
    most_o = max(len(st[1]) for st in steps if st[0] == "orig")
    most_r = max(len(st[1]) for st in steps if st[0] == "rec")
    src, rec, out = Guarded(hip, most_o * pitch, skew), Guarded(hip, most_r * rec_pitch, skew), Guarded(hip, cap * pitch, skew)
    for n, st in enumerate(steps):
        if st[0] == "orig":
            ent = st[1]
            src.upload(slots([e[2] for e in ent], pitch))
            rc = bc.decoder_add_original([e[0] for e in ent], [e[1] for e in ent], [len(e[2]) for e in ent], src.ptr, pitch)
            assert list(rc) == st[2], f"step {n}"
        elif st[0] == "rec":
            ent = st[1]
            rec.upload(slots([e[1] for e in ent], rec_pitch))
            rc = bc.decoder_add_recovery([e[0] for e in ent], [len(e[1]) for e in ent], rec.ptr, rec_pitch)
            assert list(rc) == st[2], f"step {n}"
        elif st[0] == "decode":
            decode_and_compare(bc, [Recorded(w) for w in st[1]], out, pitch, cap, f"step {n}")
        else:
            assert [bc.decoder_ack(s) for s in range(n_streams)] == st[1], f"step {n}"
        check_all(src, rec, out)


@pytest.mark.parametrize("skew", [0, 5])
@pytest.mark.parametrize("pitch,rec_pitch", LONG_PITCHES)
def test_decoder_matches_reference_on_long_packets(hip, long_payloads, pitch, rec_pitch, skew):
    """test_decoder_matches_reference at max_packet_bytes 65535 over LONG_LENS.  The reference
    decoders alone (long_decoder_script, on the CPU) recover originals of every size class -- one
    wave when added, two, four -- and of 16384 bytes and more, whose 3-byte length header the
    unframing kernel reads back; the handle must return the same packets byte for byte."""
    steps, recovered = long_decoder_script(long_payloads)
    sizes = [n for _, _, n in recovered]
    assert {size_class(n) for n in sizes} == {0, 1, 2} and max(sizes) >= 16384 and len(sizes) >= 12, sorted(sizes)
    assert min(sizes) <= 4093 and any(4094 <= n <= 16381 for n in sizes) and any(n >= 16382 for n in sizes)
    for s in range(N_STREAMS):
        assert {size_class(n) for t, _, n in recovered if t == s} == {0, 1, 2}, s
    assert all(rc == SUCCESS for st in steps if st[0] in ("orig", "rec") for rc in st[2])
    for st in steps:  # every add call of either kind runs four waves per packet, short packets among them
        if st[0] == "orig":
            assert add_waves([len(e[2]) for e in st[1]]) == 4 and min(len(e[2]) for e in st[1]) <= 4093
        elif st[0] == "rec":
            assert packet_waves([len(e[1]) for e in st[1]]) == 4
    bc = new_codec(N_STREAMS, LONG_MAXB, N_STREAMS * STREAM_ARENA)
    try:
        replay_decoder_script(hip, bc, steps, N_STREAMS, pitch, rec_pitch, skew, 16)
    finally:
        bc.close()


class ShapeRig:
    """One handle of max_packet_bytes 65535 beside a reference encoder and decoder per stream, for
    single calls of a chosen launch shape."""
    PITCH, REC_PITCH = LONG_MAXB, LONG_MAXB + OVER

    def __init__(self, hip, n_streams, most_packets):
        self.n = n_streams
        self.bc = new_codec(n_streams, LONG_MAXB, n_streams * STREAM_ARENA)
        self.encs = [RefEncoder() for _ in range(n_streams)]
        self.decs = [RefDecoder() for _ in range(n_streams)]
        self.src = Guarded(hip, most_packets * self.PITCH, 3)
        self.rec = Guarded(hip, n_streams * self.REC_PITCH, 1)
        self.out = Guarded(hip, n_streams * self.PITCH, 7)

    def call(self, packets, withheld, ack=False):
        """`packets` [(stream, payload)] added in one call and one recovery packet encoded for every
        stream, both compared with the reference; then the decoder round: the packets but those at
        the list indices `withheld` (at most one of a stream) and the recovery packets are added,
        and decode must return the withheld ones.  With `ack` the decoders' acknowledgements go to
        the encoders, whose windows then start behind this call's packets.  Returns the waves per
        packet of the add call and of the recovery packets."""
        bc, src, rec, out = self.bc, self.src, self.rec, self.out
        bufs = (src, rec, out)
        streams, lens = [s for s, _ in packets], [len(p) for _, p in packets]
        src.upload(slots([p for _, p in packets], self.PITCH))
        pn, rc = bc.encoder_add(streams, lens, src.ptr, self.PITCH)
        want = [self.encs[s].add(p) for s, p in packets]
        assert [w[0] for w in want] == [SUCCESS] * len(packets)
        assert list(rc) == [w[0] for w in want] and list(pn) == [w[1] for w in want]
        check_all(*bufs)
        elist = list(range(self.n))
        rec.fill()
        nb, rc = bc.encode(elist, rec.ptr, self.REC_PITCH)
        want_rec = [self.encs[s].encode() for s in elist]
        assert [w[0] for w in want_rec] == [SUCCESS] * self.n
        assert list(rc) == [w[0] for w in want_rec] and list(nb) == [len(w[1]) for w in want_rec]
        assert recovery_slots(rec, self.REC_PITCH, nb) == [w[1] for w in want_rec]
        check_all(*bufs)
        # the receivers: what was not withheld, then the recovery packets out of the encode's own buffer
        kept = [i for i in range(len(packets)) if i not in withheld]
        if kept:
            src.upload(slots([packets[i][1] for i in kept], self.PITCH))
            ks, kn = [streams[i] for i in kept], [int(pn[i]) for i in kept]
            rc = bc.decoder_add_original(ks, kn, [lens[i] for i in kept], src.ptr, self.PITCH)
            assert list(rc) == [self.decs[s].add_original(n, packets[i][1]) for s, n, i in zip(ks, kn, kept)] == [SUCCESS] * len(kept)
            check_all(*bufs)
            assert decode_and_compare(bc, self.decs, out, self.PITCH, self.n, "originals") == []
        rc = bc.decoder_add_recovery(elist, [int(x) for x in nb], rec.ptr, self.REC_PITCH)
        assert list(rc) == [self.decs[s].add_recovery(want_rec[s][1]) for s in elist] == [SUCCESS] * self.n
        check_all(*bufs)
        flat = decode_and_compare(bc, self.decs, out, self.PITCH, self.n, "recovery")
        assert flat == sorted((streams[i], int(pn[i]), packets[i][1]) for i in withheld), "the withheld packets did not come back"
        check_all(*bufs)
        if ack:
            for s in elist:
                arc, a = self.decs[s].ack()
                assert arc == 0 and a and bc.decoder_ack(s) == (arc, a)
                assert bc.encoder_ack(s, a) == self.encs[s].ack(a)
        return add_waves(lens), packet_waves(nb)

    def close(self):
        self.bc.close()
        for x in self.encs + self.decs:
            x.close()


def random_packets(seed, spec):
    """spec [(stream, bytes)] -> [(stream, payload)]"""
    rng = np.random.default_rng(seed)
    return [(s, rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for s, n in spec]


@pytest.mark.parametrize("length,n,waves", [(9000, 1, 2), (9000, 3, 2), (9000, 5, 2), (16384, 1, 4), (16384, 3, 4), (65535, 1, 4),
                                            (65535, 3, 4)])
def test_launch_shapes_of_equally_long_packets(hip, length, n, waves):
    """One stream, one call of n equally long packets: two waves per packet at 9000 bytes (n = 1, 3
    and 5 fill half a workgroup, one and a half, two and a half), four at 16384 and 65535; from two
    packets on they are added as a run.  The middle packet is withheld and recovered."""
    rig = ShapeRig(hip, 1, n)
    try:
        assert rig.call(random_packets(length + n, [(0, length)] * n), {n // 2}) == (waves, waves)
    finally:
        rig.close()


def test_short_and_long_packets_in_one_call(hip):
    """1-byte, 17-byte and 65535-byte packets of two streams in one call: the short ones run under the
    256 lanes of the long ones.  Stream 0 loses its 1-byte packet, stream 1 its longest."""
    rig = ShapeRig(hip, 2, 6)
    try:
        spec = [(0, 1), (1, 17), (0, 65535), (1, 1), (0, 17), (1, 65535)]
        assert rig.call(random_packets(61, spec), {0, 5}) == (4, 4)
    finally:
        rig.close()


def test_launch_shape_changes_between_calls_of_one_handle(hip):
    """Short packets only, then long ones, then short ones again on one handle: one wave per packet,
    four, one -- in the add calls and, the windows acknowledged in between, in the recovery packets."""
    rig = ShapeRig(hip, 2, 4)
    try:
        short = [(0, 100), (1, 1), (0, 17), (1, 1300)]
        shapes = [rig.call(random_packets(62, short), {2, 3}, ack=True),
                  rig.call(random_packets(63, [(0, 65535), (1, 40000), (0, 65535), (1, 16382)]), {0, 1}, ack=True),
                  rig.call(random_packets(64, short), {0, 1}, ack=True)]
        assert shapes == [(1, 1), (4, 4), (1, 1)]
    finally:
        rig.close()
