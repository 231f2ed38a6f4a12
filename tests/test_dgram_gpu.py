"""Building and parsing of datagrams in device memory (include/tonk_datagram.h,
tonk_amd.DatagramFramer) on an MI355X against the recorded results of the reference
(tests/golden/dgram_kat.txt.gz) and, for shapes beyond the fixture, against its Python restatement
(tests/dgram_ref.py, itself checked against the fixture by tests/test_dgram.py); the offset forms
of the codec's add calls; and the whole datagram path -- build, encode, seal, loss, open, parse,
decode -- joined on the device.  Every caller buffer has 64 guard bytes of 0xA5 on each side,
checked after every call, and the gaps between the slots of a call are compared too: no byte
outside what a call may write changes."""
from __future__ import annotations

import numpy as np
import pytest

import dgram_ref as R
from batch_ref import LENGTHS, Guarded
from lz_streams import Hip

pytestmark = [pytest.mark.gpu]

MAXB = 65535
FILL = Guarded.FILL
SKEWS = (0, 1, 5, 15)
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def framer():
    import tonk_amd
    f = tonk_amd.DatagramFramer(MAXB)
    yield f
    f.close()


def layout(items, pitch, offsets=None):
    """The items' bytes at i * pitch (+ offsets[i]), 0xA5 in the gaps."""
    out = np.full(max(len(items) * pitch, 1), FILL, dtype=np.uint8)
    for i, d in enumerate(items):
        at = i * pitch + (offsets[i] if offsets is not None else 0)
        out[at:at + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
    return out


def differing(got, want, pitch):
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    i, o = divmod(int(bad[0]), pitch)
    return f"slot {i}: {R.first_difference(got[i * pitch:(i + 1) * pitch], want[i * pitch:(i + 1) * pitch])} (offset {o})"


class Sources:
    """Message bodies scattered in one guarded device buffer, body k at an address whose low four
    bits are (first + k) & 15, 0xA5 between them."""

    def __init__(self, hip, bodies, skew=0, first=0):
        total = sum(len(b) + 32 for b in bodies) + 64
        self.buf = Guarded(hip, total, skew)
        self.image = np.full(total, FILL, dtype=np.uint8)
        self.addr, at = [], 0
        for k, b in enumerate(bodies):
            at += ((first + k) - (self.buf.ptr + at)) & 15
            self.addr.append(self.buf.ptr + at)
            self.image[at:at + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
            at += len(b) + 1
        self.buf.upload(self.image)

    def check(self):
        self.buf.check()
        assert (self.buf.download() == self.image).all(), "a source buffer was written"


def build_call(framer, datagrams, srcs, dev_out, pitch):
    """`datagrams`: dicts(msgs [(type, bytes)], seq, seq_bytes, nonce, nonce_bytes, handshake (12 bytes
    or None), ts24, flag_bits); srcs: the device address of every message body in order (0: zeros)."""
    dg = [i for i, d in enumerate(datagrams) for _ in d["msgs"]]
    mt = [t for d in datagrams for t, _ in d["msgs"]]
    mb = [n for d in datagrams for _, n in d["msgs"]]
    hs = np.zeros((len(datagrams), 12), dtype=np.uint8)
    for i, d in enumerate(datagrams):
        if d["handshake"] is not None:
            hs[i] = np.frombuffer(d["handshake"], dtype=np.uint8)
    return framer.build(dg, mt, mb, srcs, [d["seq"] for d in datagrams], [d["seq_bytes"] for d in datagrams],
                        [d["nonce"] for d in datagrams], [d["nonce_bytes"] for d in datagrams], [d["ts24"] for d in datagrams],
                        [d["flag_bits"] for d in datagrams], dev_out, pitch, handshake=hs,
                        has_handshake=[d["handshake"] is not None for d in datagrams])


# ---- 1. build against the reference ----

@pytest.fixture(scope="module")
def b_cases():
    """The B lines in two groups (so that a call's slots stay small): per group the lines, their
    inputs as drawn, and the expected datagrams, whose FNV is the fixture's."""
    groups = []
    for pick in (lambda n: n <= 6000, lambda n: n > 6000):
        lines = [b for b in R.kat()["B"] if pick(b["out_bytes"])]
        inputs, want = [], []
        for b in lines:
            rc, out, msg, lo, n = R.b_build(b)
            assert rc == 0 and R.fnv1a(out) == b["fnv"]
            inputs.append(R.b_inputs(b))
            want.append(out)
        groups.append((lines, inputs, want))
    assert sum(len(g[0]) for g in groups) == len(R.kat()["B"]) and all(g[0] for g in groups)
    return groups


@pytest.mark.parametrize("skew", SKEWS)
def test_build_equals_the_reference(hip, framer, b_cases, skew):
    """Every B line: one call per group at pitch largest + 11, the destination's base misaligned by
    `skew`, the bodies scattered at all 16 alignments, Padding bodies given as address 0."""
    for lines, inputs, want in b_cases:
        pitch = max(b["out_bytes"] for b in lines) + 11
        bodies = [body for i in inputs for _, body, _ in i["msgs"] if body is not None]
        src = Sources(hip, bodies, skew=(skew * 7) & 15, first=skew)
        it = iter(src.addr)
        srcs = [0 if body is None else next(it) for i in inputs for _, body, _ in i["msgs"]]
        datagrams = [dict(msgs=b["msgs"], seq=i["seq"], seq_bytes=b["seq_bytes"], nonce=i["nonce"], nonce_bytes=b["nonce_bytes"],
                          handshake=i["handshake"], ts24=i["ts24"], flag_bits=b["flag_bits"] | 0x8F) for b, i in zip(lines, inputs)]
        out = Guarded(hip, len(lines) * pitch, skew)
        ob, mb, ro, rb, rc = build_call(framer, datagrams, srcs, out.ptr, pitch)
        assert (rc == 0).all(), f"refused: {np.flatnonzero(rc)[:5]}"
        for name, got in (("out_bytes", ob), ("message_bytes", mb), ("reliable_offset", ro), ("reliable_bytes", rb)):
            bad = [i for i, b in enumerate(lines) if int(got[i]) != b[name]]
            assert not bad, f"{name} of line {lines[bad[0]]['seed']}: {int(got[bad[0]])}"
        out.check()
        msg = differing(out.download(), layout(want, pitch), pitch)
        assert not msg, f"build, base misalignment {skew}: {msg}"
        src.check()


def test_invalid_datagrams_leave_their_slot_and_refused_calls_do_nothing(hip):
    import tonk_amd
    framer = tonk_amd.DatagramFramer(100)
    try:
        rng = np.random.default_rng(3)
        ok = dict(msgs=[(6, 20), (7, 0)], seq=0x123456, seq_bytes=2, nonce=0xABCDEF, nonce_bytes=3, handshake=None, ts24=0x010203,
                  flag_bits=R.SEQCOMP)
        cases = [("type above 31", dict(ok, msgs=[(32, 5)])), ("bytes above 2047", dict(ok, msgs=[(6, 2048)])),
                 ("total above max_datagram_bytes", dict(ok, msgs=[(6, 45), (6, 45)])),
                 ("reliable without seq_bytes", dict(ok, seq_bytes=0)), ("reliable before unreliable", dict(ok, msgs=[(6, 5), (3, 5)])),
                 ("reliable behind Padding behind reliable", dict(ok, msgs=[(6, 5), (4, 5), (6, 1)])),
                 ("OnlyFEC with a sequence number", dict(ok, msgs=[(R.RAW, 30)], flag_bits=R.ONLYFEC)),
                 ("raw outside OnlyFEC", dict(ok, msgs=[(R.RAW, 30)])), ("seq_bytes 4", dict(ok, seq_bytes=4))]
        datagrams = [ok]
        for _, c in cases:
            datagrams += [c, ok]
        bodies = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for d in datagrams for _, n in d["msgs"]]
        src = Sources(hip, bodies, skew=3)
        pitch = 113
        out = Guarded(hip, len(datagrams) * pitch, 9)
        ob, mb, ro, rb, rc = build_call(framer, datagrams, src.addr, out.ptr, pitch)
        assert list(rc) == [0] + [1, 0] * len(cases), rc
        want, it = [], iter(bodies)
        for d in datagrams:
            msgs = [(t, next(it)) for t, _ in d["msgs"]]
            r = R.build(msgs, d["seq"], d["seq_bytes"], d["nonce"], d["nonce_bytes"], None, d["ts24"], d["flag_bits"], max_bytes=100, pitch=pitch)
            want.append(r[1])
        assert [len(w) for w in want] == [int(x) for x in ob] and all(len(w) == 0 for w in want[1::2])
        out.check()
        msg = differing(out.download(), layout(want, pitch), pitch)
        assert not msg, msg
        # a total above pitch: the same datagram is built at pitch 35 and refused at 34
        for p, code in ((35, 0), (34, 1)):
            small = Guarded(hip, 2 * p, 1)
            r = build_call(framer, [ok, ok], src.addr[:2] * 2, small.ptr, p)
            assert list(r[4]) == [code, code] and list(r[0]) == [35 * (1 - code)] * 2
            small.check()
            assert code == 0 or (small.download() == FILL).all()
        # whole-call refusals: nothing is written
        out.fill()
        with pytest.raises(RuntimeError, match="null pointer"):
            build_call(framer, [ok], src.addr[:2], 0, pitch)
        with pytest.raises(RuntimeError, match="pitch too small"):
            build_call(framer, [ok], src.addr[:2], out.ptr, 5)
        with pytest.raises(RuntimeError, match="datagram index"):
            framer.build([1, 0], [6, 6], [1, 1], src.addr[:2], [1, 2], [1, 1], [1, 2], [1, 1], [0, 0], [0, 0], out.ptr, pitch)
        with pytest.raises(RuntimeError, match="datagram index"):
            framer.build([0, 2], [6, 6], [1, 1], src.addr[:2], [1, 2], [1, 1], [1, 2], [1, 1], [0, 0], [0, 0], out.ptr, pitch)
        with pytest.raises(RuntimeError, match="pitch too small"):
            framer.parse([40, 41], out.ptr, 40)
        with pytest.raises(RuntimeError, match="pitch too small"):
            framer.parse([40, 30], out.ptr, 40, offset=[0, 11])
        with pytest.raises(RuntimeError, match="null pointer"):
            framer.parse([40], 0, 40)
        with pytest.raises(RuntimeError, match="null pointer"):
            framer.parse([40], out.ptr, 40, mode=2)
        out.check()
        assert (out.download() == FILL).all()
        # n = 0 and m = 0 are accepted; a datagram without a message is its footer
        r = framer.build([], [], [], [], [], [], [], [], [], [], out.ptr, pitch)
        assert all(x.size == 0 for x in r)
        r = framer.build([], [], [], [], [5], [1], [7], [1], [0x030201], [0], out.ptr, pitch)
        assert list(r[4]) == [0] and list(r[0]) == [8] and list(r[1]) == [0]
        assert out.download()[:9].tolist() == [5, 7, 1, 2, 3, 0x80 | 1 << 2 | 1, 0, 0, FILL]
        assert all(x.size == 0 for x in framer.parse([], out.ptr, pitch))
        # a section longer than the handle allows is not walked
        st, cnt, _, _, _ = framer.parse([101, 0], out.ptr, pitch)
        assert list(st) == [1, 0] and list(cnt) == [0, 0]
        src.check()
    finally:
        framer.close()


# ---- 2. parse against the reference ----

OFFSETS = 23


@pytest.fixture(scope="module")
def p_cases(hip):
    """The P lines in two groups, each uploaded twice: sections at i * pitch, and at
    i * pitch + (i * 7) % 23.  Per group: the lines, the expected results per mode (the
    restatement's, equal to the fixture's), the pitch, and the two buffers with their images."""
    k = R.kat()
    groups = []
    for pick in (lambda n: n <= 6000, lambda n: n > 6000):
        lines = [p for p in k["P"] if pick(p["bytes"])]
        sections = [R.p_section(p, k) for p in lines]
        want = []
        for mode in (0, 1):
            rows = [R.parse(s, mode) for s in sections]
            for p, (status, entries, lo, n) in zip(lines, rows):
                assert (status, len(entries), lo, n, R.table_fnv(entries)) == p["modes"][mode]
            want.append(rows)
        pitch = max(len(s) for s in sections) + 11 + OFFSETS
        placed = []
        for offsets, skew in ((None, 5), ([(i * 7) % OFFSETS for i in range(len(lines))], 0)):
            buf = Guarded(hip, len(lines) * pitch, skew)
            image = layout(sections, pitch, offsets)
            buf.upload(image)
            placed.append((offsets, buf, image))
        groups.append((lines, sections, want, pitch, placed))
    assert sum(len(g[0]) for g in groups) == len(k["P"]) and all(g[0] for g in groups)
    return groups


@pytest.mark.parametrize("cap", (1, 16, 700))
@pytest.mark.parametrize("mode", (0, 1))
def test_parse_equals_the_reference(framer, p_cases, mode, cap):
    """Every P line with a null and a non-null offset list.  Rows are `cap` entries apart in a table
    prefilled with a sentinel and one entry longer than the call needs: an entry past
    min(n_messages, cap) of its row that changed would show in the sentinel or in the next row."""
    for lines, sections, want, pitch, placed in p_cases:
        n = len(lines)
        for offsets, buf, image in placed:
            table = np.full(n * cap + 1, SENTINEL, dtype=np.uint32)
            status, count, lo, nb, _ = framer.parse([len(s) for s in sections], buf.ptr, pitch, mode=mode, cap=cap, offset=offsets,
                                                    table=table)
            expect = np.full(n * cap + 1, SENTINEL, dtype=np.uint32)
            for i, (st, entries, rlo, rn) in enumerate(want[mode]):
                got = (int(status[i]), int(count[i]), int(lo[i]), int(nb[i]))
                assert got == (st, len(entries), rlo, rn), f"line {lines[i]}, mode {mode}: {got}"
                kept = entries[:cap]
                expect[i * cap:i * cap + len(kept)] = kept
            bad = np.flatnonzero(table != expect)
            assert bad.size == 0, f"table entry {int(bad[0]) % cap} of line {lines[int(bad[0]) // cap]}: {int(table[bad[0]]):#x}, want {int(expect[bad[0]]):#x}"
            buf.check()
            assert (buf.download() == image).all(), "parse wrote to the sections"


# ---- 3. the offset forms of the codec's add calls ----

def test_adds_at_an_offset_equal_adds_at_offset_0(hip):
    import tonk_amd
    rng = np.random.default_rng(11)
    lens = [LENGTHS[(i * 3 + i // 8) % 10] for i in range(24)]
    streams = [i // 8 for i in range(24)]
    offs = [(0, 1, 7, 300)[i % 4] for i in range(24)]
    payloads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    pitch, rpitch, maxb = 129 + 300 + 3, 129 + 11, 129
    plain, shifted = Guarded(hip, 24 * pitch, 3), Guarded(hip, 24 * pitch, 6)
    plain.upload(layout(payloads, pitch))
    shifted.upload(layout(payloads, pitch, offs))
    codecs = [tonk_amd.BatchCodec(3, maxb, 48 << 20) for _ in range(4)]
    try:
        enc0, enc1, dec0, dec1 = codecs
        pn0, rc0 = enc0.encoder_add(streams, lens, plain.ptr, pitch)
        pn1, rc1 = enc1.encoder_add(streams, lens, shifted.ptr, pitch, offset=offs)
        assert (rc0 == 0).all() and (rc1 == rc0).all() and (pn1 == pn0).all() and list(pn0) == list(range(8)) * 3
        order = [0, 1, 2, 0, 1, 2]
        rec = []
        for enc in (enc0, enc1):
            out = Guarded(hip, len(order) * rpitch, 1)
            nb, rc = enc.encode(order, out.ptr, rpitch)
            assert (rc == 0).all()
            out.check()
            rec.append((out, nb, out.download()))
        assert (rec[0][1] == rec[1][1]).all() and (rec[0][2] == rec[1][2]).all(), "recovery packets differ"
        with pytest.raises(RuntimeError, match="pitch smaller"):
            enc1.encoder_add([0], [129], shifted.ptr, pitch, offset=[304])
        with pytest.raises(RuntimeError, match="pitch smaller"):
            dec1.decoder_add_original([0], [0], [129], shifted.ptr, pitch, offset=[304])
        # receiver: packet 2 of every stream is lost; the kept ones arrive in slots of their own
        keep = [i for i in range(24) if i % 8 != 2]
        got = []
        for dec, off in ((dec0, None), (dec1, [offs[(i * 5) % 24] for i in keep])):
            buf = Guarded(hip, len(keep) * pitch, 5)
            buf.upload(layout([payloads[i] for i in keep], pitch, off))
            rc = dec.decoder_add_original([streams[i] for i in keep], [int(pn0[i]) for i in keep], [lens[i] for i in keep], buf.ptr, pitch,
                                          offset=off)
            rcr = dec.decoder_add_recovery(order, rec[0][1], rec[0][0].ptr, rpitch)
            out = Guarded(hip, 8 * pitch, 2)
            src, os_, op, ob = dec.decode([0, 1, 2], out.ptr, pitch, 8)
            out.check()
            buf.check()
            got.append((list(rc), list(rcr), list(src), list(os_), list(op), list(ob), out.download()))
        assert got[0][:6] == got[1][:6] and (got[0][6] == got[1][6]).all()
        assert got[0][3] == [0, 1, 2] and got[0][4] == [2, 2, 2] and got[0][5] == [lens[2], lens[10], lens[18]]
        for j, i in enumerate((2, 10, 18)):
            assert got[0][6][j * pitch:j * pitch + lens[i]].tobytes() == payloads[i]
        plain.check()
        shifted.check()
    finally:
        for c in codecs:
            c.close()


# ---- 4. the joined path ----

def test_build_encode_seal_lose_open_parse_decode(hip):
    """3 streams x 24 datagrams of 1-4 messages, every fifth beginning with an Unreliable message;
    the reliable spans go to the encoder where they lie, two recovery packets per 8 datagrams are
    wrapped as OnlyFEC datagrams, everything is sealed; datagrams 3 and 11 of every stream are lost;
    the receiver reads the footers, opens, parses, adds the spans and the recovery packets where
    they lie, decodes, and parses what was recovered."""
    import tonk_amd
    rng = np.random.default_rng(21)
    NS, ND, MAXD, pitch = 3, 24, 1500, 1411
    choices = (0, 1, 15, 16, 17, 300)
    keys = [0x0123456789abcdef, 0, 0xffffffff00000001]
    framer, sealer, sender, receiver = (tonk_amd.DatagramFramer(MAXD), tonk_amd.DatagramSealer(NS, MAXD),
                                        tonk_amd.BatchCodec(NS, 1300, 48 << 20), tonk_amd.BatchCodec(NS, 1300, 48 << 20))
    try:
        for s, key in enumerate(keys):
            sealer.set_key(s, key)
        # datagram i = tick * 24 + stream * 8 + j is number k = tick * 8 + j of its stream
        sent = []
        for i in range(NS * ND):
            tick, s, j = i // 24, (i % 24) // 8, i % 8
            k = tick * 8 + j
            n_msgs = 1 + (i * 7 + k) % 4
            msgs = [((3 if k % 5 == 0 and m == 0 else 6 + (i + m) % 3), choices[(i * 5 + m * 7 + k) % 6]) for m in range(n_msgs)]
            if k % 5 == 0 and n_msgs == 1:
                msgs.append((6, 17))
            sent.append(dict(stream=s, k=k, msgs=msgs, seq=k, seq_bytes=2, nonce=(1 << 24) * (s + 1) + 1000 + k, nonce_bytes=3, handshake=None,
                             ts24=int(rng.integers(0, 1 << 24)), flag_bits=R.SEQCOMP))
        bodies = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for d in sent for _, n in d["msgs"]]
        it = iter(bodies)
        for d in sent:
            d["bodies"] = [next(it) for _ in d["msgs"]]
            d["ref"] = R.build(list(zip([t for t, _ in d["msgs"]], d["bodies"])), d["seq"], 2, d["nonce"] & 0xFFFFFFFF, 3, None, d["ts24"], d["flag_bits"])
            assert d["ref"][0] == 0
        assert any(d["ref"][3] > 0 for d in sent) and all(d["ref"][4] > 0 for d in sent)
        src = Sources(hip, bodies, skew=5)
        out = Guarded(hip, len(sent) * pitch, 7)
        ob, mb, ro, rb, rc = build_call(framer, sent, src.addr, out.ptr, pitch)
        assert (rc == 0).all()
        assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(ob, mb, ro, rb)] == [(len(d["ref"][1]),) + d["ref"][2:] for d in sent]
        built = out.download()
        msg = differing(built, layout([d["ref"][1] for d in sent], pitch), pitch)
        assert not msg, msg

        # the FEC step, tick by tick, on the spans where they lie
        rpitch, order = 1311, [0, 1, 2, 0, 1, 2]
        recs = Guarded(hip, 3 * len(order) * rpitch, 3)
        rec_bytes = []
        for tick in range(3):
            lo, hi = tick * 24, tick * 24 + 24
            pn, rc = sender.encoder_add([d["stream"] for d in sent[lo:hi]], rb[lo:hi], out.ptr + lo * pitch, pitch, offset=ro[lo:hi])
            assert (rc == 0).all() and [int(x) for x in pn] == [d["k"] for d in sent[lo:hi]]
            nb, rc = sender.encode(order, recs.ptr + tick * len(order) * rpitch, rpitch)
            assert (rc == 0).all()
            rec_bytes += [int(x) for x in nb]
        recs.check()
        fec = [dict(stream=order[i % 6], msgs=[(R.RAW, rec_bytes[i])], seq=0, seq_bytes=0, nonce=(1 << 24) * (order[i % 6] + 1) + 5000 + i,
                    nonce_bytes=3, handshake=None, ts24=int(rng.integers(0, 1 << 24)), flag_bits=R.ONLYFEC | R.SEQCOMP) for i in range(18)]
        fout = Guarded(hip, len(fec) * pitch, 2)
        fob, fmb, _, _, rc = build_call(framer, fec, [recs.ptr + i * rpitch for i in range(18)], fout.ptr, pitch)
        assert (rc == 0).all() and [int(x) for x in fmb] == rec_bytes and [int(x) for x in fob] == [n + 9 for n in rec_bytes]
        fout.check()
        rec_image = recs.download()
        fec_built = fout.download()
        for i in range(18):
            assert (fec_built[i * pitch:i * pitch + rec_bytes[i]] == rec_image[i * rpitch:i * rpitch + rec_bytes[i]]).all()

        for buf, items, nbytes, mbytes in ((out, sent, ob, mb), (fout, fec, fob, fmb)):
            rc = sealer.seal([d["stream"] for d in items], [d["nonce"] for d in items], nbytes, mbytes, buf.ptr, pitch)
            assert (rc == 0).all()
            buf.check()

        # the channel: datagrams 3 and 11 of every stream never arrive
        kept = [i for i, d in enumerate(sent) if d["k"] not in (3, 11)]
        lost = [i for i, d in enumerate(sent) if d["k"] in (3, 11)]
        assert len(lost) == 6
        rx = Guarded(hip, (len(kept) + len(fec)) * pitch, 4)
        arrived = [(out, i, sent[i], int(ob[i])) for i in kept] + [(fout, i, fec[i], int(fob[i])) for i in range(18)]
        for slot, (buf, i, _, _) in enumerate(arrived):
            hip.copy(rx.ptr + slot * pitch, buf.ptr + i * pitch, pitch)
        nbytes = [a[3] for a in arrived]

        # receiver: flags, lengths and the truncated fields from the footers
        foot = sealer.footers(nbytes, rx.ptr, pitch)
        flags = foot[:, 21].astype(np.uint32)
        seq_b, nonce_b, hs_b = flags & 3, (flags >> 2) & 3, np.where(flags & 0x40, 12, 0)
        assert (flags & 0x80).all() and (hs_b == 0).all() and (nonce_b == 3).all()
        only_fec = (flags & R.ONLYFEC) != 0
        assert list(only_fec) == [False] * len(kept) + [True] * 18
        msg_bytes = np.asarray(nbytes, dtype=np.uint32) - (seq_b + nonce_b + hs_b + 6)
        for slot, (_, _, d, _) in enumerate(arrived):
            # (expansion of the nonce and the sequence number is the caller's: the test knows them
            # and checks that the footer carries their low bytes)
            tail = foot[slot, :18].tobytes()
            assert tail[15:18] == (d["nonce"] & 0xFFFFFF).to_bytes(3, "little")
            if not only_fec[slot]:
                assert tail[13:15] == d["seq"].to_bytes(2, "little") and seq_b[slot] == 2
        rc = sealer.open([a[2]["stream"] for a in arrived], [a[2]["nonce"] for a in arrived], nbytes, msg_bytes, rx.ptr, pitch)
        assert (rc == 0).all(), rc
        rx.check()
        opened = rx.download()
        for slot, (_, i, d, nb) in enumerate(arrived):
            want = (built if not only_fec[slot] else fec_built)[i * pitch:i * pitch + nb - 2]
            assert (opened[slot * pitch:slot * pitch + nb - 2] == want).all(), f"datagram {slot} did not open to what was built"

        nk = len(kept)
        status, count, lo, nb_rel, table = framer.parse(msg_bytes[:nk], rx.ptr, pitch, mode=0, cap=4)
        assert (status == 0).all()
        for slot, i in enumerate(kept):
            d = sent[i]
            want = R.parse(d["ref"][1][:d["ref"][2]])
            assert want[0] == 0 and [t for t, _ in d["msgs"]] == [e >> 27 for e in want[1]]
            assert list(table[slot, :int(count[slot])]) == want[1] and (int(lo[slot]), int(nb_rel[slot])) == d["ref"][3:5]
            at = slot * pitch
            for e, body in zip(want[1], d["bodies"]):
                assert opened[at + (e & 0xFFFF):at + (e & 0xFFFF) + ((e >> 16) & 2047)].tobytes() == body
        assert (seq_b[:nk] != 0).all()  # ("Reliable data sent with no sequence number" is a flags check)
        rc = receiver.decoder_add_original([sent[i]["stream"] for i in kept], [sent[i]["seq"] for i in kept], nb_rel, rx.ptr, pitch, offset=lo)
        assert (rc == 0).all(), rc
        rc = receiver.decoder_add_recovery([d["stream"] for d in fec], msg_bytes[nk:], rx.ptr + nk * pitch, pitch)
        assert (rc == 0).all(), rc
        back = Guarded(hip, 8 * pitch, 6)
        # (a decode call returns what the decoder can solve at once: the loss inside the first
        # recovery packets' range first, the later one with the next call, as siamese_decode does)
        os_, op, obytes = [], [], []
        for _ in range(4):
            src_rc, s_, p_, b_ = receiver.decode([0, 1, 2], back.ptr + len(os_) * pitch, pitch, 8 - len(os_))
            assert set(src_rc) <= {0, 2}, src_rc
            os_, op, obytes = os_ + list(s_), op + list(p_), obytes + list(b_)
            if (src_rc == 2).all():
                break
        back.check()
        rx.check()
        assert sorted(zip(map(int, os_), map(int, op))) == [(s, k) for s in range(NS) for k in (3, 11)]
        recovered = back.download()
        by_key = {(d["stream"], d["k"]): d for d in sent}
        for j, (s, k) in enumerate(zip(os_, op)):
            rcb, dgram, _, lo_, n_ = by_key[(int(s), int(k))]["ref"]
            assert int(obytes[j]) == n_
            assert recovered[j * pitch:j * pitch + n_].tobytes() == dgram[lo_:lo_ + n_], f"stream {s} packet {k}"
        status, count, lo2, nb2, table = framer.parse(obytes, back.ptr, pitch, mode=1, cap=4)
        assert (status == 0).all() and (lo2 == 0).all() and (nb2 == obytes).all()
        for j, (s, k) in enumerate(zip(os_, op)):
            d = by_key[(int(s), int(k))]
            rel = [(t, body) for (t, _), body in zip(d["msgs"], d["bodies"]) if t >= 5]
            assert int(count[j]) == len(rel)
            for e, (t, body) in zip(table[j], rel):
                e = int(e)
                assert e >> 27 == t and (e >> 16) & 2047 == len(body)
                assert recovered[j * pitch + (e & 0xFFFF):j * pitch + (e & 0xFFFF) + len(body)].tobytes() == body
        src.check()
    finally:
        for h in (framer, sealer, sender, receiver):
            h.close()
