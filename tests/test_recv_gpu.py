"""The receive front in device memory (include/tonk_receive.h, tonk_amd.DatagramReceiver) on an
MI355X.  Datagrams are made on the device by DatagramFramer.build and DatagramSealer.seal (both
proven against the reference by their own tests); the expectations come from the Python
restatement of the reference's state machine (tests/recv_ref.py, checked against the recorded
transcripts by tests/test_recv.py) and from the transcripts themselves
(tests/golden/recv_kat.txt.gz).  Every call's buffer has 64 guard bytes of 0xA5 on each side and
0xA5 between the slots; after every call the whole buffer, every result record, the register state
of every stream read back from the device and next_expected are compared."""
from __future__ import annotations

import numpy as np
import pytest

import recv_ref as R
from batch_ref import Guarded
from lz_streams import Hip

pytestmark = [pytest.mark.gpu]

KEYS = [0, 0x0123456789abcdef, 0xffffffff00000001, 0x00000000deadbeef]
MAXB = 1400
FILL = Guarded.FILL
N_STREAMS = 12


def key_of(stream: int) -> int:
    return KEYS[stream % len(KEYS)]


@pytest.fixture(scope="module")
def hip():
    h = Hip()
    yield h
    h.close()


class Factory:
    """Datagrams as a Tonk sender makes them, on the device: DatagramFramer.build lays out one
    unreliable message (random body) and the footer, DatagramSealer.seal ciphers and tags."""

    def __init__(self, hip):
        import tonk_amd
        self.hip = hip
        self.framer = tonk_amd.DatagramFramer(MAXB)
        self.sealer = tonk_amd.DatagramSealer(N_STREAMS, MAXB)
        for s in range(N_STREAMS):
            self.sealer.set_key(s, key_of(s))
        self.rng = np.random.default_rng(20260)

    def make(self, specs):
        """specs: dicts(stream, nonce, nb, sb, bytes[, hs]).  Returns [(wire, plain)] as uint8 arrays."""
        n = len(specs)
        dg, mt, mb, bodies = [], [], [], []
        for i, s in enumerate(specs):
            F = 6 + (12 if s.get("hs") else 0) + s["nb"] + s["sb"]
            M = s["bytes"] - F
            assert M == 0 or M >= 2, s
            if M:
                dg.append(i)
                mt.append(1)
                mb.append(M - 2)
                bodies.append(self.rng.integers(0, 256, M - 2, dtype=np.uint8))
        src = Guarded(self.hip, max(sum(b.size for b in bodies), 1), 3)
        if bodies:
            src.upload(np.concatenate(bodies) if sum(b.size for b in bodies) else np.zeros(1, np.uint8))
        at = np.cumsum([0] + [b.size for b in bodies])[:-1]
        pitch = max(s["bytes"] for s in specs) + 3
        out = Guarded(self.hip, n * pitch, 5)
        hs = self.rng.integers(0, 256, (n, 12), dtype=np.uint8)
        ob, msg, _, _, rc = self.framer.build(dg, mt, mb, [src.ptr + int(a) for a in at], [s.get("seq", 7 + i) for i, s in enumerate(specs)],
                                              [s["sb"] for s in specs], [s["nonce"] & 0xFFFFFFFF for s in specs], [s["nb"] for s in specs],
                                              [(i * 2654435761 + 99) & 0xFFFFFF for i in range(n)], [0x20 if i % 3 == 0 else 0 for i in range(n)],
                                              out.ptr, pitch, handshake=hs, has_handshake=[1 if s.get("hs") else 0 for s in specs])
        assert (rc == 0).all() and [int(x) for x in ob] == [s["bytes"] for s in specs]
        plain = out.download()
        rc = self.sealer.seal([s["stream"] for s in specs], [s["nonce"] for s in specs], ob, msg, out.ptr, pitch)
        assert (rc == 0).all()
        sealed = out.download()
        out.check()
        return [(sealed[i * pitch:i * pitch + s["bytes"]].copy(), plain[i * pitch:i * pitch + s["bytes"]].copy()) for i, s in enumerate(specs)]

    def close(self):
        self.framer.close()
        self.sealer.close()


@pytest.fixture(scope="module")
def factory(hip):
    f = Factory(hip)
    yield f
    f.close()


def corrupt(wire, bit=0):
    w = wire.copy()
    w[w.size - 2 + bit // 8] ^= 1 << (bit % 8)
    return w


def receiver(keys=None, n=N_STREAMS, maxb=MAXB):
    import tonk_amd
    rx = tonk_amd.DatagramReceiver(n, maxb)
    for s in range(n):
        rx.set_key(s, key_of(s) if keys is None else keys[s])
    return rx


def fresh_model(bases=None, keys=None, n=N_STREAMS):
    return [R.Connection(key_of(s) if keys is None else keys[s], 0 if bases is None else bases[s]) for s in range(n)]


def check_call(hip, rx, model, items, pitch, skew=0, maxb=MAXB):
    """One receive call of `items` [(stream, wire)] against the model (advanced in list order):
    result codes, records, every byte of the buffer, the states and next_expected of every stream.
    Returns (rc, result)."""
    n = len(items)
    want = np.full(n * pitch, FILL, dtype=np.uint8)
    sent = want.copy()
    codes, records = [], []
    for i, (s, w) in enumerate(items):
        sent[i * pitch:i * pitch + w.size] = w
        rc, res, after = model[s].receive(w, maxb)
        want[i * pitch:i * pitch + w.size] = after
        codes.append(rc)
        records.append(res)
    buf = Guarded(hip, n * pitch, skew)
    buf.upload(sent)
    rc, result = rx.receive([s for s, _ in items], [w.size for _, w in items], buf.ptr, pitch)
    buf.check()
    got = buf.download()
    assert list(rc) == codes, (list(rc), codes)
    for i, res in enumerate(records):
        for name in result.dtype.names:
            assert int(result[name][i]) == (res[name] if res else 0), (i, name, result[i], res)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"slot {bad[0] // pitch} byte {bad[0] % pitch}: got {got[bad[0]]:#04x}, want {want[bad[0]]:#04x} ({bad.size} differ)"
    check_states(rx, model, sorted({s for s, _ in items}))
    return rc, result


def check_states(rx, model, streams):
    for s in streams:
        assert (rx.state(s) == model[s].reg.words()).all(), (s, rx.state(s)[:3], model[s].reg.words()[:3])
    assert list(rx.next_expected(streams)) == [(model[s].reg.largest + 1) & R.M64 for s in streams]


# ---- 1. lengths and alignments ----

def test_lengths_widths_and_alignments(hip, factory):
    lens = [6, 7, 8, 13, 14, 22, 23, 37, 38, 39, 46, 70, 71, 134, 135, 262, 1306]
    rx, model = receiver(), fresh_model()
    specs, nonce = [], [0, 0, 0]
    for stream in (0, 1, 2):  # keys {0, non-zero, non-zero}
        for nbytes in lens:
            for nb in range(4):
                # the sequence bytes that leave no message byte or at least a frame header
                sb = next((sb for sb in (0, 1, 2, 3) if nbytes - 6 - nb - sb == 0 or nbytes - 6 - nb - sb >= 2), None)
                if sb is None or nbytes < 6 + nb + sb:
                    continue
                nonce[stream] += 1
                specs.append(dict(stream=stream, nonce=nonce[stream], nb=nb, sb=sb, bytes=nbytes))
    made = factory.make(specs)
    assert {s["bytes"] for s in specs} == set(lens) and {s["nb"] for s in specs} == {0, 1, 2, 3}
    items = [(s["stream"], w) for s, (w, _) in zip(specs, made)]
    third = (len(items) + 2) // 3
    for part, skew in ((items[:third], 1), (items[third:2 * third], 8), (items[2 * third:], 15)):
        rc, result = check_call(hip, rx, model, part, 1311, skew)
        assert (rc == 0).all()
    # what was deciphered is what was sealed (the model's bytes above), and the records are the senders' fields
    for (s, (w, plain)) in zip(specs, made):
        after = fresh_model()[s["stream"]]
        after.reg.reset(s["nonce"] - 1)
        rc, res, back = after.receive(w)
        assert rc == 0 and (back[:res["message_bytes"]] == plain[:res["message_bytes"]]).all() and res["nonce"] == s["nonce"]
        assert (res["seq_bytes"], res["nonce_bytes"], res["message_bytes"]) == (s["sb"], s["nb"], s["bytes"] - 6 - s["nb"] - s["sb"])
    assert rx.kernel_ms()["repaired_tags"] == 0
    rx.close()


# ---- 2. agreement with the existing path ----

def test_one_datagram_per_stream_agrees_with_footers_expansion_and_open(hip, factory):
    rx = receiver()
    bases = [1000 * (s + 1) for s in range(N_STREAMS)]
    largest = list(bases)
    for s in range(N_STREAMS):
        rx.reset(s, bases[s])
    specs = [dict(stream=s, nonce=bases[s] + 1 + s, nb=s % 4 if s % 4 else (1 if s else 0), sb=s % 3, bytes=60 + 13 * s, hs=s % 5 == 4)
             for s in range(N_STREAMS)]
    specs[0]["nonce"] = bases[0] + 1  # (no nonce bytes: the next expected)
    made = factory.make(specs)
    wires = [w for w, _ in made]
    wires[3] = corrupt(wires[3], 5)
    pitch = 260
    sent = np.full(N_STREAMS * pitch, FILL, dtype=np.uint8)
    for i, w in enumerate(wires):
        sent[i * pitch:i * pitch + w.size] = w
    a, b = Guarded(hip, sent.size, 2), Guarded(hip, sent.size, 2)
    a.upload(sent)
    b.upload(sent)
    streams, nbytes = list(range(N_STREAMS)), [w.size for w in wires]
    # today's path: footers to the host, expansion there, open
    foot = factory.sealer.footers(nbytes, a.ptr, pitch)
    nonces, msgs = [], []
    for s in streams:
        flags = int(foot[s, 21])
        hs, nb = (12 if flags & 0x40 else 0), (flags >> 2) & 3
        partial = int.from_bytes(bytes(foot[s, 18 - hs - nb:18 - hs]), "little")
        nonces.append(R.expand(largest[s], partial, nb))
        msgs.append(nbytes[s] - R.footer_bytes(flags))
    rc_open = factory.sealer.open(streams, nonces, nbytes, msgs, a.ptr, pitch)
    rc, result = rx.receive(streams, nbytes, b.ptr, pitch)
    a.check()
    b.check()
    assert list(rc) == list(rc_open) == [2 if s == 3 else 0 for s in streams]
    assert (a.download() == b.download()).all()
    assert [int(x) for x in result["nonce"]] == nonces and [int(x) for x in result["message_bytes"]] == msgs
    rx.close()


# ---- 3. order and repair ----

def test_a_failed_tag_changes_what_the_next_datagram_expands_to(hip, factory):
    rx, model = receiver(), fresh_model([100] * N_STREAMS)
    for s in range(N_STREAMS):
        rx.reset(s, 100)
    trio = lambda s: [dict(stream=s, nonce=101, nb=1, sb=0, bytes=90), dict(stream=s, nonce=300, nb=2, sb=0, bytes=90),
                      dict(stream=s, nonce=110, nb=1, sb=0, bytes=90)]
    fillers = [dict(stream=2 + k % 8, nonce=101 + k // 8, nb=1, sb=0, bytes=30 + k % 17) for k in range(2 * 136)]
    made = factory.make(trio(1) + trio(10) + fillers)
    w = [x for x, _ in made]
    fill = [(f["stream"], x) for f, x in zip(fillers, w[6:])]
    # stream 1: the middle tag corrupted; stream 10: intact.  136 datagrams of other streams between
    # a stream's three: each lies in another workgroup of 64
    items = ([(1, w[0]), (10, w[3])] + fill[:136] + [(1, corrupt(w[1])), (10, w[4])] + fill[136:] + [(1, w[2]), (10, w[5])])
    where = [i for i, (s, _) in enumerate(items) if s == 1]
    assert len({i // 64 for i in where}) == 3
    rx.kernel_ms()
    rc, result = check_call(hip, rx, model, items, 96, 7)
    assert [int(rc[i]) for i in where] == [0, 2, 0] and int(result["nonce"][where[2]]) == 110
    other = [i for i, (s, _) in enumerate(items) if s == 10]
    assert [int(rc[i]) for i in other] == [0, 0, 2] and int(result["nonce"][other[2]]) == 366
    assert rx.kernel_ms()["repaired_tags"] >= 1
    rx.close()


# ---- 4. replay ----

def test_replays_slides_jumps_and_reset(hip, factory):
    rx, model = receiver(), fresh_model()
    s = 1
    specs = [dict(stream=s, nonce=n, nb=2, sb=0, bytes=50) for n in (1, 2, 3)]
    specs += [dict(stream=s, nonce=5000, nb=2, sb=0, bytes=50), dict(stream=s, nonce=2, nb=2, sb=1, bytes=51),
              dict(stream=s, nonce=960 + 4096 + 64, nb=3, sb=0, bytes=50), dict(stream=s, nonce=5001, nb=3, sb=0, bytes=50),
              dict(stream=s, nonce=1088 + 4096 + 64 * 64, nb=3, sb=0, bytes=50), dict(stream=s, nonce=9000, nb=3, sb=0, bytes=50)]
    specs += [dict(stream=t, nonce=n, nb=1, sb=0, bytes=40) for t in (0, 2) for n in (1, 2, 3)]
    w = [x for x, _ in factory.make(specs)]
    nb = [(t["stream"], x) for t, x in zip(specs[9:], w[9:])]
    # the same datagram twice in one call: the second is a duplicate and stays ciphertext
    rc, _ = check_call(hip, rx, model, [(s, w[0]), (s, w[1]), (s, w[1]), (s, w[2])] + nb, 64, 3)
    assert list(rc[:4]) == [0, 0, 3, 0]
    # again in a later call
    rc, _ = check_call(hip, rx, model, [(s, w[1]), (s, w[0])], 64, 4)
    assert list(rc) == [3, 3]
    # a slide (15 words), then a nonce below the base
    rc, _ = check_call(hip, rx, model, [(s, w[3]), (s, w[4])], 64, 5)
    assert list(rc) == [0, 3] and model[s].reg.base == 960
    # a jump of 4096 + 64 from the base (two words), then a nonce inside the window that was never seen
    rc, _ = check_call(hip, rx, model, [(s, w[5]), (s, w[6])], 64, 6)
    assert list(rc) == [0, 0] and (model[s].reg.base, model[s].reg.rotation) == (1088, 1088)
    # a jump of 4096 + 64 * 64 from the base: the window starts again there; what lies before it is too old
    rc, _ = check_call(hip, rx, model, [(s, w[7]), (s, w[8])], 64, 7)
    assert list(rc) == [0, 3] and (model[s].reg.base, model[s].reg.rotation, model[s].reg.window[0]) == (9280, 0, 1)
    # reset of one slot leaves its neighbours alone
    rx.reset(s, 777)
    model[s].reg.reset(777)
    check_states(rx, model, [0, 1, 2, 3])
    rx.close()


# ---- 5. rc 4, rc 1 and refusals ----

def test_reordered_rule_invalid_datagrams_and_refused_calls(hip, factory):
    rx, model = receiver(), fresh_model()
    specs = [dict(stream=1, nonce=5, nb=2, sb=1, bytes=40), dict(stream=1, nonce=3, nb=2, sb=1, bytes=40),  # older, fewer seq bytes: rc 4
             dict(stream=1, nonce=4, nb=2, sb=2, bytes=40),   # older, as many: rc 0
             dict(stream=1, nonce=2, nb=2, sb=0, bytes=40),   # older, none: rc 0
             dict(stream=1, nonce=6, nb=2, sb=1, bytes=40),   # the newest: rc 0
             dict(stream=2, nonce=1, nb=3, sb=3, bytes=24, hs=True), dict(stream=2, nonce=2, nb=1, sb=0, bytes=30),
             dict(stream=2, nonce=3, nb=1, sb=0, bytes=MAXB), dict(stream=2, nonce=4, nb=1, sb=0, bytes=45)]
    w = [x for x, _ in factory.make(specs)]
    rc, _ = check_call(hip, rx, model, [(1, x) for x in w[:5]], 48, 9)
    assert list(rc) == [0, 4, 0, 0, 0]
    # rc 1, each cause, among valid datagrams of the stream; state and bytes untouched (check_call)
    no_flag = w[6].copy()
    no_flag[-3] &= 0x7f
    tiny = np.array([0x80] * 5, dtype=np.uint8)
    six = np.array([0, 0, 0, 0x80 | 1 << 2, 0, 0], dtype=np.uint8)
    small = receiver(maxb=MAXB - 1)
    small_model = fresh_model()
    items = [(2, w[5][1:]), (2, no_flag), (2, tiny), (2, six), (2, w[7]), (2, w[8])]
    rc, _ = check_call(hip, small, small_model, items, MAXB + 4, 2, maxb=MAXB - 1)
    assert list(rc) == [1, 1, 1, 1, 1, 0]  # (the last one is valid: the invalid ones before it changed nothing)
    small.close()
    rc, _ = check_call(hip, rx, model, [(2, w[5]), (2, w[6]), (2, w[7]), (2, w[8])], MAXB + 4, 11)
    assert list(rc) == [0, 0, 0, 0]
    # calls refused as a whole: -2, -3, -1; every state as it was, nothing written
    buf = Guarded(hip, 4 * 48, 1)
    sent = np.full(4 * 48, FILL, dtype=np.uint8)
    sent[:40] = w[4]
    buf.upload(sent)
    with pytest.raises(RuntimeError, match="stream id out of range"):
        rx.receive([1, N_STREAMS], [40, 40], buf.ptr, 48)
    with pytest.raises(RuntimeError, match="pitch smaller"):
        rx.receive([1, 1], [40, 48], buf.ptr, 47)
    with pytest.raises(RuntimeError, match="null pointer"):
        rx.receive([1], [40], 0, 48)
    buf.check()
    assert (buf.download() == sent).all()
    check_states(rx, model, list(range(N_STREAMS)))
    rc, _ = rx.receive([], [], buf.ptr, 48)
    assert rc.size == 0
    rx.close()


# ---- 6. the fixture and a soak ----

def test_fixture_transcripts_through_the_handle(hip):
    kat = R.kat()
    n = len(kat)
    rx = receiver(keys=[key for key, _, _ in kat], n=n, maxb=65535)
    for c, (_, base, _) in enumerate(kat):
        rx.reset(c, base)
    wires = [[R.wire(key, k, g[0], g[1], g[2], g[3], g[4], g[5]) for k, g in enumerate(gs)] for key, _, gs in kat]
    chunk, deepest = 24, max(len(gs) for _, _, gs in kat)
    for call, start in enumerate(range(0, deepest, chunk)):
        # round robin over the connections on even calls, connection by connection backwards on odd ones
        picks = [(c, k) for c in range(n) for k in range(start, min(start + chunk, len(kat[c][2])))]
        picks.sort(key=(lambda p: (p[1], p[0])) if call % 2 == 0 else (lambda p: (-p[0], p[1])))
        pitch = max(wires[c][k].size for c, k in picks) + 5
        sent = np.full(len(picks) * pitch, FILL, dtype=np.uint8)
        for i, (c, k) in enumerate(picks):
            sent[i * pitch:i * pitch + wires[c][k].size] = wires[c][k]
        buf = Guarded(hip, sent.size, 1 + call % 15)
        buf.upload(sent)
        rc, result = rx.receive([c for c, _ in picks], [wires[c][k].size for c, k in picks], buf.ptr, pitch)
        buf.check()
        got = buf.download()
        for i, (c, k) in enumerate(picks):
            g = kat[c][2][k]
            assert (int(rc[i]), int(result["nonce"][i])) == (g[6], g[7]), (c, k, rc[i], result[i], g)
            assert R.S.fnv1a(got[i * pitch:i * pitch + g[4]]) == g[12], (c, k)
            assert (got[i * pitch + g[4]:(i + 1) * pitch] == FILL).all(), (c, k)
        for c in sorted({c for c, _ in picks}):
            g = kat[c][2][min(start + chunk, len(kat[c][2])) - 1]
            st = rx.state(c)
            assert (int(st[0]), int(st[1]), int(st[2])) == g[8:11], (c, st[:3], g)
            assert R.S.fnv1a(st[3:].astype("<u8").tobytes()) == g[11], c
    rx.close()


def test_soak_shuffled_with_loss_repeats_and_bad_tags(hip, factory):
    rng = np.random.default_rng(77)
    rx, model = receiver(), fresh_model([50 * s for s in range(N_STREAMS)])
    for s in range(N_STREAMS):
        rx.reset(s, 50 * s)
    specs = []
    for s in range(8):
        for k in range(40):
            nb = int(rng.integers(0, 4))
            sb = int(rng.integers(0, 4))
            specs.append(dict(stream=s, nonce=50 * s + 1 + k + (200 if k > 30 else 0), nb=nb, sb=sb, bytes=6 + nb + sb + 2 + int(rng.integers(0, 120))))
    made = [w for w, _ in factory.make(specs)]
    items = []
    for t, w in zip(specs, made):
        u = rng.random()
        if u < 0.1:
            continue  # lost
        items.append((t["stream"], corrupt(w, int(rng.integers(0, 16))) if u < 0.3 else w))
        if u > 0.9:
            items.append((t["stream"], w))  # again
    # shuffled within a reach of a dozen places
    order = np.argsort(np.arange(len(items)) + rng.uniform(0, 12, len(items)))
    items = [items[i] for i in order]
    third = len(items) // 3
    rx.kernel_ms()
    seen = set()
    for part, skew in ((items[:third], 3), (items[third:2 * third], 0), (items[2 * third:], 13)):
        rc, _ = check_call(hip, rx, model, part, 160, skew)
        seen |= {int(x) for x in rc}
    assert {0, 2, 3} <= seen
    assert rx.kernel_ms()["repaired_tags"] >= 1
    rx.close()


# ---- 7. datagrams above 1400 bytes ----

LONG_MAXB = 65535
TAG_TILE = 128  # seal.h TAMD_SEAL_TILE: tamd_rx_tag hashes a group's datagrams in tiles of 128 bytes


class LongFactory:
    """Datagrams of up to 65535 bytes: a random body (a message frame holds at most 2047 bytes, and
    the receive front does not look inside) behind the footer dgram_ref lays, ciphered and tagged
    on the device by DatagramSealer.seal, which its own test proves at 65535."""

    def __init__(self, hip):
        import tonk_amd
        self.hip = hip
        self.sealer = tonk_amd.DatagramSealer(N_STREAMS, LONG_MAXB)
        for s in range(N_STREAMS):
            self.sealer.set_key(s, key_of(s))
        self.rng = np.random.default_rng(20261)

    def make(self, specs):
        """specs: dicts(stream, nonce, nb, sb, bytes).  Returns the sealed datagrams as uint8 arrays."""
        import dgram_ref as D
        n, pitch = len(specs), max(s["bytes"] for s in specs) + 3
        plain = np.full(n * pitch, FILL, dtype=np.uint8)
        msgs = []
        for i, s in enumerate(specs):
            M = s["bytes"] - 6 - s["nb"] - s["sb"]
            assert M >= 0, s
            foot = D.footer(7 + i, s["sb"], s["nonce"], s["nb"], None, (i * 2654435761 + 99) & 0xFFFFFF, D.ONLYFEC if i % 3 == 0 else 0)
            plain[i * pitch:i * pitch + M] = self.rng.integers(0, 256, M, dtype=np.uint8)
            plain[i * pitch + M:i * pitch + s["bytes"]] = np.frombuffer(foot, dtype=np.uint8)
            msgs.append(M)
        buf = Guarded(self.hip, n * pitch, 5)
        buf.upload(plain)
        rc = self.sealer.seal([s["stream"] for s in specs], [s["nonce"] for s in specs], [s["bytes"] for s in specs], msgs, buf.ptr, pitch)
        assert (rc == 0).all()
        sealed = buf.download()
        buf.check()
        return [sealed[i * pitch:i * pitch + s["bytes"]].copy() for i, s in enumerate(specs)]

    def close(self):
        self.sealer.close()


@pytest.fixture(scope="module")
def long_factory(hip):
    f = LongFactory(hip)
    yield f
    f.close()


def short_specs(n, streams, first_nonce=1):
    """n datagrams of 6 to 40 bytes over `streams` in turn, nonces counting up per stream."""
    specs, nonce = [], {s: first_nonce - 1 for s in streams}
    for k in range(n):
        s, nbytes = streams[k % len(streams)], 6 + k % 35
        nb = min(k % 4, nbytes - 6)
        nonce[s] += 1
        specs.append(dict(stream=s, nonce=nonce[s], nb=nb, sb=min((k // 4) % 4, nbytes - 6 - nb), bytes=nbytes))
    return specs


def test_long_datagrams_at_the_tile_edges_with_every_nonce_width(hip, long_factory):
    """The tagged part (bytes - 6) one below, at and one above 11, 12, 32 and 511 tiles of 128 bytes,
    around 2048, and the two longest datagrams, each with 0, 1, 2 and 3 nonce bytes; in three
    calls, each one group of 64 whose longest datagram sets the tile loop's length for all."""
    tagged = [TAG_TILE * k + e for k in (11, 12, 32, 511) for e in (-1, 0, 1)] + [2047, 2048, 2049, 65534 - 6, 65535 - 6]
    assert max(tagged) == LONG_MAXB - 6 and (max(tagged) + TAG_TILE - 1) // TAG_TILE == 512
    rx, model = receiver(maxb=LONG_MAXB), fresh_model()
    raw = [dict(stream=(k + nb) % 3, nb=nb, sb=(k + 2 * nb) % 4, bytes=t + 6) for k, t in enumerate(tagged) for nb in range(4)]
    specs, nonce = [], [0, 0, 0]  # keys {0, non-zero, non-zero}
    for spec in raw[0::3] + raw[1::3] + raw[2::3]:  # (every third of the list holds short and long ones alike)
        nonce[spec["stream"]] += 1
        specs.append(dict(spec, nonce=nonce[spec["stream"]]))
    assert {(s["bytes"], s["nb"]) for s in specs} == {(t + 6, nb) for t in tagged for nb in range(4)}
    wires = long_factory.make(specs)
    items = [(s["stream"], w) for s, w in zip(specs, wires)]
    third = (len(items) + 2) // 3
    assert third <= 64
    for part, skew in ((items[:third], 1), (items[third:2 * third], 8), (items[2 * third:], 15)):
        assert max(w.size for _, w in part) >= 65000 and min(w.size for _, w in part) <= 4200
        rc, result = check_call(hip, rx, model, part, LONG_MAXB + 4, skew, maxb=LONG_MAXB)
        assert (rc == 0).all()
    assert rx.kernel_ms()["repaired_tags"] == 0
    rx.close()


def test_a_long_datagram_shares_its_group_with_short_ones(hip, long_factory):
    """One datagram of 65535 bytes and 63 of 6 to 40 bytes of other streams in the first group of 64
    (512 tiles for all of them), a second group of short ones only."""
    rx, model = receiver(maxb=LONG_MAXB), fresh_model()
    long_one = long_factory.make([dict(stream=0, nonce=1, nb=2, sb=1, bytes=LONG_MAXB)])[0]
    specs = short_specs(127, list(range(1, N_STREAMS)))
    shorts = [(s["stream"], w) for s, w in zip(specs, long_factory.make(specs))]
    at = 37
    items = shorts[:at] + [(0, long_one)] + shorts[at:]
    assert len(items) == 128 and at // 64 == 0 and items[at][1].size == LONG_MAXB
    assert all(6 <= w.size <= 40 for i, (_, w) in enumerate(items) if i != at)
    rc, _ = check_call(hip, rx, model, items, LONG_MAXB, 9, maxb=LONG_MAXB)
    assert (rc == 0).all()
    rx.close()


def test_repair_duplicate_and_oversize_on_long_datagrams(hip, long_factory):
    """Stream 1 sends 65535, 40000 and 65535 bytes, each in another group of 64; the first one's tag is
    corrupted, so the later two are resolved under another nonce than the guess (the one-lane
    repair hash and the decipher at length).  The second comes again at the end of the call and
    stays ciphertext.  A receiver whose maximum is one byte less refuses it untouched."""
    rx, model = receiver(maxb=LONG_MAXB), fresh_model([100] * N_STREAMS)
    for s in range(N_STREAMS):
        rx.reset(s, 100)
    trio = [dict(stream=1, nonce=300, nb=2, sb=0, bytes=LONG_MAXB), dict(stream=1, nonce=110, nb=1, sb=0, bytes=40000),
            dict(stream=1, nonce=111, nb=1, sb=1, bytes=LONG_MAXB)]
    w = long_factory.make(trio)
    specs = short_specs(128, list(range(2, 10)), 101)
    fill = [(s["stream"], x) for s, x in zip(specs, long_factory.make(specs))]
    items = [(1, corrupt(w[0]))] + fill[:64] + [(1, w[1])] + fill[64:] + [(1, w[2]), (1, w[1])]
    where = [i for i, (s, _) in enumerate(items) if s == 1]
    assert [i // 64 for i in where] == [0, 1, 2, 2]
    # the guess takes the first for good: the second's nonce byte would expand under 300, not under 100
    assert R.expand(300, 110 & 0xFF, 1) != 110 == R.expand(100, 110 & 0xFF, 1)
    rx.kernel_ms()
    rc, result = check_call(hip, rx, model, items, LONG_MAXB + 1, 7, maxb=LONG_MAXB)
    assert [int(rc[i]) for i in where] == [2, 0, 0, 3]
    assert [int(result["nonce"][i]) for i in where[1:]] == [110, 111, 110]
    assert rx.kernel_ms()["repaired_tags"] >= 1
    assert KEYS[1] and model[1].reg.largest == 111
    rx.close()
    small, small_model = receiver(maxb=40000 - 1), fresh_model([100] * N_STREAMS)
    for s in range(N_STREAMS):
        small.reset(s, 100)
    rc, _ = check_call(hip, small, small_model, [(1, w[1]), fill[0]], 40000 + 5, 2, maxb=40000 - 1)
    assert list(rc) == [1, 0]
    small.close()
