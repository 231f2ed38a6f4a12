"""What the three batched device interfaces share (tonk_amd.DatagramSealer, DatagramFramer and
BatchCodec over tonk_amd/csrc/handle.h), on an MI355X: the launch counters and kernel times of
set_timing/kernel_ms, which the profiling tools rest on; handles of one type side by side and closed
one after the other; and calls refused as a whole, which launch nothing and leave the handle
usable.  Results are compared with the Python restatements (tests/seal_ref.py, tests/dgram_ref.py)
or, for the codec, with a second handle given the same packets.  Smallest shapes throughout."""
from __future__ import annotations

import numpy as np
import pytest

import dgram_ref as DR
import seal_ref as SR
from batch_ref import Guarded
from lz_streams import Hip

pytestmark = [pytest.mark.gpu]

FILL = Guarded.FILL
K1, K2, K3 = 0x0123456789abcdef, 0xffffffff00000001, 0x00000000deadbeef


@pytest.fixture(scope="module")
def hip():
    h = Hip()
    yield h
    h.close()


def layout(items, pitch):
    """The items' bytes at i * pitch, 0xA5 in the gaps."""
    out = np.full(max(len(items) * pitch, 1), FILL, dtype=np.uint8)
    for i, d in enumerate(items):
        out[i * pitch:i * pitch + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
    return out


def placed(hip, items, pitch, skew=0):
    buf = Guarded(hip, max(len(items) * pitch, 1), skew)
    buf.upload(layout(items, pitch))
    return buf


def helper_zero(k):
    """Every launch count, time and byte count of the helper kernels is 0 (the codec's program_*
    entries are the Device's own and are left out)."""
    return all(v == 0 for name, v in k.items() if not name.startswith("program_"))


# ---- the three interfaces' smallest calls ----

S_BYTES, S_PITCH = (7, 64, 1306), 1311
S_STREAM, S_NONCE = [0, 1, 0], [5, 1 << 33, 7]
S_MSG = [n - 6 for n in S_BYTES]


def seal_data(seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8) for n in S_BYTES]


def seal_want(data, keys):
    return layout([SR.seal(d, keys[s], n, m) for d, s, n, m in zip(data, S_STREAM, S_NONCE, S_MSG)], S_PITCH)


def seal_call(s, buf, op="seal"):
    return getattr(s, op)(S_STREAM, S_NONCE, list(S_BYTES), S_MSG, buf.ptr, S_PITCH)


D_PITCH = 64
D_GRAMS = [dict(msgs=[(6, 20)], seq=0x123456, seq_bytes=2, nonce=0xABCDEF, nonce_bytes=3, ts24=0x010203, flag_bits=DR.SEQCOMP),
           dict(msgs=[(3, 33)], seq=7, seq_bytes=0, nonce=9, nonce_bytes=1, ts24=0x040506, flag_bits=0)]


class Datagrams:
    """D_GRAMS' message bodies on the device, what build makes of them and what parse finds."""

    def __init__(self, hip, seed=2):
        rng = np.random.default_rng(seed)
        self.bodies = [rng.integers(0, 256, d["msgs"][0][1], dtype=np.uint8).tobytes() for d in D_GRAMS]
        self.src = placed(hip, self.bodies, D_PITCH, 3)
        self.addr = [self.src.ptr + i * D_PITCH for i in range(len(D_GRAMS))]
        self.built = [DR.build([(d["msgs"][0][0], b)], d["seq"], d["seq_bytes"], d["nonce"], d["nonce_bytes"], None, d["ts24"],
                               d["flag_bits"]) for d, b in zip(D_GRAMS, self.bodies)]
        assert all(r[0] == 0 for r in self.built)
        self.want = layout([r[1] for r in self.built], D_PITCH)

    def build(self, framer, out):
        g = D_GRAMS
        return framer.build([0, 1], [d["msgs"][0][0] for d in g], [d["msgs"][0][1] for d in g], self.addr, [d["seq"] for d in g],
                            [d["seq_bytes"] for d in g], [d["nonce"] for d in g], [d["nonce_bytes"] for d in g],
                            [d["ts24"] for d in g], [d["flag_bits"] for d in g], out.ptr, D_PITCH)

    def check_build(self, r, out):
        ob, mb, ro, rb, rc = r
        assert (rc == 0).all()
        for i, (_, dgram, msg, lo, n) in enumerate(self.built):
            assert (int(ob[i]), int(mb[i]), int(ro[i]), int(rb[i])) == (len(dgram), msg, lo, n), i
        out.check()
        assert (out.download() == self.want).all(), "built datagrams differ from the restatement's"

    def check_parse(self, framer, out):
        """Parse the message sections of the built datagrams in `out`."""
        st, cnt, lo, nb, table = framer.parse([r[2] for r in self.built], out.ptr, D_PITCH)
        for i, (_, dgram, msg, _, _) in enumerate(self.built):
            status, entries, rlo, rn = DR.parse(dgram[:msg])
            assert (int(st[i]), int(cnt[i]), int(lo[i]), int(nb[i])) == (status, len(entries), rlo, rn) and status == 0, i
            assert list(table[i, :len(entries)]) == entries, i


C_STREAMS, C_LEN, C_PITCH, C_RPITCH, C_ARENA = 2, 100, 103, 100 + 11 + 2, 64 << 20
C_STREAM = [0, 1, 0, 1, 0, 1]


def new_codec():
    import tonk_amd
    return tonk_amd.BatchCodec(C_STREAMS, C_LEN, C_ARENA)


def codec_packets(hip, seed=3):
    rng = np.random.default_rng(seed)
    return placed(hip, [rng.integers(0, 256, C_LEN, dtype=np.uint8) for _ in C_STREAM], C_PITCH, 1)


def codec_add(bc, src, first=0):
    pn, rc = bc.encoder_add(C_STREAM, [C_LEN] * len(C_STREAM), src.ptr, C_PITCH)
    assert (rc == 0).all() and list(pn) == [first + i // 2 for i in range(len(C_STREAM))]


def codec_encode(bc, out):
    out.fill()
    nb, rc = bc.encode([0, 1], out.ptr, C_RPITCH)
    assert (rc == 0).all() and (nb > 0).all()
    out.check()
    return nb, out.download()


# ---- 1. timing accounting ----

def test_sealer_counts_launches_always_and_times_them_when_asked(hip):
    import tonk_amd
    s = tonk_amd.DatagramSealer(2, 1500)
    try:
        s.set_key(0, K1)
        s.set_key(1, K2)
        data = seal_data()
        buf = placed(hip, data, S_PITCH, 2)
        for timed in (False, True):
            s.set_timing(timed)
            buf.upload(layout(data, S_PITCH))
            assert (seal_call(s, buf) == 0).all()
            k = s.kernel_ms()
            print("sealer", timed, k)
            assert k["packets_launches"] == 1 and k["footers_launches"] == 0 and k["footers_ms"] == 0
            assert k["packets_ms"] > 0 if timed else k["packets_ms"] == 0
            assert s.footers(list(S_BYTES), buf.ptr, S_PITCH).shape == (3, 24)
            k = s.kernel_ms()
            print("sealer", timed, k)
            assert k["footers_launches"] == 1 and k["packets_launches"] == 0 and k["packets_ms"] == 0
            assert k["footers_ms"] > 0 if timed else k["footers_ms"] == 0
            assert helper_zero(s.kernel_ms())
        buf.check()
        assert (buf.download() == seal_want(data, [K1, K2])).all()
        # n == 0: empty results, nothing launched
        assert s.seal([], [], [], [], buf.ptr, S_PITCH).size == 0 and s.open([], [], [], [], buf.ptr, S_PITCH).size == 0
        assert s.tag([], [], [], buf.ptr, S_PITCH).size == 0 and s.footers([], buf.ptr, S_PITCH).shape == (0, 24)
        s.cipher([], [], [], buf.ptr, S_PITCH)
        assert helper_zero(s.kernel_ms())
        # seal, open, cipher and tag are all launches of the packets kernel
        assert (seal_call(s, buf, "open") == 0).all() and (seal_call(s, buf) == 0).all()
        s.cipher(S_STREAM, S_NONCE, S_MSG, buf.ptr, S_PITCH)
        assert s.tag(S_STREAM, S_NONCE, list(S_BYTES), buf.ptr, S_PITCH).size == 3
        k = s.kernel_ms()
        assert k["packets_launches"] == 4 and k["footers_launches"] == 0 and k["packets_ms"] > 0
        buf.check()
    finally:
        s.close()


def test_framer_counts_launches_always_and_times_them_when_asked(hip):
    import tonk_amd
    f = tonk_amd.DatagramFramer(1500)
    try:
        d = Datagrams(hip)
        out = Guarded(hip, len(D_GRAMS) * D_PITCH, 5)
        for timed in (False, True):
            f.set_timing(timed)
            out.fill()
            d.check_build(d.build(f, out), out)
            k = f.kernel_ms()
            print("framer", timed, k)
            assert k["build_launches"] == 1 and k["parse_launches"] == 0 and k["parse_ms"] == 0
            assert k["build_ms"] > 0 if timed else k["build_ms"] == 0
            d.check_parse(f, out)
            k = f.kernel_ms()
            print("framer", timed, k)
            assert k["parse_launches"] == 1 and k["build_launches"] == 0 and k["build_ms"] == 0
            assert k["parse_ms"] > 0 if timed else k["parse_ms"] == 0
            assert helper_zero(f.kernel_ms())
        assert all(x.size == 0 for x in f.build([], [], [], [], [], [], [], [], [], [], out.ptr, D_PITCH))
        assert all(x.size == 0 for x in f.parse([], out.ptr, D_PITCH))
        assert helper_zero(f.kernel_ms())
        d.src.check()
    finally:
        f.close()


def test_codec_counts_launches_always_and_times_them_when_asked(hip):
    bc = new_codec()
    try:
        src = codec_packets(hip)
        out = Guarded(hip, 2 * C_RPITCH, 3)
        for first, timed in ((0, False), (3, True)):
            bc.set_timing(timed)
            bc.kernel_ms()
            codec_add(bc, src, first)
            k = bc.kernel_ms()
            print("codec", timed, k)
            assert k["frame_launches"] == 1 and k["frame_bytes"] == len(C_STREAM) * C_LEN
            assert k["unframe_launches"] == 0 and k["tails_launches"] == 0
            assert k["frame_ms"] > 0 if timed else k["frame_ms"] == 0
            nb, _ = codec_encode(bc, out)
            k = bc.kernel_ms()
            print("codec", timed, k)
            assert k["unframe_launches"] == 1 and k["unframe_bytes"] == int(nb.sum()) and k["frame_launches"] == 0
            assert k["unframe_ms"] > 0 if timed else k["unframe_ms"] == 0
            assert k["program_launches"] >= 1 and k["program_ms"] > 0 if timed else k["program_ms"] == 0
            rc = bc.decoder_add_recovery([0, 1], nb, out.ptr, C_RPITCH)
            assert (rc == 0).all()
            k = bc.kernel_ms()
            print("codec", timed, k)
            assert k["tails_launches"] == 1 and k["unframe_launches"] == 0
            assert k["frame_launches"] == 1 and k["frame_bytes"] == int(nb.sum())  # (the packets kept go into rows)
            assert k["tails_ms"] > 0 if timed else k["tails_ms"] == 0
            assert helper_zero(bc.kernel_ms())
        # n == 0: empty results, nothing launched
        assert all(x.size == 0 for x in bc.encoder_add([], [], src.ptr, C_PITCH))
        assert all(x.size == 0 for x in bc.encode([], out.ptr, C_RPITCH))
        assert bc.decoder_add_original([], [], [], src.ptr, C_PITCH).size == 0
        assert bc.decoder_add_recovery([], [], out.ptr, C_RPITCH).size == 0
        assert all(x.size == 0 for x in bc.decode([], out.ptr, C_PITCH, 4))
        assert helper_zero(bc.kernel_ms())
        src.check()
    finally:
        bc.close()


# ---- 2. lifetimes ----

def test_two_sealers_keep_their_own_keys_and_outlive_each_other(hip):
    import tonk_amd
    a, b = tonk_amd.DatagramSealer(2, 1500), tonk_amd.DatagramSealer(2, 1500)
    try:
        data = seal_data(4)
        a.set_key(0, K1)
        b.set_key(0, K2)
        a.set_key(1, K3)  # (b's stream 1 keeps the zero key)
        ba, bb = placed(hip, data, S_PITCH, 1), placed(hip, data, S_PITCH, 6)
        assert (seal_call(a, ba) == 0).all() and (seal_call(b, bb) == 0).all()
        ba.check()
        bb.check()
        assert (ba.download() == seal_want(data, [K1, K3])).all() and (bb.download() == seal_want(data, [K2, 0])).all()
        a.set_key(0, K3)  # a key set on one handle between the other's calls
        assert (seal_call(b, bb, "open") == 0).all() and (seal_call(a, ba, "open") != 0).any()
        sealed = [SR.seal(d, (K2, 0)[s], n, m) for d, s, n, m in zip(data, S_STREAM, S_NONCE, S_MSG)]
        back = [np.concatenate([d[:-2], s[-2:]]) for d, s in zip(data, sealed)]  # (the tag stays)
        assert (bb.download() == layout(back, S_PITCH)).all()
        a.close()
        bb.upload(layout(data, S_PITCH))
        assert (seal_call(b, bb) == 0).all()
        assert (bb.download() == seal_want(data, [K2, 0])).all()
        a.close()
    finally:
        a.close()
        b.close()
        b.close()


def test_two_framers_side_by_side_and_one_after_the_other(hip):
    import tonk_amd
    f1, f2 = tonk_amd.DatagramFramer(1500), tonk_amd.DatagramFramer(100)
    try:
        d1, d2 = Datagrams(hip, 5), Datagrams(hip, 6)
        o1, o2 = Guarded(hip, 2 * D_PITCH, 2), Guarded(hip, 2 * D_PITCH, 7)
        r1 = d1.build(f1, o1)
        r2 = d2.build(f2, o2)
        d1.check_build(r1, o1)
        d2.check_build(r2, o2)
        d2.check_parse(f2, o2)
        d1.check_parse(f1, o1)
        f1.close()
        o2.fill()
        d1.check_build(d1.build(f2, o2), o2)
        d1.check_parse(f2, o2)
        f1.close()
    finally:
        f1.close()
        f2.close()
        f2.close()


def test_two_codecs_side_by_side_and_one_after_the_other(hip):
    c1, c2 = new_codec(), new_codec()
    try:
        src = codec_packets(hip, 7)
        o1, o2 = Guarded(hip, 2 * C_RPITCH, 0), Guarded(hip, 2 * C_RPITCH, 4)
        codec_add(c1, src)
        codec_add(c2, src)
        nb1, r1 = codec_encode(c1, o1)
        nb2, r2 = codec_encode(c2, o2)
        assert (nb1 == nb2).all() and (r1 == r2).all(), "two handles given the same packets disagree"
        nb1, r1 = codec_encode(c1, o1)
        c1.close()
        nb2, r2 = codec_encode(c2, o2)
        assert (nb1 == nb2).all() and (r1 == r2).all()
        c1.close()
        src.check()
    finally:
        c1.close()
        c2.close()
        c2.close()


def test_a_sealer_a_framer_and_a_codec_alive_together(hip):
    import tonk_amd
    s, f, bc = tonk_amd.DatagramSealer(2, 1500), tonk_amd.DatagramFramer(1500), new_codec()
    try:
        data, d, src = seal_data(8), Datagrams(hip, 9), codec_packets(hip, 10)
        buf, out, rec = placed(hip, data, S_PITCH), Guarded(hip, 2 * D_PITCH), Guarded(hip, 2 * C_RPITCH)
        codec_add(bc, src)
        d.check_build(d.build(f, out), out)
        assert (seal_call(s, buf) == 0).all()
        assert (buf.download() == seal_want(data, [0, 0])).all()
        codec_encode(bc, rec)
        d.check_parse(f, out)
    finally:
        s.close()
        f.close()
        bc.close()


# ---- 3. refusals ----

def test_refused_calls_launch_nothing_and_leave_the_handle_usable(hip):
    import tonk_amd
    s, f, bc, twin = tonk_amd.DatagramSealer(2, 1500), tonk_amd.DatagramFramer(1500), new_codec(), new_codec()
    try:
        data, d, src = seal_data(11), Datagrams(hip, 12), codec_packets(hip, 13)
        buf, out = placed(hip, data, S_PITCH, 3), Guarded(hip, 2 * D_PITCH, 1)
        rec, rec2 = Guarded(hip, 2 * C_RPITCH, 2), Guarded(hip, 2 * C_RPITCH, 5)
        s.set_key(0, K1)
        with pytest.raises(RuntimeError, match=r"seal refused \(rc=-2: stream id out of range\)"):
            s.seal([0, 2, 0], S_NONCE, list(S_BYTES), S_MSG, buf.ptr, S_PITCH)
        with pytest.raises(RuntimeError, match=r"open refused \(rc=-3: pitch smaller"):
            s.open(S_STREAM, S_NONCE, list(S_BYTES), S_MSG, buf.ptr, 1305)
        assert helper_zero(s.kernel_ms())
        assert (buf.download() == layout(data, S_PITCH)).all()
        assert (seal_call(s, buf) == 0).all()
        assert (buf.download() == seal_want(data, [K1, 0])).all()
        assert s.kernel_ms()["packets_launches"] == 1

        out.fill()
        with pytest.raises(RuntimeError, match=r"build refused \(rc=-2: datagram index"):
            f.build([1, 0], [6, 6], [1, 1], d.addr, [1, 2], [1, 1], [1, 2], [1, 1], [0, 0], [0, 0], out.ptr, D_PITCH)
        with pytest.raises(RuntimeError, match=r"build refused \(rc=-3: pitch too small\)"):
            f.build([0, 1], [6, 6], [1, 1], d.addr, [1, 2], [1, 1], [1, 2], [1, 1], [0, 0], [0, 0], out.ptr, 5)
        with pytest.raises(RuntimeError, match=r"parse refused \(rc=-3: pitch too small\)"):
            f.parse([40, 41], out.ptr, 40)
        assert helper_zero(f.kernel_ms()) and (out.download() == FILL).all()
        d.check_build(d.build(f, out), out)
        d.check_parse(f, out)
        k = f.kernel_ms()
        assert k["build_launches"] == 1 and k["parse_launches"] == 1

        bc.kernel_ms()
        with pytest.raises(RuntimeError, match=r"encoder_add refused \(rc=-2: stream id out of range\)"):
            bc.encoder_add([0, 2], [C_LEN] * 2, src.ptr, C_PITCH)
        with pytest.raises(RuntimeError, match=r"encoder_add refused \(rc=-3: pitch smaller"):
            bc.encoder_add([0, 1], [C_LEN] * 2, src.ptr, C_LEN - 1)
        with pytest.raises(RuntimeError, match=r"encode refused \(rc=-3: pitch smaller"):
            bc.encode([0, 1], rec.ptr, C_LEN)
        assert helper_zero(bc.kernel_ms())
        codec_add(bc, src)
        codec_add(twin, src)
        nb, r = codec_encode(bc, rec)
        nb2, r2 = codec_encode(twin, rec2)
        assert (nb == nb2).all() and (r == r2).all(), "a handle that refused calls encodes differently"
        k = bc.kernel_ms()
        assert k["frame_launches"] == 1 and k["unframe_launches"] == 1
        buf.check()
        src.check()
    finally:
        s.close()
        f.close()
        bc.close()
        twin.close()
