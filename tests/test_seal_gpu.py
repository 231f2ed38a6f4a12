"""Seal and open of datagrams in device memory (include/tonk_seal.h, tonk_amd.DatagramSealer) on an
MI355X against the recorded outputs of the reference's SimpleCipher (tests/golden/seal_kat.txt.gz)
and, for shapes beyond the fixture, against its Python restatement (tests/seal_ref.py, itself
checked against the fixture by tests/test_seal.py).  Every caller buffer has 64 guard bytes of 0xA5
on each side, checked after every call, and the gaps between the slots of a call are compared too:
no byte outside what a call may write changes."""
from __future__ import annotations

import numpy as np
import pytest

import seal_ref as R
from batch_ref import Guarded
from lz_streams import Hip

pytestmark = [pytest.mark.gpu]

KEYS = [0, 0x0123456789abcdef, 0xffffffff00000001, 0x00000000deadbeef, 0x8000000000000000]
MAXB = 65535
FILL = Guarded.FILL
SKEWS = (0, 1, 5, 15)


@pytest.fixture(scope="module")
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def sealer():
    import tonk_amd
    s = tonk_amd.DatagramSealer(len(KEYS), MAXB)
    for i, k in enumerate(KEYS):
        s.set_key(i, k)
    yield s
    s.close()


def layout(items, pitch):
    """The items' bytes at i * pitch, 0xA5 in the gaps."""
    out = np.full(max(len(items) * pitch, 1), FILL, dtype=np.uint8)
    for i, d in enumerate(items):
        out[i * pitch:i * pitch + d.size] = d
    return out


def differing(got, want, pitch):
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    i, o = divmod(int(bad[0]), pitch)
    return f"slot {i}: {R.first_difference(got[i * pitch:(i + 1) * pitch], want[i * pitch:(i + 1) * pitch])} (offset {o})"


class Call:
    """One call's datagrams on the device between guards."""

    def __init__(self, hip, items, pitch, skew=0):
        self.pitch, self.n = pitch, len(items)
        self.buf = Guarded(hip, max(self.n * pitch, 1), skew)
        self.buf.upload(layout(items, pitch))

    def get(self):
        self.buf.check()
        return self.buf.download()


# ---- 1. the primitives against the reference ----

@pytest.fixture(scope="module")
def c_cases():
    """The C lines in two groups (up to 4000 bytes, and the 65535-byte cases, so that a call's
    slots stay small): per group the lines, the device input (plaintext where msg == len, else the
    restatement's bytes with the first msg ciphered) and the expected bytes, whose FNV is the
    fixture's."""
    groups = []
    for pick in (lambda n: n <= 4000, lambda n: n > 4000):
        lines = [c for c in R.kat()["C"] if pick(c[2])]
        given, want = [], []
        for (key, seq, n, msg, tag, fnv) in lines:
            plain = R.payload(n, msg)
            out = R.cipher(plain, key, seq, msg)
            assert R.fnv1a(out) == fnv
            given.append(plain if msg == n else out)
            want.append(out)
        groups.append((lines, given, want))
    return groups


@pytest.mark.parametrize("skew", SKEWS)
def test_cipher_and_tag_equal_the_reference(hip, sealer, c_cases, skew):
    """cipher + tag over every C case with msg == len, tag alone over the rest: one cipher call and
    one tag call per group at pitch max(len) + 11."""
    for lines, given, want in c_cases:
        pitch = max(c[2] for c in lines) + 11
        stream = [KEYS.index(c[0]) for c in lines]
        nonce = [c[1] for c in lines]
        lens = [c[2] for c in lines]
        call = Call(hip, given, pitch, skew)
        sealer.cipher(stream, nonce, [c[2] if c[3] == c[2] else 0 for c in lines], call.buf.ptr, pitch)
        got = call.get()
        msg = differing(got, layout(want, pitch), pitch)
        assert not msg, f"cipher, base misalignment {skew}: {msg}"
        tags = sealer.tag(stream, nonce, lens, call.buf.ptr, pitch)
        assert (call.get() == got).all(), "tag wrote to the data"
        bad = [i for i, c in enumerate(lines) if int(tags[i]) != c[4]]
        assert not bad, f"tag of case {lines[bad[0]]} is {int(tags[bad[0]]):#06x} ({len(bad)} differ)"


# ---- 2. whole datagrams ----

@pytest.fixture(scope="module")
def d_cases():
    groups = []
    for pick in (lambda n: n <= 4006, lambda n: n > 4006):
        lines = [d for d in R.kat()["D"] if pick(d[2])]
        plain, sealed = [], []
        for (key, seq, n, msg, ts24, flags, fnv) in lines:
            p = R.datagram(n, msg, ts24, flags)
            s = R.seal(p, key, seq, msg)
            assert R.fnv1a(s) == fnv
            plain.append(p)
            sealed.append(s)
        groups.append((lines, plain, sealed))
    return groups


@pytest.mark.parametrize("skew", (0, 5))
def test_datagrams_seal_to_the_reference_and_open_back(hip, sealer, d_cases, skew):
    for lines, plain, sealed in d_cases:
        pitch = max(d[2] for d in lines) + 11
        stream = [KEYS.index(d[0]) for d in lines]
        nonce, nbytes, msgs = [d[1] for d in lines], [d[2] for d in lines], [d[3] for d in lines]
        call = Call(hip, plain, pitch, skew)
        rc = sealer.seal(stream, nonce, nbytes, msgs, call.buf.ptr, pitch)
        assert (rc == 0).all()
        msg = differing(call.get(), layout(sealed, pitch), pitch)
        assert not msg, f"seal: {msg}"
        rc = sealer.open(stream, nonce, nbytes, msgs, call.buf.ptr, pitch)
        assert (rc == 0).all(), f"open refused {np.flatnonzero(rc)[:5]}"
        back = [np.concatenate([p[:-2], s[-2:]]) for p, s in zip(plain, sealed)]  # (the tag stays)
        msg = differing(call.get(), layout(back, pitch), pitch)
        assert not msg, f"open: {msg}"


# ---- 3. grouping ----

def mixed(n, seed):
    """n datagrams: bytes 6, 7, 38, 39, 70, 1306, 4006 in turn, message_bytes 0, T, T - 12,
    streams (and so keys, the zero key among them) interleaved."""
    rng = np.random.default_rng(seed)
    sizes = (6, 7, 38, 39, 70, 1306, 4006)
    items = []
    for i in range(n):
        nb = sizes[i % 7]
        T = nb - 6
        msg = (0, T, max(T - 12, 0))[(i // 7 + i) % 3]
        items.append(dict(stream=(i * 3 + i // 5) % len(KEYS), nonce=int(rng.integers(0, 2**63)) * 2 + (i & 1), bytes=nb,
                          msg=msg, data=rng.integers(0, 256, nb, dtype=np.uint8)))
    return items


def ref_seal(it):
    return R.seal(it["data"], KEYS[it["stream"]], it["nonce"], it["msg"])


def fields(items):
    return ([it["stream"] for it in items], [it["nonce"] for it in items], [it["bytes"] for it in items],
            [it["msg"] for it in items])


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129))
def test_groups_of_mixed_datagrams(hip, sealer, n):
    items = mixed(n, 100 + n)
    pitch = 4006 + 3
    call = Call(hip, [it["data"] for it in items], pitch, 3)
    rc = sealer.seal(*fields(items), call.buf.ptr, pitch)
    assert (rc == 0).all()
    sealed = [ref_seal(it) for it in items]
    msg = differing(call.get(), layout(sealed, pitch), pitch)
    assert not msg, f"seal of {n}: {msg}"
    zero = [i for i, it in enumerate(items) if KEYS[it["stream"]] == 0]
    for i in zero:  # no cipher under the zero key, and still a tag
        assert (sealed[i][:-2] == items[i]["data"][:-2]).all()
    assert zero or n == 1
    rc = sealer.open(*fields(items), call.buf.ptr, pitch)
    assert (rc == 0).all()
    back = [np.concatenate([it["data"][:-2], s[-2:]]) for it, s in zip(items, sealed)]
    msg = differing(call.get(), layout(back, pitch), pitch)
    assert not msg, f"open of {n}: {msg}"


# ---- 4. shared boundaries ----

@pytest.mark.parametrize("n,nb", ((130, 37), (66, 1301)))
def test_datagrams_back_to_back_share_dwords_and_granules(hip, sealer, n, nb):
    """Pitch = bytes, odd: every boundary between two datagrams falls inside a dword."""
    rng = np.random.default_rng(nb)
    T = nb - 6
    items = [dict(stream=1 + i % 4, nonce=1000 + i, bytes=nb, msg=(T, T - 12, T - 1)[i % 3],
                  data=rng.integers(0, 256, nb, dtype=np.uint8)) for i in range(n)]
    for skew in (0, 7):
        call = Call(hip, [it["data"] for it in items], nb, skew)
        rc = sealer.seal(*fields(items), call.buf.ptr, nb)
        assert (rc == 0).all()
        sealed = [ref_seal(it) for it in items]
        msg = differing(call.get(), layout(sealed, nb), nb)
        assert not msg, f"seal: {msg}"
        rc = sealer.open(*fields(items), call.buf.ptr, nb)
        assert (rc == 0).all()
        back = [np.concatenate([it["data"][:-2], s[-2:]]) for it, s in zip(items, sealed)]
        msg = differing(call.get(), layout(back, nb), nb)
        assert not msg, f"open: {msg}"


# ---- 5. rejections ----

def test_damaged_datagrams_are_refused_and_left_alone(hip, sealer):
    rng = np.random.default_rng(5)
    nb, pitch = 1306, 1311
    T = nb - 6
    base = [dict(stream=1 + i % 3, nonce=(7 << 32) + 50 + i, bytes=nb, msg=T - 12, data=rng.integers(0, 256, nb, dtype=np.uint8))
            for i in range(24)]
    sealed = [ref_seal(it) for it in base]
    given = [s.copy() for s in sealed]
    items = [dict(it) for it in base]
    # odd slots are damaged, each in its own way; even slots are their untouched neighbours
    for k, at in enumerate((0, T - 1, T, T + 2, T + 3, T + 4, T + 5)):
        given[2 * k + 1][at] ^= 1 << (k % 8)
    items[15]["nonce"] += 1
    items[17]["nonce"] ^= 1 << 32
    items[19]["stream"] = 1 + (items[19]["stream"] % 3)  # another stream's key
    assert KEYS[items[19]["stream"]] != KEYS[base[19]["stream"]]
    bad = [1, 3, 5, 7, 9, 11, 13, 15, 17, 19]
    call = Call(hip, given, pitch, 9)
    rc = sealer.open(*fields(items), call.buf.ptr, pitch)
    want_rc = np.zeros(len(items), dtype=np.int32)
    want_rc[bad] = 2
    assert (rc == want_rc).all(), rc
    want = [given[i] if i in bad else np.concatenate([base[i]["data"][:-2], sealed[i][-2:]]) for i in range(len(items))]
    msg = differing(call.get(), layout(want, pitch), pitch)
    assert not msg, msg


def test_invalid_datagrams_and_refused_calls(hip, sealer):
    import tonk_amd
    rng = np.random.default_rng(6)
    small = tonk_amd.DatagramSealer(2, 100)
    try:
        small.set_key(0, KEYS[1])
        small.set_key(1, KEYS[2])
        pitch = 128
        nbytes = [5, 40, 101, 40, 0]
        msgs = [0, 35, 10, 34, 0]  # bytes < 6; message_bytes = T + 1; bytes > max; valid; bytes 0
        data = [rng.integers(0, 256, max(n, 1), dtype=np.uint8)[:n] for n in nbytes]
        for op in (small.seal, small.open):
            call = Call(hip, data, pitch, 2)
            rc = op([0, 1, 0, 1, 0], [1, 2, 3, 4, 5], nbytes, msgs, call.buf.ptr, pitch)
            assert list(rc) == [1, 1, 1, 0 if op == small.seal else 2, 1], rc
            want = list(data)
            if op == small.seal:
                want[3] = R.seal(data[3], KEYS[2], 4, 34)
            msg = differing(call.get(), layout(want, pitch), pitch)
            assert not msg, msg
        call = Call(hip, data, pitch)
        before = call.get()
        with pytest.raises(RuntimeError, match="stream id out of range"):
            small.seal([0, 2], [1, 2], [40, 40], [0, 0], call.buf.ptr, pitch)
        with pytest.raises(RuntimeError, match="pitch smaller"):
            small.open([0, 1], [1, 2], [40, 41], [0, 0], call.buf.ptr, 40)
        with pytest.raises(RuntimeError, match="pitch smaller"):
            small.cipher([0], [1], [50], call.buf.ptr, 49)
        with pytest.raises(RuntimeError, match="stream id out of range"):
            small.tag([5], [1], [50], call.buf.ptr, pitch)
        with pytest.raises(RuntimeError, match="stream id out of range"):
            small.set_key(2, 1)
        assert (call.get() == before).all()
        # a refused call leaves the handle usable
        assert list(small.seal([0], [1], [40], [34], call.buf.ptr, pitch)) == [0]
    finally:
        small.close()


# ---- 6. keys ----

def test_set_key_changes_the_next_call_only_for_its_stream(hip):
    import tonk_amd
    rng = np.random.default_rng(8)
    s = tonk_amd.DatagramSealer(3, 1500)
    try:
        nb, pitch = 70, 75
        data = [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(3)]
        keys = [0, 0, 0]  # a fresh stream's key is 0
        for change in (None, (1, KEYS[1]), (2, KEYS[3]), (1, KEYS[2]), (1, 0)):
            if change:
                s.set_key(*change)
                keys[change[0]] = change[1]
            call = Call(hip, data, pitch, 1)
            rc = s.seal([0, 1, 2], [11, 12, 13], [nb] * 3, [nb - 6] * 3, call.buf.ptr, pitch)
            assert (rc == 0).all()
            want = [R.seal(data[i], keys[i], 11 + i, nb - 6) for i in range(3)]
            msg = differing(call.get(), layout(want, pitch), pitch)
            assert not msg, f"after {change}: {msg}"
    finally:
        s.close()


# ---- 7. footers ----

def test_footers_are_right_aligned_and_zero_filled(hip, sealer):
    rng = np.random.default_rng(9)
    nbytes = [1, 6, 23, 24, 25, 1306]
    pitch = 1311
    data = [rng.integers(0, 256, n, dtype=np.uint8) for n in nbytes]
    call = Call(hip, data, pitch, 13)
    got = sealer.footers(nbytes, call.buf.ptr, pitch)
    assert got.shape == (len(nbytes), 24)
    for i, d in enumerate(data):
        want = np.zeros(24, dtype=np.uint8)
        tl = min(d.size, 24)
        want[24 - tl:] = d[d.size - tl:]
        assert (got[i] == want).all(), (nbytes[i], got[i], want)
    assert (call.get() == layout(data, pitch)).all()
