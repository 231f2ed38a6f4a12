"""CPU checks of datagram building and parsing (include/tonk_datagram.h): the header and the
library's exports, the refusal to run without an MI355X, parameter checks that come before any
device call, the Python restatement (tests/dgram_ref.py) against every recorded result of the
reference (tests/golden/dgram_kat.txt.gz), the byte logic of the kernels (tonk_amd/csrc/dgram.h) as
a serial host walk -- tests/native/dgram_check.cpp, plain and under the address and
undefined-behaviour sanitizers, each a stand-alone program -- and the offset forms of the two add
calls of include/tonk_batch.h."""
from __future__ import annotations

import ctypes
import gzip
import os
import re
import subprocess

import pytest

import dgram_ref as R
from batch_ref import LENGTHS
from conftest import NATIVE, ROOT, _make

HEADER = os.path.join(ROOT, "include", "tonk_datagram.h")
FUNCTIONS = ["tamd_dgram_create", "tamd_dgram_destroy", "tamd_dgram_error", "tamd_dgram_build", "tamd_dgram_parse",
             "tamd_dgram_set_timing", "tamd_dgram_kernel_ms"]
N_ARGS = {"tamd_dgram_build": 22, "tamd_dgram_parse": 13}
BODY_LENGTHS = {0, 1, 2, 13, 14, 15, 16, 17, 18, 29, 30, 31, 32, 33, 1300, 2047}


def declared(path, prefix):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#define[^\n]*", "", text)
    return set(re.findall(r"\b(" + prefix + r"\w+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    import tonk_amd
    if not os.path.exists(tonk_amd.LIB_PATH):
        tonk_amd.build()
    return ctypes.CDLL(tonk_amd.LIB_PATH)


def test_header_declares_the_interface_and_the_library_exports_it(lib):
    names = declared(HEADER, "tamd_dgram_")
    for n in FUNCTIONS:
        assert n in names, n
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, f"declared in tonk_datagram.h but not exported: {missing}"
    text = " ".join(open(HEADER).read().lower().split())
    # what stays with the caller
    for word in ("expansion", "reliable data sent with no sequence number", "anti-replay", "delivery", "decompression",
                 "onlyfec datagrams are not parsed", "asynchronous"):
        assert word in text, f"the header does not speak of {word}"


def test_python_module_exports_datagram_framer():
    import tonk_amd
    assert "DatagramFramer" in tonk_amd.__all__
    for m in ("build", "parse", "set_timing", "kernel_ms", "close"):
        assert callable(getattr(tonk_amd.DatagramFramer, m)), m


class Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("max_datagram_bytes", ctypes.c_uint32)]


def create(lib, p):
    lib.tamd_dgram_create.restype = ctypes.c_void_p
    lib.tamd_dgram_create.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    err = ctypes.create_string_buffer(256)
    h = lib.tamd_dgram_create(ctypes.byref(p) if p is not None else None, err, 256)
    return h, err.value


def test_bad_parameters_are_refused_before_any_device_call(lib):
    """Null, a datagram size below 8 or above 65535: "bad parameters" with or without a GPU (the
    check comes first); every call on a null handle is refused as a whole."""
    for p in (None, Params(0, 0), Params(0, 7), Params(0, 65536)):
        h, err = create(lib, p)
        assert not h and b"bad parameters" in err, (p, err)
    lib.tamd_dgram_error.restype = ctypes.c_char_p
    lib.tamd_dgram_error.argtypes = [ctypes.c_void_p]
    assert lib.tamd_dgram_error(None) == b"bad handle"
    for name, k in N_ARGS.items():
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        f.argtypes = None
        assert f(*([None] * k)) == -1, name
    lib.tamd_dgram_destroy.argtypes = [ctypes.c_void_p]
    lib.tamd_dgram_destroy(None)
    lib.tamd_dgram_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.tamd_dgram_set_timing(None, 1)
    import tonk_amd
    for arg in (0, 7, 65536):
        with pytest.raises(RuntimeError, match="bad parameters"):
            tonk_amd.DatagramFramer(arg)


def test_no_cpu_fallback_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h, err = create(lib, Params(0, 1500))
    assert not h
    assert b"no HIP device" in err or b"gfx950" in err
    import tonk_amd
    with pytest.raises(RuntimeError, match="no HIP device|gfx950"):
        tonk_amd.DatagramFramer(1500)


def test_offset_forms_of_the_batch_adds_are_declared_and_exported(lib):
    names = declared(os.path.join(ROOT, "include", "tonk_batch.h"), "tamd_batch_")
    for name, k in (("tamd_batch_encoder_add_at", 9), ("tamd_batch_decoder_add_original_at", 9)):
        assert name in names and hasattr(lib, name), name
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        f.argtypes = None
        assert f(*([None] * k)) == -1, name
    import inspect
    import tonk_amd
    for m in ("encoder_add", "decoder_add_original"):
        assert inspect.signature(getattr(tonk_amd.BatchCodec, m)).parameters["offset"].default is None


def test_fixture_holds_the_cases():
    k = R.kat()
    B, P = k["B"], k["P"]
    plain = [b for b in B if not b["flag_bits"] & R.ONLYFEC]
    combos = {(b["seq_bytes"], b["nonce_bytes"], b["handshake"], bool(b["flag_bits"] & R.SEQCOMP)) for b in plain}
    assert len(combos) == 64
    assert {1, 2, 3, 17} <= {len(b["msgs"]) for b in plain}
    assert {n for b in plain for _, n in b["msgs"]} >= BODY_LENGTHS
    assert {b["msgs"][-1][1] for b in plain if b["msgs"][-1][0] == R.PADDING} >= BODY_LENGTHS
    assert any(b["msgs"][-1][0] == R.PADDING and b["reliable_bytes"] for b in plain)
    assert any(b["reliable_offset"] > 0 for b in plain)
    fec = [b for b in B if b["flag_bits"] & R.ONLYFEC]
    assert [b["msgs"] for b in fec] == [[(R.RAW, n)] for n in LENGTHS if n <= 4000]
    assert any(b["out_bytes"] == 65535 for b in B)
    assert sorted(p["a"] for p in P if p["gen"] == 0) == [i for i, b in enumerate(B) if not b["flag_bits"] & R.ONLYFEC]
    assert [p["a"] for p in P if p["gen"] == 1] == list(range(1401))
    assert [p["modes"][0][1] for p in P if p["gen"] == 2] == [675]
    rnd = [p for p in P if p["gen"] == 3]
    assert [p["bytes"] for p in rnd[:2]] == [0, 1] and len(rnd) == 202 and all(2 <= p["bytes"] <= 1400 for p in rnd[2:])
    errs = [p for p in P if p["gen"] == 4]
    for frames in (5, 9):
        for at in (0, frames // 2, frames - 1):
            got = {p["c"]: p for p in errs if p["a"] == frames and p["b"] == at}
            assert got[2]["modes"][0][:2] == (2, at) and got[3]["modes"][1][:2] == (3, at)
            # an AckAck of 2, 3 and 4 bytes under both sets of rules
            assert [got[c]["modes"][0][0] for c in (20, 30, 40)] == [4, 0, 4]
            assert [got[c]["modes"][1][:2] for c in (20, 30, 40)] == [(0, frames)] * 3
    assert [p["bytes"] for p in P if p["gen"] == 5] == [65535]
    assert os.path.getsize(R.KAT) < 128 * 1024


def test_python_restatement_reproduces_every_line_of_the_fixture():
    k = R.kat()
    for i, b in enumerate(k["B"]):
        rc, out, msg, lo, n = R.b_build(b)
        assert (rc, len(out), msg, lo, n) == (0, b["out_bytes"], b["message_bytes"], b["reliable_offset"], b["reliable_bytes"]), ("B", i)
        assert R.fnv1a(out) == b["fnv"], ("B", i)
    for i, p in enumerate(k["P"]):
        s = R.p_section(p, k)
        assert len(s) == p["bytes"], ("P", i)
        for mode in (0, 1):
            status, entries, lo, n = R.parse(s, mode)
            assert (status, len(entries), lo, n, R.table_fnv(entries)) == p["modes"][mode], ("P", i, mode)


def test_restatement_refuses_what_the_header_names():
    ok = lambda msgs, sb=1, fb=0, **kw: R.build(msgs, 7, sb, 9, 1, None, 5, fb, **kw)[0]
    assert ok([(6, b"x")]) == 0 and ok([(6, b"x")], sb=0) == 1
    assert ok([(32, b"x")]) == 1 and ok([(3, bytes(2048))]) == 1 and ok([(3, bytes(2047))]) == 0
    assert ok([(6, b"x"), (3, b"y")]) == 1 and ok([(6, b"x"), (4, b"\0\0")]) == 0 and ok([(6, b"x"), (4, b""), (6, b"z")]) == 1
    assert ok([(R.RAW, b"abc")], sb=0, fb=R.ONLYFEC) == 0 and ok([(R.RAW, b"abc")], sb=1, fb=R.ONLYFEC) == 1
    assert ok([(R.RAW, b"abc")], sb=0) == 1
    assert ok([(6, bytes(30))], max_bytes=40) == 0 and ok([(6, bytes(30))], max_bytes=39) == 1 and ok([(6, bytes(30))], pitch=39) == 1
    rc, out, msg, lo, n = R.build([(3, b"abcd"), (6, bytes(10)), (4, bytes(7))], 7, 2, 9, 0, None, 5, 0)
    assert (rc, msg, lo, n, len(out)) == (0, 27, 6, 12, 35)


@pytest.mark.parametrize("which", ["dgram_check", "dgram_check_san"])
def test_dgram_logic_on_the_host(which, tmp_path):
    """The stand-alone walk of dgram.h, plain and with the sanitizers linked in: every B line at 16
    source x 16 destination misalignments between guards, every P line at 16 misalignments in both
    modes with capped tables, and the refusals."""
    _make(NATIVE, "-f", "dgram.mk", f"_build/{which}")
    path = str(tmp_path / "dgram_kat.txt")
    with gzip.open(R.KAT, "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    r = subprocess.run([os.path.join(NATIVE, "_build", which), path], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    k = R.kat()
    assert int(r.stdout.split()[1]) >= len(k["B"]) + len(k["P"])
