"""CPU checks of the datagram cipher and tag (include/tonk_seal.h): the header and the library's
exports, the refusal to run without an MI355X, parameter checks that come before any device call,
the Python restatement (tests/seal_ref.py) against every recorded output of the reference
(tests/golden/seal_kat.txt.gz), and the byte logic of the kernels (tonk_amd/csrc/seal.h) as a serial
host walk -- tests/native/seal_check.cpp, plain and under the address and undefined-behaviour
sanitizers, each a stand-alone program."""
from __future__ import annotations

import ctypes
import gzip
import os
import re
import subprocess

import pytest

import seal_ref as R
from conftest import NATIVE, ROOT, _make

HEADER = os.path.join(ROOT, "include", "tonk_seal.h")
FUNCTIONS = ["tamd_seal_create", "tamd_seal_destroy", "tamd_seal_error", "tamd_seal_set_key", "tamd_seal_seal",
             "tamd_seal_open", "tamd_seal_cipher", "tamd_seal_tag", "tamd_seal_footers", "tamd_seal_set_timing",
             "tamd_seal_kernel_ms"]
N_ARGS = {"tamd_seal_set_key": 3, "tamd_seal_seal": 9, "tamd_seal_open": 9, "tamd_seal_cipher": 7, "tamd_seal_tag": 8,
          "tamd_seal_footers": 6}


def declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#define[^\n]*", "", text)
    return set(re.findall(r"\b(tamd_seal_\w+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    import tonk_amd
    if not os.path.exists(tonk_amd.LIB_PATH):
        tonk_amd.build()
    return ctypes.CDLL(tonk_amd.LIB_PATH)


def test_header_declares_the_interface_and_the_library_exports_it(lib):
    names = declared()
    for n in FUNCTIONS:
        assert n in names, n
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, f"declared in tonk_seal.h but not exported: {missing}"
    text = open(HEADER).read().lower()
    # the caller writes timestamp and flags before seal; what stays with the caller
    for word in ("before the call", "anti-replay", "strikeregister", "handshakes", "asynchronous"):
        assert word in text, f"the header does not speak of {word}"


def test_python_module_exports_datagram_sealer():
    import tonk_amd
    assert "DatagramSealer" in tonk_amd.__all__
    for m in ("set_key", "seal", "open", "cipher", "tag", "footers", "close"):
        assert callable(getattr(tonk_amd.DatagramSealer, m)), m


class Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("max_datagram_bytes", ctypes.c_uint32)]


def create(lib, p):
    lib.tamd_seal_create.restype = ctypes.c_void_p
    lib.tamd_seal_create.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    err = ctypes.create_string_buffer(256)
    h = lib.tamd_seal_create(ctypes.byref(p) if p is not None else None, err, 256)
    return h, err.value


def test_bad_parameters_are_refused_before_any_device_call(lib):
    """Null, zero streams, a datagram size of 0 or above 65535: "bad parameters" with or without a
    GPU (the check comes first); every call on a null handle is refused as a whole."""
    for p in (None, Params(0, 0, 1500), Params(0, 4, 0), Params(0, 4, 65536)):
        h, err = create(lib, p)
        assert not h and b"bad parameters" in err, (p, err)
    lib.tamd_seal_error.restype = ctypes.c_char_p
    lib.tamd_seal_error.argtypes = [ctypes.c_void_p]
    assert lib.tamd_seal_error(None) == b"bad handle"
    for name, k in N_ARGS.items():
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        f.argtypes = None
        args = [None] * k
        if name == "tamd_seal_set_key":
            args = [None, ctypes.c_uint32(0), ctypes.c_uint64(5)]
        assert f(*args) == -1, name
    lib.tamd_seal_destroy.argtypes = [ctypes.c_void_p]
    lib.tamd_seal_destroy(None)
    import tonk_amd
    for args in ((0, 1500), (4, 0), (4, 70000)):
        with pytest.raises(RuntimeError, match="bad parameters"):
            tonk_amd.DatagramSealer(*args)


def test_no_cpu_fallback_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h, err = create(lib, Params(0, 3, 1500))
    assert not h
    assert b"no HIP device" in err or b"gfx950" in err
    import tonk_amd
    with pytest.raises(RuntimeError, match="no HIP device|gfx950"):
        tonk_amd.DatagramSealer(3, 1500)


def test_fixture_holds_the_cases():
    """Every key, sequence and length the fixture is meant to pin, and every path of the hash."""
    k = R.kat()
    keys = {0, 0x0123456789abcdef, 0xffffffff00000001, 0x00000000deadbeef, 0x8000000000000000}
    seqs = {0, 1, 0xffffffff, 0x100000000, 0xabcdef0123456789}
    assert {c[0] for c in k["C"]} == keys and {c[1] for c in k["C"]} == seqs
    assert {c[2] for c in k["C"]} == set(range(131)) | {255, 256, 257, 1023, 1024, 1025, 1300, 1311, 1500, 4000, 65535}
    for n in range(41):
        assert len({(c[0], c[1]) for c in k["C"] if c[2] == n}) == 25, n
    for c in k["C"]:
        assert c[3] <= c[2]
    assert {d[0] for d in k["D"]} == keys and {6, 7, 1306, 65535} <= {d[2] for d in k["D"]}
    assert len(k["I"]) >= 5 and os.path.getsize(R.KAT) < 256 * 1024


def test_python_restatement_reproduces_every_line_of_the_fixture():
    k = R.kat()
    for (key, seq, n, msg, tag, fnv) in k["C"]:
        d = R.cipher(R.payload(n, msg), key, seq, msg)
        assert R.tag(d, key, seq) == tag and R.fnv1a(d) == fnv, ("C", hex(key), hex(seq), n, msg)
    for (key, v, tag) in k["I"]:
        assert R.tag_int(key, v) == tag, ("I", hex(key), hex(v))
    for (key, seq, n, msg, ts24, flags, fnv) in k["D"]:
        plain = R.datagram(n, msg, ts24, flags)
        d = R.seal(plain, key, seq, msg)
        assert R.fnv1a(d) == fnv, ("D", hex(key), hex(seq), n, msg)
        rc, back = R.open_(d, key, seq, msg)
        assert rc == 0 and (back[:n - 2] == plain[:n - 2]).all()


def test_closed_form_keystream_is_the_running_sum():
    """W(w) against the reference's loop as its source states it: k[i] += a[i] per 16 bytes, then a
    4-byte tail loop from k[0], then a partial word."""
    for key in (0x0123456789abcdef, 0x00000000deadbeef):
        for seq in (0, 0xabcdef0123456789):
            K, A = list(R.expand(key)), R.adder(seq)
            for n in (1, 3, 4, 15, 16, 17, 31, 37, 64, 70):
                k, out, left = list(K), [], n
                while left >= 16:
                    for i in range(4):
                        k[i] = (k[i] + A[i]) & R.M32
                        out += list(k[i].to_bytes(4, "little"))
                    left -= 16
                i = 0
                while left > 0:
                    k[i & 3] = (k[i & 3] + A[i & 3]) & R.M32
                    out += list(k[i & 3].to_bytes(4, "little"))[:min(left, 4)]
                    left -= min(left, 4)
                    i += 1
                assert bytes(out) == R.keystream(key, seq, n).tobytes(), (hex(key), hex(seq), n)


@pytest.mark.parametrize("which", ["seal_check", "seal_check_san"])
def test_seal_logic_on_the_host(which, tmp_path):
    """The stand-alone walk of seal.h, plain and with the sanitizers linked in: every C, I and D
    line of the fixture at source misalignments 0..15 between guards, every sealed datagram opened
    back to its plaintext, a damaged tag refused with nothing written, and the invalid datagrams."""
    _make(NATIVE, "-f", "seal.mk", f"_build/{which}")
    path = str(tmp_path / "seal_kat.txt")
    with gzip.open(R.KAT, "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    r = subprocess.run([os.path.join(NATIVE, "_build", which), path], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    k = R.kat()
    assert int(r.stdout.split()[1]) >= len(k["C"]) + len(k["I"]) + len(k["D"])
