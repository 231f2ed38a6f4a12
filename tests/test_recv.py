"""CPU checks of the receive front (include/tonk_receive.h): the header against the library's
exports and its version script, the refusal to run without an MI355X, parameter checks that come
before any device call, the Python restatement (tests/recv_ref.py) against every recorded
transcript of the reference (tests/golden/recv_kat.txt.gz), what the fixture covers, and the byte
and state logic of the kernels (tonk_amd/csrc/recv.h) as a serial host walk --
tests/native/recv_check.cpp, plain and under the address and undefined-behaviour sanitizers, each a
stand-alone program."""
from __future__ import annotations

import ctypes
import gzip
import os
import re
import subprocess

import pytest

import recv_ref as R
from conftest import NATIVE, ROOT, _make

HEADER = os.path.join(ROOT, "include", "tonk_receive.h")
FUNCTIONS = ["tamd_recv_create", "tamd_recv_destroy", "tamd_recv_error", "tamd_recv_set_key", "tamd_recv_reset", "tamd_recv_receive",
             "tamd_recv_next_expected", "tamd_recv_state", "tamd_recv_set_timing", "tamd_recv_kernel_ms"]
N_ARGS = {"tamd_recv_set_key": 3, "tamd_recv_reset": 3, "tamd_recv_receive": 8, "tamd_recv_next_expected": 4, "tamd_recv_state": 3}


def declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#define[^\n]*", "", text)
    return set(re.findall(r"\b(tamd_recv_\w+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    import tonk_amd
    if not os.path.exists(tonk_amd.RECV_LIB_PATH):
        tonk_amd.build()
    return ctypes.CDLL(tonk_amd.RECV_LIB_PATH)


def test_header_declares_the_interface_and_the_library_exports_exactly_it(lib):
    import tonk_amd
    names = declared()
    assert names == set(FUNCTIONS)
    out = subprocess.run(["nm", "-D", "--defined-only", tonk_amd.RECV_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert exported == names, f"exports and header differ: {sorted(exported ^ names)}"
    script = open(os.path.join(ROOT, "tonk_amd", "csrc", "recv.map")).read()
    assert re.search(r"global:\s*tamd_recv_\*;\s*local:\s*\*;", script)
    text = open(HEADER).read().lower()
    # what stays with the caller
    for word in ("reliable sequence", "time synchronisation", "handshake hook", "disablesequencenumbercompress", "key exchange",
                 "asynchronous"):
        assert word in text, f"the header does not speak of {word}"


def test_engine_library_is_linked_as_before():
    """libtonk_amd.so keeps its object list: nothing of the receive front is in it."""
    mk = open(os.path.join(ROOT, "tonk_amd", "Makefile")).read()
    srcs = re.search(r"^HIP_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert "recv" not in srcs and "recv" not in re.search(r"^HOST_SRCS\s*:=(.*)$", mk, flags=re.M).group(1)
    assert re.search(r"^all:.*libtonk_amd_recv\.so", mk, flags=re.M)
    assert "--version-script=csrc/recv.map" in mk


def test_python_module_exports_datagram_receiver():
    import tonk_amd
    assert "DatagramReceiver" in tonk_amd.__all__ and "RECV_LIB_PATH" in tonk_amd.__all__
    for m in ("set_key", "reset", "receive", "next_expected", "state", "close", "kernel_ms", "set_timing"):
        assert callable(getattr(tonk_amd.DatagramReceiver, m)), m
    assert tonk_amd.DatagramReceiver.KERNEL_MS_FIELDS[-1] == "repaired_tags"


class Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("max_datagram_bytes", ctypes.c_uint32)]


def create(lib, p):
    lib.tamd_recv_create.restype = ctypes.c_void_p
    lib.tamd_recv_create.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    err = ctypes.create_string_buffer(256)
    h = lib.tamd_recv_create(ctypes.byref(p) if p is not None else None, err, 256)
    return h, err.value


def test_bad_parameters_are_refused_before_any_device_call(lib):
    for p in (None, Params(0, 0, 1500), Params(0, 4, 0), Params(0, 4, 65536)):
        h, err = create(lib, p)
        assert not h and b"bad parameters" in err, (p, err)
    lib.tamd_recv_error.restype = ctypes.c_char_p
    lib.tamd_recv_error.argtypes = [ctypes.c_void_p]
    assert lib.tamd_recv_error(None) == b"bad handle"
    for name, k in N_ARGS.items():
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        f.argtypes = None
        args = [None] * k
        if name in ("tamd_recv_set_key", "tamd_recv_reset"):
            args = [None, ctypes.c_uint32(0), ctypes.c_uint64(5)]
        if name == "tamd_recv_state":
            args = [None, ctypes.c_uint32(0), None]
        assert f(*args) == -1, name
    lib.tamd_recv_destroy.argtypes = [ctypes.c_void_p]
    lib.tamd_recv_destroy(None)
    lib.tamd_recv_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    lib.tamd_recv_kernel_ms(None, None, 9)
    import tonk_amd
    for args in ((0, 1500), (4, 0), (4, 70000)):
        with pytest.raises(RuntimeError, match="bad parameters"):
            tonk_amd.DatagramReceiver(*args)


def test_no_cpu_fallback_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h, err = create(lib, Params(0, 3, 1500))
    assert not h
    assert b"no HIP device" in err or b"gfx950" in err
    import tonk_amd
    with pytest.raises(RuntimeError, match="no HIP device|gfx950"):
        tonk_amd.DatagramReceiver(3, 1500)


def test_fixture_holds_the_cases():
    """What the transcripts are meant to pin (tests/native/recv_golden.cpp)."""
    k = R.kat()
    lines = [g for (_, _, gs) in k for g in gs]
    assert {g[6] for g in lines} == {0, 2, 3, 4} and {g[1] for g in lines} == {0, 1, 2, 3} == {g[2] for g in lines}
    assert {g[3] for g in lines} == {0, 1} and {6, 7, 24, 1306} <= {g[4] for g in lines}
    assert 0 in {key for (key, _, _) in k} and len({key for (key, _, _) in k}) >= 4
    # every width over the wraps of 0xff, 0xffff, 0xffffff (and 2^32, 2^64), both ways
    for edge in (0xff, 0xffff, 0xffffff, 0xffffffff, R.M64):
        for nb in range(4):
            gs = [g for (_, base, gs) in k if base == edge - 8 for g in gs if g[1] == nb]
            past = [g for g in gs if g[6] == 0 and g[7] == g[0] and (g[0] - edge - 1) & R.M64 < 16]
            assert past and any(g[6] == 0 and (edge - g[0]) & R.M64 < 8 for g in gs), (hex(edge), nb)
            if nb:
                assert any(g[6] == 0 and g[0] == (edge - 8 + 6) & R.M64 for g in gs), "back over the wrap"
    # gaps of exactly MSB and MSB +- 1 ahead of and behind the largest: ahead the expansion is right
    # below MSB, behind up to MSB, and 2 MSB off beyond
    for nb in (1, 2, 3):
        msb = 1 << (8 * nb - 1)
        ahead, behind = set(), set()
        for (_, base, gs) in k:
            for i, g in enumerate(gs):
                before = gs[i - 1][8] if i else base
                up, down = (g[0] - before) & R.M64, (before - g[0]) & R.M64
                if g[1] == nb and up in (msb - 1, msb, msb + 1):
                    ahead.add(up - msb)
                    assert (g[7] == g[0]) == (up < msb) and (g[7] - g[0]) & R.M64 in (0, (-2 * msb) & R.M64)
                if g[1] == nb and down in (msb - 1, msb, msb + 1):
                    behind.add(down - msb)
                    assert (g[7] == g[0]) == (down <= msb) and (g[7] - g[0]) & R.M64 in (0, 2 * msb)
        assert ahead == behind == {-1, 0, 1}, nb
    # slides of 1, 2 and 63 words, the full reset, rotation past 4096
    slides = set()
    wrapped = False
    for (_, base, gs) in k:
        prev = (base, 0)
        for g in gs:
            if g[9] != prev[0]:
                slides.add(((g[9] - prev[0]) & R.M64) // 64 if g[10] or g[9] - prev[0] < 4096 else "reset")
                wrapped = wrapped or (g[10] < prev[1] and g[10] != 0)
            prev = (g[9], g[10])
    assert {1, 2, 63, "reset"} <= slides and wrapped, slides
    # nonces below the base, repeats
    assert any(g[6] == 3 and R.less(g[7], g[9]) for g in lines)
    assert any(g[6] == 3 and not R.less(g[7], g[9]) for g in lines)
    # rc 4 both ways: older with fewer sequence than nonce bytes; older but not fewer; newest
    assert any(g[6] == 4 for g in lines)
    assert any(g[6] == 0 and 0 < g[2] and g[2] >= g[1] and R.less(g[7], g[8]) for g in lines)
    assert any(g[6] == 0 and 0 < g[2] < g[1] and g[7] == g[8] for g in lines)
    # the order case: with the middle tag corrupted the third datagram is 110 and accepted, else 366 and refused
    order = [gs for (key, base, gs) in k if base == 100 and [g[0] for g in gs[:3]] == [101, 300, 110]]
    assert sorted((gs[1][5] != 0, gs[1][6], gs[2][6], gs[2][7]) for gs in order) == [(False, 0, 2, 366), (True, 2, 0, 110)]
    assert os.path.getsize(R.KAT) < 256 * 1024


def test_python_restatement_reproduces_every_line_of_the_fixture():
    for ci, (key, base, gs) in enumerate(R.kat()):
        c = R.Connection(key, base)
        for k, g in enumerate(gs):
            d = R.wire(key, k, g[0], g[1], g[2], g[3], g[4], g[5])
            rc, res, after = c.receive(d)
            assert rc == g[6] and res["nonce"] == g[7], (ci, k, rc, res)
            assert (c.reg.largest, c.reg.base, c.reg.rotation, c.reg.window_fnv()) == g[8:12], (ci, k)
            assert R.S.fnv1a(after) == g[12], (ci, k)


@pytest.mark.parametrize("which", ["recv_check", "recv_check_san"])
def test_recv_logic_on_the_host(which, tmp_path):
    """The stand-alone walk of recv.h, plain and with the sanitizers linked in: every transcript of
    the fixture through the sequential model and through the kernels' split (1 and 16 lanes, two
    list orders, three call sizes, 16 misalignments between guards, real and arbitrary guesses),
    the invalid datagrams, and the soak, whose share of repaired guesses must be above zero."""
    _make(NATIVE, "-f", "recv.mk", f"_build/{which}")
    path = str(tmp_path / "recv_kat.txt")
    with gzip.open(R.KAT, "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    r = subprocess.run([os.path.join(NATIVE, "_build", which), path], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    n_lines = sum(len(gs) for (_, _, gs) in R.kat())
    assert int(words[1]) >= 16 * n_lines + 2 * 2000 * 64
    assert words[2] == "repaired" and float(words[3]) > 0.0
