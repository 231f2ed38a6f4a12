"""CPU checks of the batched codecs over the caller's device packets (include/tonk_batch.h):
the header and the library's exports, the refusal to run without an MI355X, parameter checks that
come before any device call, and the byte logic of the framing kernels (tonk_amd/csrc/frame.h) as
a host walk over 1, 64, 128 and 256 lanes -- tests/native/frame_check.cpp, plain and under the
address and undefined-behaviour sanitizers, each a stand-alone program."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import NATIVE, ROOT, _make, length_header

HEADER = os.path.join(ROOT, "include", "tonk_batch.h")
FUNCTIONS = ["tamd_batch_create", "tamd_batch_destroy", "tamd_batch_error", "tamd_batch_encoder_add", "tamd_batch_encode",
             "tamd_batch_encoder_ack", "tamd_batch_decoder_add_original", "tamd_batch_decoder_add_recovery",
             "tamd_batch_decode", "tamd_batch_decoder_ack"]
# frame_check.cpp's cases
LENS = [1, 2, 15, 16, 17, 63, 64, 127, 128, 129, 1023, 1024, 1025, 1300, 1535, 1536, 1537, 4000, 16383, 16384, 65535]


def declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#define[^\n]*", "", text)
    return set(re.findall(r"\b(tamd_batch_\w+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    import tonk_amd
    if not os.path.exists(tonk_amd.LIB_PATH):
        tonk_amd.build()
    return ctypes.CDLL(tonk_amd.LIB_PATH)


def frame_check(which="frame_check"):
    _make(NATIVE, "-f", "frame.mk", f"_build/{which}")
    return os.path.join(NATIVE, "_build", which)


def test_header_declares_the_interface_and_the_library_exports_it(lib):
    names = declared()
    for n in FUNCTIONS:
        assert n in names, n
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, f"declared in tonk_batch.h but not exported: {missing}"
    text = open(HEADER).read()
    for word in ("retransmit", "remove_before", "pipelining", "zero-copy", "Worker pools".lower()):
        assert word in text.lower(), f"the header does not say that {word} is out of scope"


def test_python_module_exports_batch_codec():
    import tonk_amd
    assert "BatchCodec" in tonk_amd.__all__
    for m in ("encoder_add", "encode", "encoder_ack", "decoder_add_original", "decoder_add_recovery", "decode",
              "decoder_ack", "close"):
        assert callable(getattr(tonk_amd.BatchCodec, m)), m


class Params(ctypes.Structure):
    _fields_ = [("device", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("max_packet_bytes", ctypes.c_uint32),
                ("arena_bytes", ctypes.c_uint64)]


def create(lib, p):
    lib.tamd_batch_create.restype = ctypes.c_void_p
    lib.tamd_batch_create.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    err = ctypes.create_string_buffer(256)
    h = lib.tamd_batch_create(ctypes.byref(p) if p is not None else None, err, 256)
    return h, err.value


def test_bad_parameters_are_refused_before_any_device_call(lib):
    """Null, zero streams, a packet size of 0 or above 65535, no arena: "bad parameters" with or
    without a GPU (the check comes first)."""
    for p in (None, Params(0, 0, 1300, 64 << 20), Params(0, 4, 0, 64 << 20), Params(0, 4, 65536, 64 << 20),
              Params(0, 4, 1300, 0)):
        h, err = create(lib, p)
        assert not h and b"bad parameters" in err, (p, err)
    h, err = create(lib, None)
    lib.tamd_batch_error.restype = ctypes.c_char_p
    lib.tamd_batch_error.argtypes = [ctypes.c_void_p]
    assert lib.tamd_batch_error(None) == b"bad handle"
    # calls on a null handle are refused as a whole
    for name in FUNCTIONS[3:]:
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        assert f(*([None] * 11)[:{"tamd_batch_encoder_add": 8, "tamd_batch_encode": 7, "tamd_batch_encoder_ack": 5,
                                 "tamd_batch_decoder_add_original": 8, "tamd_batch_decoder_add_recovery": 7,
                                 "tamd_batch_decode": 11, "tamd_batch_decoder_ack": 5}[name]]) == -1, name
    import tonk_amd
    for args in ((0, 1300, 64 << 20), (4, 0, 64 << 20), (4, 70000, 64 << 20), (4, 1300, 0)):
        with pytest.raises(RuntimeError, match="bad parameters"):
            tonk_amd.BatchCodec(*args)


def test_no_cpu_fallback_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h, err = create(lib, Params(0, 3, 4000, 64 << 20))
    assert not h
    assert b"no HIP device" in err or b"gfx950" in err
    import tonk_amd
    with pytest.raises(RuntimeError, match="no HIP device|gfx950"):
        tonk_amd.BatchCodec(3, 4000, 64 << 20)


def expected_rows():
    """The framed rows frame_check writes: length_header(len) || payload || zeros to the row's
    capacity, payload byte i of case (len, mis) = i * 131 + len * 7 + mis * 13 + 1."""
    out = []
    for n in LENS:
        i = np.arange(n, dtype=np.uint32)
        cap = (n + 3 + 63) // 64 * 64
        for mis in range(16):
            hdr = np.frombuffer(length_header(n), dtype=np.uint8)
            row = np.zeros(cap, dtype=np.uint8)
            row[:hdr.size] = hdr
            row[hdr.size:hdr.size + n] = (i * 131 + n * 7 + mis * 13 + 1).astype(np.uint8)
            out.append(row)
    return np.concatenate(out)


@pytest.mark.parametrize("which", ["frame_check", "frame_check_san"])
def test_frame_logic_on_the_host(which, tmp_path):
    """The stand-alone walk, plain and with the sanitizers linked in: header round trips for every
    length 1..70000, framing and unframing over the lengths x source misalignments 0..15 with one
    lane and with the 64, 128 and 256 lanes of one, two and four waves, the rejections with nothing
    written, every byte written by exactly one lane, the launch shape's (packet, lane) cover; its
    headers and framed rows against the oracle's."""
    exe = frame_check(which)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert int(r.stdout.split()[1]) >= 4 * len(LENS) * 16 + 15  # (four lane counts; 3 x 5 launch shapes)

    path = str(tmp_path / "headers.bin")
    r = subprocess.run([exe, "headers", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    got = np.fromfile(path, dtype=np.uint8).reshape(-1, 4)
    assert got.shape[0] == 70000
    for n in range(1, 70001):
        h = length_header(n)
        assert got[n - 1, 0] == len(h) and got[n - 1, 1:1 + len(h)].tobytes() == h, n

    path = str(tmp_path / "rows.bin")
    r = subprocess.run([exe, "rows", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    got, want = np.fromfile(path, dtype=np.uint8), expected_rows()
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first differing byte of the framed rows at {bad[0]}"
