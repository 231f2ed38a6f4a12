"""CPU checks of the stateful batched compressor and decompressor (include/tonk_compress_batch.h):
the placement kernel's byte logic (tonk_amd/csrc/lz_place.h) and the pass planner
(tonk_amd/csrc/lz_pass.h) as a stand-alone host program -- tests/native/cbatch_check.cpp, plain
and under the address and undefined-behaviour sanitizers -- the header's prototypes against the
Python binding, the class's single base, and the refusals that come before any device call."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import pytest

from conftest import NATIVE, ROOT, _make

HEADER = "tonk_compress_batch.h"
PREFIX = "tamd_cbatch"
N_ARGS = {"tamd_cbatch_compress": 8, "tamd_cbatch_decompress": 10, "tamd_cbatch_reset": 4}
COMMON = {"create": 3, "destroy": 1, "error": 1, "set_timing": 2, "kernel_ms": 3}


class Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("device", "n_streams", "max_message_bytes", "sides", "abut")]


def prototypes(header, prefix):
    """name -> parameter count of every function the header declares."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*|#define[^\n]*", "", text)
    return {name: params.count(",") + 1 for name, params in re.findall(r"\b(" + prefix + r"_\w+)\s*\(([^()]*)\)\s*;", text)}


@pytest.fixture(scope="module")
def lib():
    import tonk_amd
    if not os.path.exists(tonk_amd.CBATCH_LIB_PATH):
        tonk_amd.build()
    return ctypes.CDLL(tonk_amd.CBATCH_LIB_PATH)


@pytest.mark.parametrize("what", ["place", "plan"])
@pytest.mark.parametrize("which", ["cbatch_check", "cbatch_check_san"])
def test_cbatch_logic_on_the_host(which, what):
    """place: three abutting messages of a stream from sources of their own, by 1 and 16 lanes in
    either order, at 16 source offsets x 16 slot phases x ten lengths x slots inside the ring,
    across its end and inside the mirrored first 64 bytes, against a memcpy model between guards.
    plan: seeded random calls; every item in one pass, per-stream order, positions equal to
    RingTracks stepped one by one, and no window byte overwritten within its pass."""
    _make(NATIVE, "-f", "cbatch.mk", f"_build/{which}")
    r = subprocess.run([os.path.join(NATIVE, "_build", which), what], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    # place: 10 lengths x 9 slot bases x 16 phases x 16 source offsets; plan: 3 maxima x 2 caps x 8 rounds x 3 calls
    assert int(r.stdout.split()[1]) == (10 * 9 * 16 * 16 if what == "place" else 3 * 2 * 8 * 3)


def test_every_function_of_the_header_is_bound_with_its_parameter_count():
    import tonk_amd
    if not os.path.exists(tonk_amd.CBATCH_LIB_PATH):
        tonk_amd.build()
    L = tonk_amd.lib(tonk_amd.CBATCH_LIB_PATH)
    want = dict(N_ARGS, **{f"{PREFIX}_{name}": k for name, k in COMMON.items()})
    assert prototypes(HEADER, PREFIX) == want, "the header's prototypes and the test's table differ"
    klass = tonk_amd.BatchCompressor
    klass._bind()
    for name, k in want.items():
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == k, name
    # a second bind is a no-op: a prototype changed by hand in between stays as it is
    f = getattr(L, f"{PREFIX}_error")
    kept = f.argtypes
    f.argtypes = None
    try:
        klass._bind()
        assert f.argtypes is None
    finally:
        f.argtypes = kept


def test_the_class_has_the_one_base_and_none_of_its_methods():
    import tonk_amd
    from tonk_amd._handle import Handle
    cls = tonk_amd.BatchCompressor
    assert "BatchCompressor" in tonk_amd.__all__
    assert cls.__bases__ == (Handle,)
    for name in ("set_timing", "kernel_ms", "close", "__del__", "_check", "_create"):
        assert name not in vars(cls) and callable(getattr(cls, name)), name
    for name in ("compress", "decompress", "reset"):
        assert callable(getattr(cls, name)), name
    assert len(cls.KERNEL_MS_FIELDS) >= 4 and cls._REFUSED.keys() == {-1, -2, -3, -4}
    assert cls.KERNEL_MS_FIELDS[:3] == ("place_ms", "compress_ms", "decompress_ms")


def test_header_states_the_contract_and_the_library_exports_it(lib):
    for name in list(N_ARGS) + [f"{PREFIX}_{n}" for n in COMMON]:
        assert hasattr(lib, name), name
    text = " ".join(open(os.path.join(ROOT, "include", HEADER)).read().lower().split())
    for word in ("send as is", "32 readable bytes", "overlaps", "insertuncompressed", "-13", "-14", "4 gib", "asynchronous",
                 "tamd_compressor_compress"):
        assert word in text, f"the header does not speak of {word}"
    # the sides' bits as the Python module has them
    from tonk_amd import cbatch
    defs = dict(re.findall(r"#define (TAMD_CBATCH_\w+) (\d+)u", open(os.path.join(ROOT, "include", HEADER)).read()))
    assert {k: int(v) for k, v in defs.items()} == {"TAMD_CBATCH_COMPRESS": cbatch.COMPRESS, "TAMD_CBATCH_DECOMPRESS": cbatch.DECOMPRESS}


def test_library_exports_the_interface_only():
    """libtonk_amd_cbatch.so carries the compression kernels a second time: their host stubs stay
    local, so a program that links it beside libtonk_amd.so sees one definition of each."""
    import tonk_amd
    if not os.path.exists(tonk_amd.CBATCH_LIB_PATH):
        tonk_amd.build()
    out = subprocess.run(["nm", "-D", "--defined-only", tonk_amd.CBATCH_LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert names == set(N_ARGS) | {f"{PREFIX}_{n}" for n in COMMON}, sorted(names)[:20]


def test_bad_parameters_are_refused_before_any_device_call(lib):
    """Null, no streams, a maximum of 0 or above 24000, no side or an unknown one: "bad parameters"
    with or without a GPU (the check comes first); every call on a null handle is refused."""
    lib.tamd_cbatch_create.restype = ctypes.c_void_p
    lib.tamd_cbatch_create.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    for p in (None, Params(0, 0, 1300, 3), Params(0, 4, 0, 3), Params(0, 4, 24001, 3), Params(0, 4, 1300, 0), Params(0, 4, 1300, 4),
              Params(0, 4, 1300, 8 | 1), Params(0, 4, 1300, 3, 2)):
        err = ctypes.create_string_buffer(256)
        assert lib.tamd_cbatch_create(ctypes.byref(p) if p else None, err, len(err)) is None
        assert err.value == b"bad parameters", (p and (p.n_streams, p.max_message_bytes, p.sides), err.value)
    for f in (lib.tamd_cbatch_compress, lib.tamd_cbatch_decompress, lib.tamd_cbatch_reset):
        f.restype = ctypes.c_int
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.tamd_cbatch_compress.argtypes = [vp, u32, vp, vp, vp, vp, u64, vp]
    lib.tamd_cbatch_decompress.argtypes = [vp, u32, vp, vp, vp, vp, vp, u64, vp, vp]
    lib.tamd_cbatch_reset.argtypes = [vp, u32, vp, u32]
    assert lib.tamd_cbatch_compress(None, 0, None, None, None, None, 1300, None) == -1
    assert lib.tamd_cbatch_decompress(None, 0, None, None, None, None, None, 1300, None, None) == -1
    assert lib.tamd_cbatch_reset(None, 0, None, 3) == -1
    import tonk_amd
    for args in ((0, 1300), (4, 0), (4, 24001), (4, 1300, 0), (4, 1300, 4)):
        with pytest.raises(RuntimeError, match="bad parameters"):
            tonk_amd.BatchCompressor(*args)


def test_creation_needs_a_gfx950_device():
    """There is no CPU fallback: without an MI355X creation raises and names the reason."""
    import tonk_amd
    try:
        h = tonk_amd.BatchCompressor(2, 1300)
    except RuntimeError as e:
        assert re.search("no HIP device|gfx950", str(e)), e
    else:
        h.close()
