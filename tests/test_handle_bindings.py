"""CPU checks of what the Python classes over the batched device interfaces share
(tonk_amd/_handle.py): every function of include/tonk_batch.h, tonk_seal.h and tonk_datagram.h is
bound with as many argument types as its prototype has parameters, binding twice changes nothing,
and the three classes have one base.  No handle is created: no GPU is needed."""
from __future__ import annotations

import os
import re

import pytest

from conftest import ROOT
from test_dgram import N_ARGS as DGRAM_ARGS
from test_seal import N_ARGS as SEAL_ARGS

BATCH_ARGS = {"tamd_batch_encoder_add": 8, "tamd_batch_encoder_add_at": 9, "tamd_batch_encode": 7, "tamd_batch_encoder_ack": 5,
              "tamd_batch_decoder_add_original": 8, "tamd_batch_decoder_add_original_at": 9,
              "tamd_batch_decoder_add_recovery": 7, "tamd_batch_decode": 11, "tamd_batch_decoder_ack": 5}
COMMON = {"create": 3, "destroy": 1, "error": 1, "set_timing": 2, "kernel_ms": 3}
INTERFACES = [("BatchCodec", "tamd_batch", "tonk_batch.h", BATCH_ARGS), ("DatagramSealer", "tamd_seal", "tonk_seal.h", SEAL_ARGS),
              ("DatagramFramer", "tamd_dgram", "tonk_datagram.h", DGRAM_ARGS)]


def prototypes(header, prefix):
    """name -> parameter count of every function the header declares."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*|#define[^\n]*", "", text)
    return {name: params.count(",") + 1 for name, params in re.findall(r"\b(" + prefix + r"_\w+)\s*\(([^()]*)\)\s*;", text)}


@pytest.mark.parametrize("cls,prefix,header,n_args", INTERFACES)
def test_every_function_of_the_header_is_bound_with_its_parameter_count(cls, prefix, header, n_args):
    import tonk_amd
    if not os.path.exists(tonk_amd.LIB_PATH):
        tonk_amd.build()
    L = tonk_amd.lib()
    want = dict(n_args, **{f"{prefix}_{name}": k for name, k in COMMON.items()})
    assert prototypes(header, prefix) == want, "the header's prototypes and the tests' tables differ"
    klass = getattr(tonk_amd, cls)
    klass._bind()  # the class's binding step
    for name, k in want.items():
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == k, name
    # a second bind is a no-op: a prototype changed by hand in between stays as it is
    f = getattr(L, f"{prefix}_error")
    kept = f.argtypes
    f.argtypes = None
    try:
        klass._bind()
        assert f.argtypes is None
    finally:
        f.argtypes = kept


def test_the_three_classes_share_one_base():
    import tonk_amd
    from tonk_amd._handle import Handle
    for cls in (tonk_amd.BatchCodec, tonk_amd.DatagramSealer, tonk_amd.DatagramFramer):
        assert cls.__bases__ == (Handle,), cls
        for name in ("set_timing", "kernel_ms", "close", "__del__", "_check", "_create"):
            assert name not in vars(cls) and callable(getattr(cls, name)), (cls, name)
        assert len(cls.KERNEL_MS_FIELDS) >= 4 and cls._REFUSED.keys() == {-1, -2, -3, -4}
