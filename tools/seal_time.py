#!/usr/bin/env python3
"""Time of sealing and opening a tick's datagrams in device memory (include/tonk_seal.h).

Workload: 16,384 datagrams of 1,306 bytes (tools/batch_time.py's tick of 64 streams x 256 packets
of 1,300 bytes, with the six untagged footer bytes) at pitch 1,311, every stream under its own
key, all but the last 12 tagged bytes ciphered.  `reps` timed tamd_seal_seal launches and as many
tamd_seal_open launches after `warmup` warm-up launches, each interleaved with a hipMemcpyAsync
device-to-device copy of the same bytes; kernel times from HIP events (tamd_seal_kernel_ms), the
host time per call from the wall clock.  The opened datagrams are compared with the originals.
The two primitives are timed alone over the same bytes (tamd_seal_cipher over the message bytes,
tamd_seal_tag over the tagged bytes): they are the two phases of a seal.

  python tools/seal_time.py [--reps 20] [--warmup 3] [--out profiles/seal_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from batch_time import copy_ms, hip_runtime  # noqa: E402

STREAMS, TICK, BYTES, PITCH = 64, 256, 1306, 1311
FOOTERS = 12  # nonce and sequence footers: tagged, not ciphered


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("seal_time: no GPU (there is no CPU path to time)")
    import tonk_amd
    hip = hip_runtime()
    rng = np.random.default_rng(2025)
    n = STREAMS * TICK
    plain = np.full((n, PITCH), 0xA5, dtype=np.uint8)
    plain[:, :BYTES] = rng.integers(0, 256, (n, BYTES), dtype=np.uint8)
    d_buf = torch.from_numpy(plain.reshape(-1)).cuda()
    d_flat = torch.zeros(n * BYTES, dtype=torch.uint8, device="cuda")
    d_copy = torch.zeros(n * BYTES, dtype=torch.uint8, device="cuda")
    stream = np.repeat(np.arange(STREAMS, dtype=np.uint32), TICK)
    nbytes = np.full(n, BYTES, dtype=np.uint32)
    msg = np.full(n, BYTES - 6 - FOOTERS, dtype=np.uint32)

    s = tonk_amd.DatagramSealer(STREAMS, 1500)
    for k in range(STREAMS):
        s.set_key(k, int(rng.integers(1, 2**63)))
    s.set_timing(True)
    seal_ms, open_ms, c_ms, host_seal, host_open = [], [], [], [], []
    for rep in range(a.warmup + a.reps):
        nonce = (np.arange(n, dtype=np.uint64) % TICK) + np.uint64(rep * TICK)
        t0 = time.perf_counter()
        rc = s.seal(stream, nonce, nbytes, msg, d_buf.data_ptr(), PITCH)
        t1 = time.perf_counter()
        ks = s.kernel_ms()
        cs = copy_ms(torch, hip, d_copy, d_flat, n * BYTES)
        assert (rc == 0).all() and ks["packets_launches"] == 1
        t2 = time.perf_counter()
        rc = s.open(stream, nonce, nbytes, msg, d_buf.data_ptr(), PITCH)
        t3 = time.perf_counter()
        ko = s.kernel_ms()
        co = copy_ms(torch, hip, d_copy, d_flat, n * BYTES)
        assert (rc == 0).all() and ko["packets_launches"] == 1, "a sealed datagram did not open"
        if rep >= a.warmup:
            seal_ms.append(ks["packets_ms"])
            open_ms.append(ko["packets_ms"])
            c_ms += [cs, co]
            host_seal.append((t1 - t0) * 1e3)
            host_open.append((t3 - t2) * 1e3)
    cipher_ms, tag_ms = [], []
    nonce = np.arange(n, dtype=np.uint64)
    for rep in range(a.warmup + a.reps):  # (an even number of cipher calls: the bytes end as they were)
        s.cipher(stream, nonce, msg, d_buf.data_ptr(), PITCH)
        kc = s.kernel_ms()
        s.tag(stream, nonce, nbytes - 6, d_buf.data_ptr(), PITCH)
        kt = s.kernel_ms()
        if rep >= a.warmup:
            cipher_ms.append(kc["packets_ms"])
            tag_ms.append(kt["packets_ms"])
    if (a.warmup + a.reps) % 2:
        s.cipher(stream, nonce, msg, d_buf.data_ptr(), PITCH)
    back = d_buf.cpu().numpy().reshape(n, PITCH)
    assert (back[:, :BYTES - 2] == plain[:, :BYTES - 2]).all() and (back[:, BYTES:] == 0xA5).all(), "open did not restore the datagrams"
    s.close()

    def side(ms, host, copy):
        m = statistics.median(ms)
        return {"kernel_ms_median": round(m, 5), "kernel_ms_range": [round(min(ms), 5), round(max(ms), 5)],
                "tb_per_s": round(n * BYTES / (m * 1e-3) / 1e12, 4), "kernel_over_copy": round(copy / m, 3),
                "host_ms_per_call_median": round(statistics.median(host), 4)}

    cm = statistics.median(c_ms)
    result = {"datagrams": n, "streams": STREAMS, "bytes": BYTES, "pitch": PITCH, "message_bytes": int(msg[0]),
              "total_bytes": n * BYTES, "reps": a.reps, "warmup": a.warmup,
              "copy": {"ms_median": round(cm, 5), "ms_range": [round(min(c_ms), 5), round(max(c_ms), 5)],
                       "tb_per_s": round(n * BYTES / (cm * 1e-3) / 1e12, 4)},
              "seal": side(seal_ms, host_seal, cm), "open": side(open_ms, host_open, cm),
              "cipher_alone_kernel_ms_median": round(statistics.median(cipher_ms), 5),
              "tag_alone_kernel_ms_median": round(statistics.median(tag_ms), 5)}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
