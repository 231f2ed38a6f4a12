#!/usr/bin/env python3
"""Time of building and parsing a tick's datagrams in device memory (include/tonk_datagram.h).

Workload: 16,384 datagrams of 1,306 bytes at pitch 1,311 (tools/batch_time.py's tick of 64 streams
x 256 packets, tools/seal_time.py's datagrams), in two shapes:

  single  one Unreliable message of 1,286 bytes and the handshake footer (2 + 1,286 + 12 + 6)
  mix     four messages -- an AckAck of 3 bytes, an Unreliable message of 17, reliable ones of 300
          and 966 -- with three sequence and three nonce bytes (8 + 1,286 + 6 + 6)

The bodies lie back to back in one source buffer (1,286 bytes per datagram: every body at another
alignment).  `reps` timed tamd_dgram_build launches and as many tamd_dgram_parse launches over
what was built after `warmup` warm-up launches, each interleaved with a hipMemcpyAsync
device-to-device copy of the same number of bytes; kernel times from HIP events
(tamd_dgram_kernel_ms), the host time per call from the wall clock.  The built bytes and the parsed
tables are compared with tests/dgram_ref.py's for the first and the last datagram.

  python tools/dgram_time.py [--reps 20] [--warmup 3] [--out profiles/dgram_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from batch_time import copy_ms, hip_runtime  # noqa: E402

STREAMS, TICK, BYTES, PITCH, BODY = 64, 256, 1306, 1311, 1286
SHAPES = {"single": dict(msgs=[(3, 1286)], seq_bytes=0, nonce_bytes=0, handshake=True),
          "mix": dict(msgs=[(2, 3), (3, 17), (6, 300), (7, 966)], seq_bytes=3, nonce_bytes=3, handshake=False)}


def run(torch, hip, tonk_amd, name, shape, reps, warmup):
    import dgram_ref as R
    rng = np.random.default_rng(2026)
    n = STREAMS * TICK
    msgs = shape["msgs"]
    assert sum(b for _, b in msgs) == BODY
    bodies = rng.integers(0, 256, n * BODY, dtype=np.uint8)
    d_src = torch.from_numpy(bodies).cuda()
    d_out = torch.full((n * PITCH,), 0xA5, dtype=torch.uint8, device="cuda")
    d_flat = torch.zeros(n * BYTES, dtype=torch.uint8, device="cuda")
    d_copy = torch.zeros(n * BYTES, dtype=torch.uint8, device="cuda")
    k = len(msgs)
    dgram = np.repeat(np.arange(n, dtype=np.uint32), k)
    mtype = np.tile(np.array([t for t, _ in msgs], dtype=np.uint32), n)
    mbytes = np.tile(np.array([b for _, b in msgs], dtype=np.uint32), n)
    starts = np.concatenate([[0], np.cumsum([b for _, b in msgs])[:-1]]).astype(np.uint64)
    src = (np.uint64(d_src.data_ptr()) + (np.arange(n, dtype=np.uint64) * np.uint64(BODY))[:, None] + starts[None, :]).reshape(-1)
    seq = np.arange(n, dtype=np.uint32) % TICK
    nonce = np.arange(n, dtype=np.uint32) + 77
    ts24 = (np.arange(n, dtype=np.uint32) * 2654435761 >> 8).astype(np.uint32) & 0xFFFFFF
    hs = rng.integers(0, 256, (n, 12), dtype=np.uint8) if shape["handshake"] else None
    has = np.ones(n, dtype=np.uint8) if shape["handshake"] else None
    sb, nb, fb = np.full(n, shape["seq_bytes"], np.uint32), np.full(n, shape["nonce_bytes"], np.uint32), np.full(n, R.SEQCOMP, np.uint32)

    f = tonk_amd.DatagramFramer(1500)
    f.set_timing(True)
    build_ms, parse_ms, c_ms, host_build, host_parse = [], [], [], [], []
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        ob, mb, ro, rb, rc = f.build(dgram, mtype, mbytes, src, seq, sb, nonce, nb, ts24, fb, d_out.data_ptr(), PITCH, handshake=hs,
                                     has_handshake=has)
        t1 = time.perf_counter()
        kb = f.kernel_ms()
        cb = copy_ms(torch, hip, d_copy, d_flat, n * BYTES)
        assert (rc == 0).all() and (ob == BYTES).all() and kb["build_launches"] == 1
        t2 = time.perf_counter()
        status, count, lo, nrel, table = f.parse(mb, d_out.data_ptr(), PITCH, mode=0, cap=k)
        t3 = time.perf_counter()
        kp = f.kernel_ms()
        cp = copy_ms(torch, hip, d_copy, d_flat, n * BYTES)
        assert (status == 0).all() and (count == k).all() and kp["parse_launches"] == 1
        if rep >= warmup:
            build_ms.append(kb["build_ms"])
            parse_ms.append(kp["parse_ms"])
            c_ms += [cb, cp]
            host_build.append((t1 - t0) * 1e3)
            host_parse.append((t3 - t2) * 1e3)
    f.close()
    built = d_out.cpu().numpy().reshape(n, PITCH)
    assert (built[:, BYTES:] == 0xA5).all(), "build wrote past a datagram"
    for i in (0, n - 1):
        body = bodies[i * BODY:(i + 1) * BODY]
        parts, at = [], 0
        for t, b in msgs:
            parts.append((t, body[at:at + b].tobytes()))
            at += b
        want = R.build(parts, int(seq[i]), shape["seq_bytes"], int(nonce[i]), shape["nonce_bytes"], hs[i].tobytes() if hs is not None else None,
                       int(ts24[i]), R.SEQCOMP)
        assert want[0] == 0 and built[i, :BYTES].tobytes() == want[1], f"datagram {i} differs from the restatement"
        assert list(table[i]) == R.parse(want[1][:want[2]])[1] and (int(lo[i]), int(nrel[i])) == want[3:5]

    def side(ms, host, copy):
        m = statistics.median(ms)
        return {"kernel_ms_median": round(m, 5), "kernel_ms_range": [round(min(ms), 5), round(max(ms), 5)],
                "tb_per_s": round(n * BYTES / (m * 1e-3) / 1e12, 4), "kernel_over_copy": round(copy / m, 3),
                "host_ms_per_call_median": round(statistics.median(host), 4)}

    cm = statistics.median(c_ms)
    return {"messages_per_datagram": k, "message_bytes": int(mb[0]),
            "copy": {"ms_median": round(cm, 5), "ms_range": [round(min(c_ms), 5), round(max(c_ms), 5)],
                     "tb_per_s": round(n * BYTES / (cm * 1e-3) / 1e12, 4)},
            "build": side(build_ms, host_build, cm), "parse": side(parse_ms, host_parse, cm)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dgram_time: no GPU (there is no CPU path to time)")
    import tonk_amd
    hip = hip_runtime()
    result = {"datagrams": STREAMS * TICK, "streams": STREAMS, "bytes": BYTES, "pitch": PITCH, "total_bytes": STREAMS * TICK * BYTES,
              "reps": a.reps, "warmup": a.warmup}
    for name, shape in SHAPES.items():
        result[name] = run(torch, hip, tonk_amd, name, shape, a.reps, a.warmup)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
