#!/usr/bin/env python3
"""Time of receiving a tick's datagrams in device memory (include/tonk_receive.h).

Workload: DESIGN.md section 12's tick, 16,384 datagrams of 1,306 bytes at pitch 1,311 with three
nonce bytes (and three sequence bytes: 1,294 message bytes), every stream under its own key, in two
layouts -- wide (16,384 streams x 1 datagram) and deep (1,024 streams x 16, in arrival order: the
k-th datagrams of all streams lie together) -- each clean and with 1 % of the tags corrupted.  Every
call receives fresh datagrams (sealed on the device by DatagramSealer under the next nonces).  Per
configuration, `reps` timed calls after `warmup`, interleaved call by call with two yardsticks on
the same datagrams:

  (a) today's exact path: DatagramSealer.footers, nonce expansion and the anti-replay register in
      numpy on the host, DatagramSealer.open -- one round for wide, sixteen for deep (a round per
      depth, because the expansion of a datagram needs the verdicts of the one before);
  (b) a hipMemcpyAsync device-to-device copy of the same bytes.

Reported: the wall time of the receive call, the device time per kernel kind from HIP events
(tamd_recv_kernel_ms), the repaired tags per call, and the ratios to (a) and (b).  The bytes and
verdicts of the receive call and of (a) are compared after every call.

  python tools/recv_time.py [--reps 20] [--warmup 3] [--out profiles/recv_time.json]
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

N, BYTES, PITCH = 16384, 1306, 1311
NB, SB = 3, 3
MSG = BYTES - 6 - NB - SB
FLAGS = 0x80 | NB << 2 | SB
BITS = 4096


class HostRegisters:
    """StrikeRegister and CounterExpand for many streams at once in numpy: what a caller of
    tamd_seal_open keeps on the host today.  A nonce that slides a window is taken one by one."""

    def __init__(self, n):
        self.largest = np.zeros(n, dtype=np.uint64)
        self.base = np.zeros(n, dtype=np.uint64)
        self.rotation = np.zeros(n, dtype=np.int64)
        self.window = np.zeros((n, 64), dtype=np.uint64)

    def expand(self, s, partial, nb):
        bits = (8 * nb).astype(np.uint64)
        mask = (np.uint64(1) << bits) - np.uint64(1)
        gap = (partial.astype(np.uint64) - self.largest[s]) & mask
        signed = gap.astype(np.int64) - (((gap >> (bits - np.uint64(1))) & np.uint64(1)).astype(np.int64) << bits.astype(np.int64))
        out = (self.largest[s].view(np.int64) + signed).view(np.uint64)
        return np.where(nb == 0, self.largest[s] + np.uint64(1), out)

    def is_duplicate(self, s, nonce):
        dist = (nonce - self.base[s]).view(np.int64)
        bit = (np.clip(dist, 0, BITS - 1) + self.rotation[s]) % BITS
        struck = (self.window[s, bit // 64] >> (bit % 64).astype(np.uint64)) & np.uint64(1)
        return (dist < 0) | ((dist < BITS) & (struck != 0))

    def accept(self, s, nonce):
        """Streams are distinct within a call."""
        ahead = (nonce - self.largest[s]).view(np.int64) > 0
        self.largest[s[ahead]] = nonce[ahead]
        dist = (nonce - self.base[s]).view(np.int64)
        inside = (dist >= 0) & (dist < BITS)
        bit = (dist[inside] + self.rotation[s[inside]]) % BITS
        self.window[s[inside], bit // 64] |= np.uint64(1) << (bit % 64).astype(np.uint64)
        for k in np.flatnonzero(dist >= BITS):  # a slide or a reset
            st, d = int(s[k]), int(dist[k])
            slide = (d - BITS) // 64 + 1
            if slide >= 64:
                self.base[st], self.rotation[st] = nonce[k], 0
                self.window[st] = 0
                self.window[st, 0] = 1
                continue
            word = int(self.rotation[st]) // 64
            for _ in range(slide):
                self.window[st, word] = 0
                word = (word + 1) % 64
            self.base[st] += np.uint64(slide * 64)
            self.rotation[st] = (self.rotation[st] + slide * 64) % BITS
            b = (d - slide * 64 + int(self.rotation[st])) % BITS
            self.window[st, b // 64] |= np.uint64(1) << np.uint64(b % 64)


def todays_path(sealer, reg, stream, dev, n_rounds):
    """Yardstick (a) over the call's datagrams at `dev`: per round the footers come to the host, the
    nonces are expanded and checked there, open runs, and its verdicts go into the registers.
    Returns the result codes in tamd_recv_receive's numbering."""
    per = N // n_rounds
    rc_all = np.zeros(N, dtype=np.int32)
    nbytes = np.full(per, BYTES, dtype=np.uint32)
    for r in range(n_rounds):
        s = stream[r * per:(r + 1) * per].astype(np.int64)
        at = dev + r * per * PITCH
        foot = sealer.footers(nbytes, at, PITCH)
        flags = foot[:, 21].astype(np.int64)
        hs, nb, sb = np.where(flags & 0x40, 12, 0), (flags >> 2) & 3, flags & 3
        partial = np.zeros(per, dtype=np.uint64)
        rows = np.arange(per)
        for k in range(3):
            col = np.clip(18 - hs - nb + k, 0, 23)
            partial |= np.where(k < nb, foot[rows, col].astype(np.uint64) << np.uint64(8 * k), np.uint64(0))
        nonce = reg.expand(s, partial, nb)
        dup = reg.is_duplicate(s, nonce)
        msg = (BYTES - 6 - hs - nb - sb).astype(np.uint32)
        rc = sealer.open(s, nonce, np.where(dup, 0, nbytes), msg, at, PITCH)  # (0 bytes: refused, untouched)
        ok = (rc == 0) & ~dup
        reg.accept(s[ok], nonce[ok])
        rc_all[r * per:(r + 1) * per] = np.where(dup, 3, rc)
    return rc_all


def run(torch, hip, tonk_amd, layout, corrupt_share, reps, warmup, rng):
    streams, depth = (N, 1) if layout == "wide" else (N // 16, 16)
    stream = np.tile(np.arange(streams, dtype=np.uint32), depth)  # arrival order: round k of all streams together
    depth_of = np.repeat(np.arange(depth, dtype=np.uint64), streams)
    nbytes = np.full(N, BYTES, dtype=np.uint32)
    msg = np.full(N, MSG, dtype=np.uint32)
    template = np.full((N, PITCH), 0xA5, dtype=np.uint8)
    template[:, :BYTES] = rng.integers(0, 256, (N, BYTES), dtype=np.uint8)
    template[:, BYTES - 3] = FLAGS
    d_template = torch.from_numpy(template).cuda()
    d_flat = torch.zeros(N * BYTES, dtype=torch.uint8, device="cuda")
    d_copy = torch.zeros(N * BYTES, dtype=torch.uint8, device="cuda")
    sealer = tonk_amd.DatagramSealer(streams, 1500)
    rx = tonk_amd.DatagramReceiver(streams, 1500)
    for k in range(streams):
        key = int(rng.integers(1, 2**63))
        sealer.set_key(k, key)
        rx.set_key(k, key)
    rx.set_timing(True)
    reg = HostRegisters(streams)
    wall, wall_a, c_ms, kinds, repaired, bad = [], [], [], {k: [] for k in ("predict", "tag", "resolve", "decipher")}, [], []
    for rep in range(warmup + reps):
        nonce = np.uint64(rep * depth + 1) + depth_of
        d_buf = d_template.clone()
        d_buf[:, MSG + SB:MSG + SB + NB] = torch.from_numpy(np.stack([(nonce >> np.uint64(8 * k)).astype(np.uint8) for k in range(NB)], axis=1)).cuda()
        rc = sealer.seal(stream, nonce, nbytes, msg, d_buf.data_ptr(), PITCH)
        assert (rc == 0).all()
        hit = rng.choice(N, int(N * corrupt_share), replace=False) if corrupt_share else np.zeros(0, dtype=np.int64)
        if hit.size:
            d_buf[torch.from_numpy(hit).cuda(), BYTES - 2] ^= 1
        d_a = d_buf.clone()
        torch.cuda.synchronize()
        rx.kernel_ms()
        t0 = time.perf_counter()
        rc, result = rx.receive(stream, nbytes, d_buf.data_ptr(), PITCH)
        t1 = time.perf_counter()
        km = rx.kernel_ms()
        t2 = time.perf_counter()
        rc_a = todays_path(sealer, reg, stream, d_a.data_ptr(), depth)
        t3 = time.perf_counter()
        cm = copy_ms(torch, hip, d_copy, d_flat, N * BYTES)
        assert (rc == rc_a).all(), "receive and today's path disagree on a verdict"
        assert torch.equal(d_buf, d_a), "receive and today's path disagree on a byte"
        assert int((rc == 2).sum()) == hit.size and int((rc == 0).sum()) == N - hit.size
        assert km["predict_launches"] == 2 and km["tag_launches"] == km["resolve_launches"] == km["decipher_launches"] == 1
        if rep >= warmup:
            wall.append((t1 - t0) * 1e3)
            wall_a.append((t3 - t2) * 1e3)
            c_ms.append(cm)
            for k in kinds:
                kinds[k].append(km[k + "_ms"])
            repaired.append(km["repaired_tags"])
            bad.append(int(hit.size))
    for s in range(0, streams, max(1, streams // 64)):  # the registers ended equal
        st = rx.state(s)
        assert int(st[0]) == int(reg.largest[s]) and int(st[1]) == int(reg.base[s]) and (st[3:] == reg.window[s]).all()
    rx.close()
    sealer.close()
    med = statistics.median
    kernel = {k: round(med(v), 5) for k, v in kinds.items()}
    total = round(sum(med(v) for v in kinds.values()), 5)
    return {"layout": layout, "streams": streams, "depth": depth, "corrupted_share": corrupt_share, "corrupted_per_call": round(med(bad), 1),
            "receive_wall_ms_median": round(med(wall), 4), "receive_wall_ms_range": [round(min(wall), 4), round(max(wall), 4)],
            "kernel_ms_median": kernel, "kernel_ms_sum": total, "repaired_tags_per_call_median": med(repaired),
            "todays_path_rounds": depth, "todays_path_wall_ms_median": round(med(wall_a), 4),
            "copy_ms_median": round(med(c_ms), 5),
            "wall_over_todays_path": round(med(wall) / med(wall_a), 4), "kernel_sum_over_copy": round(total / med(c_ms), 3),
            "wall_over_copy": round(med(wall) / med(c_ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("recv_time: no GPU (there is no CPU path to time)")
    import tonk_amd
    hip = hip_runtime()
    rng = np.random.default_rng(2026)
    runs = [run(torch, hip, tonk_amd, layout, share, a.reps, a.warmup, rng) for layout in ("wide", "deep") for share in (0.0, 0.01)]
    result = {"datagrams": N, "bytes": BYTES, "pitch": PITCH, "nonce_bytes": NB, "seq_bytes": SB, "message_bytes": MSG,
              "total_bytes": N * BYTES, "reps": a.reps, "warmup": a.warmup, "runs": runs}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
