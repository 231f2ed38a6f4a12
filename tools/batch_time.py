#!/usr/bin/env python3
"""Rate of the batched codecs over the caller's device packets (include/tonk_batch.h).

Workload: 64 streams, 1300-byte packets, ticks of 256 originals and 5 recovery packets per stream
from a sender handle to the decoder side of a second handle, 1 % seeded loss on originals and
recovery packets alike, acknowledgements carried back every tick.  Every packet starts and ends in
device memory; the recovery packets' buffer goes from tamd_batch_encode straight into
tamd_batch_decoder_add_recovery.  Reported:

* payload GiB/s end to end (original payload bytes over the wall time of the timed ticks), the
  host time per call, and the kernels' own times from HIP events (tamd_batch_kernel_ms);
* (a) the reference codec (oracle/_ref/golden_gen, which links libsiamese_ref.so) on 16 host
  threads over the same shape: 64 streams x the same originals x 1300 B, 1 % loss, 5 recovery
  packets per 256 originals, an acknowledgement every 256 originals;
* (b) for tamd_frame_rows and tamd_unframe_rows, a hipMemcpyAsync device-to-device copy of the same
  bytes: the median of `reps` launches after `warmup` warm-up launches, kernel and copy interleaved.

  python tools/batch_time.py [--ticks 12] [--reps 20] [--warmup 3] [--threads 16] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, PAYLOAD, TICK, N_REC, LOSS = 64, 1300, 256, 5, 0.01
PITCH = PAYLOAD + 11  # odd: slots at every alignment


def hip_runtime():
    """The HIP runtime mapped into this process (the one the library and torch use)."""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln}, key=lambda p: "/torch/" not in p)
    L = ctypes.CDLL(paths[0])
    L.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return L


def copy_ms(torch, hip, dst, src, nbytes):
    """One hipMemcpyAsync device-to-device copy of nbytes, timed with events on torch's stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = torch.cuda.current_stream()
    a.record(st)
    assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, st.cuda_stream) == 0  # hipMemcpyDeviceToDevice
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def reference_rate(threads, n_orig):
    import tonk_amd
    exe = os.path.join(ROOT, "oracle", "_ref", "golden_gen")
    if not os.path.exists(exe):
        return None
    wp = tonk_amd.WorkloadParams(n=n_orig, payload=PAYLOAD, loss=LOSS, fec=N_REC / TICK, ack=TICK)
    r = subprocess.run([exe, "time", f"threads={threads}", f"streams={STREAMS}", "reps=1", "runs=5"] + wp.args(),
                       capture_output=True, text=True, timeout=900)
    passes = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    if r.returncode != 0 or not passes:
        return None
    vals = sorted(j["gib_per_s"] for j in passes)
    return {"gib_per_s": round(vals[len(vals) // 2], 4), "spread": [round(vals[0], 4), round(vals[-1], 4)],
            "threads": threads, "passes": len(passes),
            "sample": f"oracle/_ref/golden_gen time: {STREAMS} streams x {n_orig} originals x {PAYLOAD} B, {LOSS:.0%} loss "
                      f"(the workload's own draws), {N_REC} recovery packets per {TICK} originals spread over them, an "
                      f"acknowledgement every {TICK} originals, fresh codecs per pass"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_time: no GPU (there is no CPU path to time)")
    import tonk_amd
    hip = hip_runtime()
    rng = np.random.default_rng(2024)
    n = STREAMS * TICK
    # one tick's packets, stream by stream (reused every tick: the codecs' work does not depend on the bytes)
    pay = rng.integers(0, 256, (n, PAYLOAD), dtype=np.uint8)
    buf = np.full((n, PITCH), 0xA5, dtype=np.uint8)
    buf[:, :PAYLOAD] = pay
    d_src = torch.from_numpy(buf.reshape(-1)).cuda()
    d_rec = torch.zeros(STREAMS * N_REC * PITCH, dtype=torch.uint8, device="cuda")
    cap = 64 * STREAMS
    d_out = torch.zeros(cap * PITCH, dtype=torch.uint8, device="cuda")
    stream = np.repeat(np.arange(STREAMS, dtype=np.uint32), TICK)
    lens = np.full(n, PAYLOAD, dtype=np.uint32)
    elist = np.repeat(np.arange(STREAMS, dtype=np.uint32), N_REC)
    all_streams = np.arange(STREAMS, dtype=np.uint32)

    tx = tonk_amd.BatchCodec(STREAMS, PAYLOAD, 1 << 30)
    rx = tonk_amd.BatchCodec(STREAMS, PAYLOAD, 1 << 30)
    calls = ("encoder_add", "encode", "decoder_add_original", "decoder_add_recovery", "decode", "acks")
    host = dict.fromkeys(calls, 0.0)
    lost = recovered = 0

    def tick(t, timed, verify=False):
        nonlocal lost, recovered
        nums = (np.tile(np.arange(TICK, dtype=np.uint32), STREAMS) + t * TICK).astype(np.uint32)
        drop_o, drop_r = rng.random(n) < LOSS, rng.random(STREAMS * N_REC) < LOSS
        t0 = time.perf_counter()
        pn, rc = tx.encoder_add(stream, lens, d_src.data_ptr(), PITCH)
        t1 = time.perf_counter()
        nb, erc = tx.encode(elist, d_rec.data_ptr(), PITCH)
        t2 = time.perf_counter()
        orc = rx.decoder_add_original(stream, nums, np.where(drop_o, 0, lens).astype(np.uint32), d_src.data_ptr(), PITCH)
        t3 = time.perf_counter()
        rrc = rx.decoder_add_recovery(elist, np.where(drop_r, 0, nb).astype(np.uint32), d_rec.data_ptr(), PITCH)
        t4 = time.perf_counter()
        drc, o_s, o_n, o_b = rx.decode(all_streams, d_out.data_ptr(), PITCH, cap)
        t5 = time.perf_counter()
        for s in range(STREAMS):
            arc, ack = rx.decoder_ack(s)
            assert arc == 0 and tx.encoder_ack(s, ack)[0] == 0
        t6 = time.perf_counter()
        assert (rc == 0).all() and (pn == nums).all() and (erc == 0).all(), "the sender refused a packet"
        assert (orc[~drop_o] == 0).all() and (rrc[~drop_r] == 0).all(), "the receiver refused a packet"
        if timed:
            for k, v in zip(calls, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5)):
                host[k] += v
            lost += int(drop_o.sum())
            recovered += len(o_s)
        if verify and len(o_s):
            got = d_out[:len(o_s) * PITCH].cpu().numpy().reshape(-1, PITCH)
            for j in range(len(o_s)):
                assert o_b[j] == PAYLOAD and (got[j, :PAYLOAD] == pay[int(o_s[j]) * TICK + int(o_n[j]) % TICK]).all(), j
        return t6 - t0

    for t in range(2):  # warm-up ticks (first launches, staging growth)
        tick(t, False)
    tx.set_timing(True)
    rx.set_timing(True)
    tx.kernel_ms()
    rx.kernel_ms()
    wall = sum(tick(2 + t, True) for t in range(a.ticks))
    ktx, krx = tx.kernel_ms(), rx.kernel_ms()
    tick(2 + a.ticks, False, verify=True)
    payload_bytes = float(a.ticks) * n * PAYLOAD
    e2e = payload_bytes / wall / 2**30
    kernels = {k: round(ktx[k] + krx[k], 4) for k in ktx}
    result = {"streams": STREAMS, "payload_bytes": PAYLOAD, "originals_per_tick": TICK, "recovery_per_tick": N_REC,
              "loss": LOSS, "pitch": PITCH, "ticks": a.ticks, "lost_originals": lost, "recovered_originals": recovered,
              "end_to_end": {"gib_per_s": round(e2e, 4), "wall_ms_per_tick": round(wall / a.ticks * 1e3, 3),
                             "host_ms_per_tick": {k: round(v / a.ticks * 1e3, 3) for k, v in host.items()}},
              "kernel_ms_per_tick": {k: round(v / a.ticks, 4) for k, v in kernels.items() if k.endswith("_ms")},
              "kernel_totals": kernels}
    tx.close()
    rx.close()

    # (b) tamd_frame_rows beside a device-to-device copy of the same bytes, interleaved: a tick's
    # originals into a fresh handle per launch series (no acknowledgements: 23 x 256 packets fit a window)
    fr = tonk_amd.BatchCodec(STREAMS, PAYLOAD, 2 << 30)
    fr.set_timing(True)
    d_copy = torch.zeros(n * PAYLOAD, dtype=torch.uint8, device="cuda")
    d_flat = torch.from_numpy(pay.reshape(-1)).cuda()
    k_ms, c_ms = [], []
    for rep in range(a.warmup + a.reps):
        pn, rc = fr.encoder_add(stream, lens, d_src.data_ptr(), PITCH)
        assert (rc == 0).all()
        km = fr.kernel_ms()
        cm = copy_ms(torch, hip, d_copy, d_flat, n * PAYLOAD)
        if rep >= a.warmup:
            assert km["frame_launches"] == 1 and km["frame_bytes"] == n * PAYLOAD
            k_ms.append(km["frame_ms"])
            c_ms.append(cm)
    # tamd_unframe_rows: the recovery packets of those windows out (raw rows), the launch as the
    # workload has it (64 x 5 packets), beside a copy of the same bytes
    u_ms, uc_ms, u_bytes = [], [], 0
    for rep in range(a.warmup + a.reps):
        nb, rc = fr.encode(elist, d_rec.data_ptr(), PITCH)
        assert (rc == 0).all()
        km = fr.kernel_ms()
        u_bytes = int(nb.sum())
        cm = copy_ms(torch, hip, d_copy, d_flat, u_bytes)
        if rep >= a.warmup:
            assert km["unframe_launches"] == 1 and km["unframe_bytes"] == u_bytes
            u_ms.append(km["unframe_ms"])
            uc_ms.append(cm)
    fr.close()

    def rate(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / 1e12, 4)

    fm, cm, um, ucm = (statistics.median(v) for v in (k_ms, c_ms, u_ms, uc_ms))
    result["frame_vs_copy"] = {
        "reps": a.reps, "warmup": a.warmup,
        "frame": {"packets": n, "payload_bytes": n * PAYLOAD, "kernel_ms_median": round(fm, 5), "kernel_ms_range": [round(min(k_ms), 5), round(max(k_ms), 5)],
                  "payload_tb_per_s": rate(n * PAYLOAD, fm), "copy_ms_median": round(cm, 5), "copy_tb_per_s": rate(n * PAYLOAD, cm),
                  "kernel_over_copy": round(cm / fm, 3)},
        "unframe": {"packets": int(elist.size), "bytes": u_bytes, "kernel_ms_median": round(um, 5), "kernel_ms_range": [round(min(u_ms), 5), round(max(u_ms), 5)],
                    "tb_per_s": rate(u_bytes, um), "copy_ms_median": round(ucm, 5), "copy_tb_per_s": rate(u_bytes, ucm),
                    "kernel_over_copy": round(ucm / um, 3)}}
    ref = reference_rate(a.threads, (2 + a.ticks) * TICK)
    result["reference_cpu"] = ref
    if ref:
        result["end_to_end"]["over_reference"] = round(e2e / ref["gib_per_s"], 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
