#!/usr/bin/env python3
"""Rate of the decompression kernel (tamd_decompress_batch's kernel_ms) beside the reference
decompressor on host threads.

Input: bench.py's compress_messages shape, wide (one stream is one wave): 4,096 streams x 64
messages by default.  Decoded twice: the GPU compressor's blocks (tamd_compress_batch, chained on
the device) and the reference compressor's blocks (zstd level 1: Huffman literals).  Baseline: the
reference decompressor over the same blocks on 16 host threads (tests/native/_build/unlz_check
bench, which links oracle/_ref/libmsgcodec_ref.so; decoding alone is timed, the median of 9
repetitions).  Rates are GiB/s of restored bytes; kernel
time is the median of the timed launches after warm-up.

  python tools/decompress_time.py [--streams 4096] [--msgs 64] [--reps 20] [--threads 16] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import msgcodec_py  # noqa: E402
from msgcodec_py import MAX  # noqa: E402


def ref_compress_all(data, lens, n_streams, n_msgs):
    L = msgcodec_py.load()
    slots = np.zeros((n_streams * n_msgs, MAX), dtype=np.uint8)
    written = np.zeros(n_streams * n_msgs, dtype=np.uint32)
    w = ctypes.c_uint(0)
    for s in range(n_streams):
        c = L.ref_comp_new(MAX)
        row = np.ascontiguousarray(data[s])
        pos = 0
        for k in range(n_msgs):
            i = s * n_msgs + k
            n = int(lens[i])
            L.ref_comp(c, row.ctypes.data + pos, n, slots[i].ctypes.data, ctypes.byref(w))
            written[i] = w.value
            pos += n
        L.ref_comp_free(c)
    return slots, written


def fill_uncompressed(slots, written, data, lens, n_streams, n_msgs):
    """The caller's part of the chain: messages sent as is are copied into their slots."""
    for s in range(n_streams):
        pos = 0
        for k in range(n_msgs):
            i = s * n_msgs + k
            n = int(lens[i])
            if written[i] == 0:
                slots[i, :n] = data[s, pos:pos + n]
            pos += n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--msgs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("decompress_time: no GPU (there is no CPU path to time)")
    import bench
    from tonk_amd.compress import compress_batch, decompress_batch
    n_streams, n_msgs, total = a.streams, a.msgs, a.streams * a.msgs
    data, lens, stride = bench.compress_messages(n_streams, n_msgs)
    lens = np.asarray(lens, dtype=np.uint32).reshape(-1)
    restored_bytes = float(lens.sum())
    exe = os.path.join(ROOT, "tests", "native", "_build", "unlz_check")
    result = {"streams": n_streams, "messages_per_stream": n_msgs, "max_bytes": MAX, "restored_bytes": int(restored_bytes),
              "reps": a.reps, "warmup": a.warmup, "cases": {}}

    d_data = torch.from_numpy(data).cuda()
    d_blocks = torch.zeros(total * MAX + 32, dtype=torch.uint8, device="cuda")
    written, _ = compress_batch(d_data.data_ptr(), stride, n_streams, n_msgs, lens, MAX, d_blocks.data_ptr())
    gpu_slots = d_blocks[:total * MAX].cpu().numpy().reshape(total, MAX).copy()
    ref_slots, ref_written = ref_compress_all(data, lens, n_streams, n_msgs)
    d_out = torch.zeros(total * MAX, dtype=torch.uint8, device="cuda")
    # Two more cases split the kernel's time: every message sent as is (the InsertUncompressed
    # path: copies only), and every message as a block of raw literals with no sequences (adds
    # what a block costs before its first sequence: placing, staging, the headers).
    none = np.zeros(total, dtype=np.uint32)
    raw_slots = np.zeros((total, MAX), dtype=np.uint8)
    raw_bytes = np.zeros(total, dtype=np.uint32)
    fill_uncompressed(raw_slots, none, data, lens, n_streams, n_msgs)
    for i in range(total):
        n = int(lens[i])
        if n + 4 > MAX:
            continue  # (stays an uncompressed message: the block would not fit its slot)
        h = 0x04 | ((n & 15) << 4) | ((n >> 4) << 8)  # Raw_Literals_Block, 12-bit size
        raw_slots[i, 2:2 + n] = raw_slots[i, :n].copy()
        raw_slots[i, 0], raw_slots[i, 1], raw_slots[i, 2 + n] = h & 255, h >> 8, 0
        raw_bytes[i] = n + 3
    for name, slots, wr in (("gpu_compressor_blocks", gpu_slots, written), ("reference_compressor_blocks", ref_slots, ref_written),
                            ("uncompressed_messages", np.zeros((total, MAX), dtype=np.uint8), none),
                            ("raw_literal_blocks", raw_slots, raw_bytes)):
        if name != "raw_literal_blocks":
            fill_uncompressed(slots, wr, data, lens, n_streams, n_msgs)
        in_bytes = np.where(wr > 0, wr, lens).astype(np.uint32)
        is_block = (wr > 0).astype(np.uint8)
        d_blocks[:total * MAX] = torch.from_numpy(slots.reshape(-1)).cuda()
        times = []
        for rep in range(a.warmup + a.reps):
            restored, status, ms = decompress_batch(d_blocks.data_ptr(), n_streams, n_msgs, in_bytes, is_block, MAX,
                                                    d_out.data_ptr())
            if rep >= a.warmup:
                times.append(ms)
        torch.cuda.synchronize()
        assert (status == 0).all() and (restored == lens).all(), "a message was not restored"
        got = d_out.cpu().numpy().reshape(total, MAX)
        for i in range(0, total, max(1, total // 512)):  # spot check against the input
            s, k = divmod(i, n_msgs)
            p = int(lens.reshape(n_streams, n_msgs)[s, :k].sum())
            assert (got[i, :lens[i]] == data[s, p:p + lens[i]]).all(), i
        med = statistics.median(times)
        gpu_rate = restored_bytes / (med * 1e-3) / 2**30
        if name in ("uncompressed_messages", "raw_literal_blocks"):
            result["cases"][name] = {"blocks": int(is_block.sum()), "kernel_ms_median": round(med, 4),
                                     "gpu_gib_per_s": round(gpu_rate, 3)}
            continue
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "blocks.bin")
            msgcodec_py.write_streams(path, [(MAX, [(is_block[i], slots[i, :in_bytes[i]].tobytes())
                                                    for i in range(s * n_msgs, (s + 1) * n_msgs)]) for s in range(n_streams)])
            r = subprocess.run([exe, "bench", path, str(a.threads), "9"], capture_output=True, text=True, check=True)
        cpu = json.loads(r.stdout.strip().splitlines()[-1])
        result["cases"][name] = {
            "blocks": int(is_block.sum()), "compressed_bytes": int(in_bytes.sum()),
            "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times), 4), "kernel_ms_max": round(max(times), 4),
            "gpu_gib_per_s": round(gpu_rate, 3), "cpu_threads": a.threads, "cpu_gib_per_s": cpu["gib_per_s"],
            "cpu_gib_per_s_range": [cpu["gib_per_s_slowest"], cpu["gib_per_s_fastest"]], "cpu_reps": cpu["reps"],
            "gpu_over_cpu": round(gpu_rate / cpu["gib_per_s"], 3)}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
