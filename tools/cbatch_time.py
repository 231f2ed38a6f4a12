#!/usr/bin/env python3
"""Time of compressing and restoring a tick's messages of many connections in device memory
(include/tonk_compress_batch.h), beside the two paths the library had before it.

Two ticks, over compressible messages of 64..1300 bytes (slices of a text of nine words, one in
four of them random bytes, as tests/lz_streams.py's mixed_messages):

  wide   16,384 streams x 1 message
  deep    1,024 streams x 16 messages

Every stream has its own history: the ticks before the timed ones are warm-up, enough of them that
every ring has restarted at least once (24,000 bytes per stream).  Per timed tick, in this order and
in one process:

  handle   BatchCompressor.compress, then .decompress of what it returned (blocks where there are
           blocks, the originals in place where not): wall time per call and device time per kernel
           kind (kernel_ms).  On the deep tick also a handle created with abut.
  dropin   (a) the same messages through the per-message drop-in (MessageCompressor /
           MessageDecompressor, host memory in and out) from 16 threads, a stream's messages in
           order on one thread: wall time
  fresh    (b) tamd_compress_batch / tamd_decompress_batch on fresh streams of the tick's messages,
           every message a job of its own: device time only, the kernel-only floor with no history

How many of the handle's `written` values differ from the drop-in's over all ticks is reported
(none should), and restored messages are compared with the originals.  `--seed-share` runs tamd_compress_batch with one message
per job over streams with history under TONK_AMD_LZ_PROF and reports the share of a job that is
the seeding of its window (the library's own phase stamps).

  python tools/cbatch_time.py [--reps 20] [--out profiles/cbatch_time.json] [--seed-share]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX, LO, HI, DICT, THREADS = 1300, 64, 1300, 24000, 16
TICKS = {"wide": (16384, 1), "deep": (1024, 16)}
WORDS = [b"siamese ", b"tonk ", b"packet ", b"recovery ", b"window ", b"lane ", b"sum ", b"ack ", b"0123 "]


def corpus(rng, nbytes):
    """Text of the nine words in random order, and as many random bytes behind it."""
    idx = rng.integers(0, len(WORDS), nbytes // 4)
    text = np.frombuffer(b"".join(WORDS[i] for i in idx)[:nbytes], dtype=np.uint8)
    return np.concatenate([text, rng.integers(0, 256, nbytes, dtype=np.uint8)]), text.size


def draw_tick(rng, corp, text_bytes, n_streams, per):
    """A tick's messages: lens (streams, per) and each stream's bytes end to end in its row."""
    lens = rng.integers(LO, HI + 1, (n_streams, per)).astype(np.uint32)
    random = rng.integers(0, 4, (n_streams, per)) == 0
    offs = rng.integers(0, text_bytes - HI, (n_streams, per)) + np.where(random, text_bytes, 0)
    stride = (per * HI + 64 + 15) // 16 * 16
    rows = np.zeros((n_streams, stride), dtype=np.uint8)
    starts = (np.cumsum(lens, axis=1) - lens).astype(np.int64)
    flat_len = lens.reshape(-1).astype(np.int64)
    total = int(flat_len.sum())
    first = np.cumsum(flat_len) - flat_len
    within = np.arange(total) - np.repeat(first, flat_len)
    src_idx = np.repeat(offs.reshape(-1), flat_len) + within
    row = np.repeat(np.repeat(np.arange(n_streams), per), flat_len)
    col = np.repeat(starts.reshape(-1), flat_len) + within
    rows[row, col] = corp[src_idx]
    return lens, starts.astype(np.uint64), rows, stride


def run_threads(n, work):
    err = []

    def go(t):
        try:
            work(t)
        except Exception as e:  # surfaced below
            err.append(repr(e))

    th = [threading.Thread(target=go, args=(t,)) for t in range(n)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not err, err[:3]
    return (time.perf_counter() - t0) * 1e3


def run_tick(torch, tonk_amd, name, n_streams, per, reps, log):
    from tonk_amd import cbatch
    from tonk_amd.compress import MessageCompressor, MessageDecompressor, compress_batch, decompress_batch
    rng = np.random.default_rng(2026)
    corp, text_bytes = corpus(rng, 1 << 20)
    n = n_streams * per
    warmup = DICT // (per * (LO + HI) // 2) + 2
    handles = {"exact": False} if per == 1 else {"exact": False, "abut": True}
    comp = {k: tonk_amd.BatchCompressor(n_streams, MAX, sides=cbatch.COMPRESS, abut=v) for k, v in handles.items()}
    deco = {k: tonk_amd.BatchCompressor(n_streams, MAX, sides=cbatch.DECOMPRESS) for k in handles}
    for h in list(comp.values()) + list(deco.values()):
        h.set_timing(True)
    d_comp = [MessageCompressor(MAX) for _ in range(n_streams)]
    d_deco = [MessageDecompressor(MAX) for _ in range(n_streams)]
    stream = np.repeat(np.arange(n_streams, dtype=np.uint32), per)
    d_out = torch.empty(n * MAX + 64, dtype=torch.uint8, device="cuda")
    d_res = torch.empty(n * MAX + 64, dtype=torch.uint8, device="cuda")
    d_slots = torch.zeros(n * MAX + 64, dtype=torch.uint8, device="cuda")
    rec = {k: {"compress_wall": [], "decompress_wall": [], "place_ms": [], "compress_ms": [], "decompress_ms": [], "launches": []}
           for k in handles}
    rec["dropin"] = {"compress_wall": [], "decompress_wall": []}
    rec["fresh"] = {"compress_ms": [], "decompress_ms": []}
    sent = blocks = differing = 0
    for tick in range(warmup + reps):
        lens, starts, rows, stride = draw_tick(rng, corp, text_bytes, n_streams, per)
        d_rows = torch.from_numpy(rows).cuda()
        flat = lens.reshape(-1)
        src = (np.uint64(d_rows.data_ptr()) + np.arange(n_streams, dtype=np.uint64)[:, None] * np.uint64(stride) + starts).reshape(-1)
        timed = tick >= warmup
        msgs = [rows[s, int(starts[s, k]):int(starts[s, k]) + int(lens[s, k])].tobytes() for s in range(n_streams) for k in range(per)]
        written = {}
        for k in handles:
            d_out.fill_(0xA5)
            t0 = time.perf_counter()
            w = comp[k].compress(stream, src, flat, d_out.data_ptr(), MAX)
            t1 = time.perf_counter()
            kc = comp[k].kernel_ms()
            isb = (w != 0).astype(np.uint8)
            ins = np.where(w != 0, np.uint64(d_out.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(MAX), src)
            t2 = time.perf_counter()
            restored, status = deco[k].decompress(stream, ins, np.where(w != 0, w, flat), isb, d_res.data_ptr(), MAX)
            t3 = time.perf_counter()
            kd = deco[k].kernel_ms()
            assert (status == 0).all() and (restored == flat).all(), (name, k, tick)
            written[k] = w
            if timed:
                r = rec[k]
                r["compress_wall"].append((t1 - t0) * 1e3)
                r["decompress_wall"].append((t3 - t2) * 1e3)
                r["place_ms"].append(kc["place_ms"])
                r["compress_ms"].append(kc["compress_ms"])
                r["decompress_ms"].append(kd["decompress_ms"])
                r["launches"].append(kc["compress_launches"])
            if tick == warmup + reps - 1:  # the restored blocks of the last tick, byte for byte
                got = d_res.cpu().numpy()[:n * MAX].reshape(n, MAX)
                for i in np.flatnonzero(isb)[:: max(1, n // 2048)]:
                    assert got[i, :flat[i]].tobytes() == msgs[i], (name, k, int(i))
        # (a) the drop-in from 16 threads: stream s on thread s % 16
        d_blocks = [None] * n

        def comp_work(t):
            for s in range(t, n_streams, THREADS):
                for k in range(per):
                    d_blocks[s * per + k] = d_comp[s].compress(msgs[s * per + k])

        def deco_work(t):
            for s in range(t, n_streams, THREADS):
                for k in range(per):
                    b = d_blocks[s * per + k]
                    if b:
                        assert d_deco[s].decompress(b) == msgs[s * per + k]
                    else:
                        d_deco[s].insert_uncompressed(msgs[s * per + k])

        ca = run_threads(THREADS, comp_work)
        da = run_threads(THREADS, deco_work)
        dw = np.array([len(b) for b in d_blocks], dtype=np.uint32)
        differ_now = int((written["exact"] != dw).sum())
        differing += differ_now
        # (b) fresh streams of the same messages, a message per job
        wf, cms = compress_batch(d_rows.data_ptr(), stride, n_streams, per, flat, MAX, d_out.data_ptr(), msgs_per_job=1)
        padded = np.zeros((n, MAX), dtype=np.uint8)
        for i in np.flatnonzero(wf == 0):
            padded[i, :flat[i]] = np.frombuffer(msgs[i], dtype=np.uint8)
        asis = torch.from_numpy(wf == 0).cuda()
        d_slots[:n * MAX].view(n, MAX)[asis] = torch.from_numpy(padded).cuda()[asis]
        d_slots[:n * MAX].view(n, MAX)[~asis] = d_out[:n * MAX].view(n, MAX)[~asis]
        torch.cuda.synchronize()
        rf, sf, dms = decompress_batch(d_slots.data_ptr(), n_streams, per, np.where(wf != 0, wf, flat), wf != 0, MAX, d_res.data_ptr())
        assert (sf == 0).all() and (rf == flat).all()
        if timed:
            rec["dropin"]["compress_wall"].append(ca)
            rec["dropin"]["decompress_wall"].append(da)
            rec["fresh"]["compress_ms"].append(cms)
            rec["fresh"]["decompress_ms"].append(dms)
            sent += int(flat.sum())
            blocks += int(np.where(written["exact"] != 0, written["exact"], flat).sum())
        print(f"{name}: tick {tick + 1}/{warmup + reps} handle {1e3 * (t1 - t0):.2f}+{1e3 * (t3 - t2):.2f} ms, drop-in {ca:.0f}+{da:.0f} ms, "
              f"{differ_now} written values differ from the drop-in's", file=log, flush=True)
    for h in list(comp.values()) + list(deco.values()) + d_comp + d_deco:
        h.close()

    def med(v):
        return {"median": round(statistics.median(v), 4), "range": [round(min(v), 4), round(max(v), 4)]}

    out = {"streams": n_streams, "messages_per_stream": per, "messages": n, "warmup_ticks": warmup, "timed_ticks": reps,
           "message_bytes_per_tick": sent // reps, "ratio": round(sent / blocks, 3),
           "written_differing_from_dropin": differing, "messages_compared": n * (warmup + reps)}
    for k, r in rec.items():
        out[k] = {f: med(v) for f, v in r.items()}
    return out


def seed_share(log):
    """tamd_compress_batch, one message per job, 1,024 streams x 40 messages (the later jobs have a
    full window), under TONK_AMD_LZ_PROF: the library prints the jobs' mean phase times."""
    os.environ["TONK_AMD_LZ_PROF"] = "1"
    import torch
    from tonk_amd.compress import compress_batch
    rng = np.random.default_rng(7)
    corp, text_bytes = corpus(rng, 1 << 20)
    n_streams, per = 1024, 40
    lens, _, rows, stride = draw_tick(rng, corp, text_bytes, n_streams, per)
    d_rows = torch.from_numpy(rows).cuda()
    d_out = torch.empty(n_streams * per * MAX, dtype=torch.uint8, device="cuda")
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            for _ in range(2):
                compress_batch(d_rows.data_ptr(), stride, n_streams, per, lens.reshape(-1), MAX, d_out.data_ptr(), msgs_per_job=1)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode()
    line = [ln for ln in text.splitlines() if ln.startswith("lz phases")][-1]
    print(line, file=log)
    us = {k: float(v) for k, v in re.findall(r"(window|probe|parse|codes\+tables|chains|stream|out) ([0-9.]+)", line)}
    total = sum(us.values())
    return {"streams": n_streams, "messages_per_stream": per, "us_per_job": us, "window_share": round(us["window"] / total, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ticks", default="wide,deep")
    ap.add_argument("--seed-share", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to the JSON an earlier run left in --out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cbatch_time: no GPU (there is no CPU path to time)")
    result = {"max_message_bytes": MAX, "message_bytes": [LO, HI], "dropin_threads": THREADS}
    if a.seed_share:
        result["seed_share"] = seed_share(sys.stderr)
    import tonk_amd
    for name in a.ticks.split(","):
        if name:
            result[name] = run_tick(torch, tonk_amd, name, *TICKS[name], a.reps, sys.stderr)
    if a.out and a.append and os.path.exists(a.out):  # (a tick per process: every drop-in's ring is fresh memory)
        with open(a.out) as f:
            result = dict(json.load(f), **result)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
