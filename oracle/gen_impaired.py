#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: generate the impaired-channel fixtures from the REFERENCE codec.

Runs `oracle/_ref/golden_gen impaired` (the driver of oracle/impaired.h linked against the
reference Siamese codec) for every scenario below and writes

  tests/golden/imp_<name>.txt.gz   full transcript (gzip, mtime 0)
  tests/golden/impaired.json       args, sha256 and summary line of each

tests/golden/scenarios.json and the fixtures of oracle/gen_golden.py are not touched.  As there,
the reference memcmp-checks every recovered packet against the true payload while it runs
(golden_gen exits non-zero otherwise), so no fixture can pin a wrong decode.

usage: python oracle/gen_impaired.py
"""
from __future__ import annotations

import gzip
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from tonk_amd import WorkloadParams  # noqa: E402  (parameter helpers only)

GEN = os.path.join(HERE, "_ref", "golden_gen")
OUT = os.path.join(ROOT, "tests", "golden")


def q32(p: float) -> int:
    """A probability as a threshold on a 32-bit draw (as the loss threshold)."""
    return min(0xFFFFFFFF, int(p * 4294967296.0))


def impair(reorder=0.0, reach=1, dup=0.0, ackloss=0.0, ackdelay=0.0, ackreach=0, ackdup=0.0, hold_first=0, seed=3000):
    return [f"reorder={q32(reorder)}", f"reach={reach}", f"dup={q32(dup)}", f"ackloss={q32(ackloss)}",
            f"ackdelay={q32(ackdelay)}", f"ackreach={ackreach}", f"ackdup={q32(ackdup)}", f"hold_first={hold_first}",
            f"seed_impair={seed}"]


def scenarios():
    """name -> (WorkloadParams, impairment arguments, note)"""
    s = {}
    s["imp_near"] = (WorkloadParams(n=2000, loss=0.02, ack=64), impair(reorder=0.15, reach=8, dup=0.03),
                     "short reordering and a few duplicates")
    s["imp_far"] = (WorkloadParams(n=3000, loss=0.02, ack=32), impair(reorder=0.05, reach=300),
                    "packets arrive after the window has passed them")
    s["imp_recfirst"] = (WorkloadParams(n=600, loss=0.02, fec=0.25, ack=16), impair(hold_first=40),
                         "the first 40 originals held past the first recovery packets: an empty decoder takes its "
                         "window from a recovery packet")
    s["imp_var_dup"] = (WorkloadParams(n=2000, payload=1, payload_max=1500, loss=0.03, ack=32),
                        impair(reorder=0.10, reach=40, dup=0.10), "variable lengths, many duplicates")
    s["imp_acks"] = (WorkloadParams(n=3000, loss=0.02, ack=16),
                     impair(ackloss=0.30, ackdelay=0.30, ackreach=3, ackdup=0.10),
                     "acknowledgements dropped, stale and repeated; packets in order")
    s["imp_burst_arq"] = (WorkloadParams(n=3000, loss=0.05, burst=8, fec=0.10, ack=128, arq=200),
                          impair(reorder=0.10, reach=250, dup=0.05),
                          "bursts, and ARQ copies that overtake held first copies")
    s["imp_rtx"] = (WorkloadParams(n=2000, loss=0.05, ack=32, rtx=8, rtx_msec=3),
                    impair(reorder=0.10, reach=30, ackloss=0.20), "retransmission under the virtual clock")
    # (with retransmission on, a repeated acknowledgement taken for a new one would move the RTO)
    s["imp_all"] = (WorkloadParams(n=3000, payload=1, payload_max=1500, loss=0.03, ack=32, arq=400, rtx=8, rtx_msec=3),
                    impair(reorder=0.08, reach=60, dup=0.04, ackloss=0.10, ackdelay=0.15, ackreach=2, ackdup=0.15),
                    "everything on at moderate rates")
    # most acknowledgements lost: the encoder's sums live long, the decoder's window start moves
    # past their first column, and when an acknowledgement does get through the sums restart; a
    # held row of the old sums then arrives with a loss still open ("sum region clipped")
    s["imp_clip"] = (WorkloadParams(n=3000, loss=0.05, burst=3, fec=0.12, ack=8),
                     impair(reorder=0.30, reach=60, ackloss=0.70), "old Siamese sums arriving after the sums restarted")
    return s


def run(wp: WorkloadParams, imp: list[str]) -> str:
    args = [GEN, "impaired", "/dev/stdout"] + wp.args() + imp + ["seed_data=1000", "seed_loss=2000"]
    r = subprocess.run(args, capture_output=True, check=True)
    return r.stdout.decode()


def main() -> int:
    if not os.path.exists(GEN):
        print("build the reference first: make -C oracle", file=sys.stderr)
        return 2
    os.makedirs(OUT, exist_ok=True)
    index = {"generator": "oracle/_ref/golden_gen impaired (reference codec, oracle/impaired.h)", "scenarios": {}}
    for name, (wp, imp, note) in scenarios().items():
        text = run(wp, imp)
        lines = text.strip().splitlines()
        # a decoder that gave up (Siamese_Disabled from a decoder call) is part of the specification
        disabled = any(ln.split()[:2] in (["D", "5"], ["O", "5"], ["R", "5"]) or
                       (ln[0] in "HQ" and ln.split()[3] == "5") for ln in lines)
        index["scenarios"][name] = {"args": wp.args() + imp, "sha256": hashlib.sha256(text.encode()).hexdigest(),
                                    "lines": len(lines), "summary": lines[-1], "file": f"{name}.txt.gz",
                                    "note": note, "decoder_disabled": disabled}
        with open(os.path.join(OUT, f"{name}.txt.gz"), "wb") as raw, \
                gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
            f.write(text.encode())
        print(f"{name}: {len(lines)} lines{' DISABLED' if disabled else ''} {lines[-1]}")
    with open(os.path.join(OUT, "impaired.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
