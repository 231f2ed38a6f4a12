"""Batched adds leave the codecs' windows exactly as single adds do, and the session backend's
computed input handles are the ones its table held.

The encoder keeps nothing per element: segments for the packets and time runs for the send times
(encoder.h), so an add costs the same for every run length.  tests/native/window_check drives two
encoders through one seeded schedule -- adds of 1-63 packets (Encoder::add_run against single
Encoder::add calls), clock steps of 0-30 ms, acknowledgements with 0-3 loss ranges that cut
segments mid-run, retransmit ticks and encodes -- and compares after every call each live
element's view (row, offset, bytes, column, send time), remaining_slots, the RTO, the next and
next-expected columns, and every retransmit and encode result; each send time is also held against
a per-element record the tool keeps itself.  The same for Decoder::add_run_inorder against
add_original: acknowledgement bytes (next expected and got bits), every element's packet, statistics.

Shapes: windows of at most 300 unacknowledged elements, 2,000 originals, 100 seeds from column 0
(windows restart at columns that are no multiple of 8 whenever an acknowledgement empties them:
placeholders), and fewer seeds from a start column with column % 8 != 0 and from 2^22 - 100, where
runs cross the column wrap (reaching that column takes 4 M adds per encoder, so 5 seeds).  The
decoder's window only starts at column 0: it moves on by decoding, which this tool does not do.

tests/native/handle_check compares ResidentBackend::row and run_rows with the table alloc_inputs
used to fill, for every index: pool a power of two, not one, n no multiple of the pool, a pool of
one row (the stored table), with and without contig.
"""
import json
import os
import subprocess

import pytest

from conftest import NATIVE, _make


@pytest.fixture(scope="module")
def tools():
    _make(NATIVE, "-f", "window_check.mk")
    return os.path.join(NATIVE, "_build")


def run(tool, *args):
    r = subprocess.run([tool, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


@pytest.mark.parametrize("seeds,start", [(100, 0), (20, 5), (5, (1 << 22) - 100), (5, (1 << 22) - 3)])
def test_encoder_window_runs(tools, seeds, start):
    got = run(os.path.join(tools, "window_check"), "enc", f"seeds={seeds}", "n=2000", f"start={start}")
    assert got["seeds"] == seeds and got["checks"] > 50 * seeds
    # the schedules reached what they are for
    for key in ("retransmits", "encodes", "loss_ranges", "placeholder_windows"):
        assert got[key] > 0, key


def test_decoder_window_runs(tools):
    got = run(os.path.join(tools, "window_check"), "dec", "seeds=100", "n=2000")
    assert got["seeds"] == 100 and got["checks"] > 30 * 100


def test_computed_handles(tools):
    got = run(os.path.join(tools, "handle_check"))
    assert got["cases"] == 20 and got["compared"] > 100000
