"""CPU parity of the engine's host control plane (no GPU).

tests/native/cp_harness drives tonk_amd/csrc/{encoder,decoder,engine}.cpp through each golden
scenario; the device programs they emit are executed by the oracle's CPU interpreter of the
program format (oracle_run_program).  The resulting transcript -- every recovery packet digest,
every decode with recovered-payload digests, every acknowledgement, the codec statistics --
must equal the REFERENCE codec's transcript byte for byte.

Modes: ``sync`` runs each program as soon as a result is needed (one program per API call, as
the C-ABI does); ``batch`` defers execution over ``batch`` originals (as the device-resident
session does), which exercises chain snapshots, expansion of in-flight rows and multi-level
programs; ``batch-pipe`` adds the session's level pipelining (a program's upper levels run
beside the next program's first levels) and checks those pairs for read/write hazards.
"""
from __future__ import annotations

import os
import subprocess

import pytest

from conftest import NATIVE, _make, first_diff, golden_text

SCENARIOS = ["c1_256_p3", "c2_4096_p1_ack64", "c2_4096_p1_noack", "c3_4096_p2_ack64_s0",
             "c3_4096_p2_ack64_s1", "c3_4096_p2_ack64_s63", "c4_4096_p1_ack64_s511", "c5_65536_ge5_b4",
             "var_1_1500_p2_ack32", "tiny_1_20_p5_ack16", "big_9000_p3_ack64", "hiloss_p20_arq",
             "norecloss_p5_arq", "single_p0", "burst8_p5", "rtx_p2_ack64", "rtx_p5_ack32", "rtx_p3_noack",
             "rtx_restart_p1_ack4", "rtx_restart_p2_ack2"]
MODES = [("sync", 0), ("batch", 1000), ("batch", 4096), ("sync-dirty", 0), ("batch-dirty", 1000),
         ("batch-pipe", 1000), ("batch-pipe", 4096), ("batch-pipedrain", 1000), ("batch-pipeexp", 512),
         ("batch-pipesplit", 1000), ("sync-exp", 0), ("batch-pipecontig", 4096), ("batch-pipecontigsplit", 1000)]


@pytest.fixture(scope="module")
def harness():
    _make(NATIVE, "_build/cp_harness")
    return os.path.join(NATIVE, "_build", "cp_harness")


@pytest.mark.parametrize("mode,batch", MODES)
@pytest.mark.parametrize("name", SCENARIOS)
def test_control_plane_matches_reference(harness, golden_index, tmp_path, name, mode, batch):
    sc = golden_index["scenarios"][name]
    sid = sc["stream"]
    out = tmp_path / "t.txt"
    # "-dirty": flushes visit only the codecs touched since the last one (the C ABI's context);
    # "-pipe": levels pipelined across programs as the session launches them, every pair of
    # levels that would run together checked for hazards; "-pipedrain": every second program
    # also completes all in-flight ones (the session's record mode), so rows are reused sooner
    base, dirty = mode.split("-")[0], int(mode.endswith("-dirty"))
    # "-pipeexp": also the few-stream session's expansion limit (expansions over 16 terms are
    # read as rows, one level up) and its back substitution over materialized rows (from 2
    # unknowns)
    pipe, drain = int("-pipe" in mode), 2 * int(mode.endswith("-pipedrain"))
    # "-exp" alone: the same limits on per-call programs (the siamese.h C ABI's contexts)
    few = mode.endswith("exp")
    expand = 16 if few else 0xFFFFFFFF
    backsub = 2 if few else 0xFFFFFFFF
    # the batched session splits direct dense ranges over 48 packets (Context::dense_split);
    # "-pipesplit" splits every range over 16, so most Siamese rows take the two-level form
    split = 16 if mode.endswith("split") else 48 if mode in ("batch-pipe", "batch-pipedrain", "batch-pipecontig") else 0
    # "-pipecontig": every original in a row reserved up front, in order, borrowed by the codecs
    # (the batched session's layout): windows are long segments, so Siamese rows read their sum
    # ranges straight from the packets and consecutive ones are grouped (Encoder::defer_dense)
    contig = int("contig" in mode)
    # (every mode also checks that no op of a level writes a row another op of that level uses)
    # "sync-exp" and "batch-dirty" also encode ahead as the C ABI does (Encoder::encode_is_quiet,
    # rewind): up to 15 and 3 recovery packets
    ahead = 15 if mode == "sync-exp" else 3 if mode == "batch-dirty" else 0
    # ... and "sync-exp" / "batch-pipeexp" take the C ABI's and the few-stream session's lane-sum
    # snapshot levels (Context::short_scans)
    short = int(mode in ("sync-exp", "batch-pipeexp"))
    args = [harness, str(out), f"mode={base}", f"batch={batch}", f"dirty={dirty}", f"pipeline={pipe}",
            f"drain={drain}", f"expand={expand}", f"backsub={backsub}", f"split={split}", f"contig={contig}",
            f"ahead={ahead}", f"short={short}"] + sc["args"] + [
        f"seed_data={1000 + sid}", f"seed_loss={2000 + sid}"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = out.read_text()
    want = golden_text(name)
    assert got == want, first_diff(want, got)


@pytest.mark.parametrize("mode", [["mode=batch", "batch=4096"], ["mode=batch", "batch=1000", "pipeline=1", "split=48", "contig=1"],
                                  ["mode=sync", "dirty=1", "expand=16", "backsub=2"]])
@pytest.mark.parametrize("name", ["c2_4096_p1_ack64", "c3_4096_p2_ack64_s63", "c5_65536_ge5_b4", "hiloss_p20_arq",
                                  "burst8_p5", "big_9000_p3_ack64"])
def test_control_plane_lane_eliminations(harness, golden_index, tmp_path, name, mode):
    """The decoder's Siamese-row eliminations through its running lane sums only (ddirect=0), the
    path rows with long or fragmented sum ranges take (the default reads short ranges of long
    runs straight from the packets, Decoder::eliminate_direct): transcript == reference's."""
    sc = golden_index["scenarios"][name]
    sid = sc["stream"]
    out = tmp_path / "t.txt"
    r = subprocess.run([harness, str(out), "ddirect=0"] + mode + sc["args"] +
                       [f"seed_data={1000 + sid}", f"seed_loss={2000 + sid}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = golden_text(name)
    assert out.read_text() == want, first_diff(want, out.read_text())


@pytest.mark.parametrize("contig", [0, 1])
@pytest.mark.parametrize("batch_name,sid", [("cfg2_64x4096_p2_ack64", 0), ("cfg2_64x4096_p2_ack64", 37),
                                             ("cfg3_rank7_64x12288_p1_ack64", 448),
                                             ("cfg3_rank7_64x12288_p1_ack64", 511)])
def test_control_plane_batch_streams(harness, golden_index, tmp_path, batch_name, sid, contig):
    """Streams of the multi-stream fixtures (BASELINE configs[2], the rank-7 shard of configs[3])
    through the control plane in the bench's batch mode, pipelined as the session launches it in
    record mode: transcript digest == reference's, no launch-order hazard."""
    import hashlib
    entry = golden_index["batches"][batch_name]
    out = tmp_path / "t.txt"
    args = [harness, str(out), "mode=batch", "batch=4096", "dirty=0", "pipeline=1", "drain=2", "split=48",
            f"contig={contig}"] + entry["args"] + [
        f"seed_data={1000 + sid}", f"seed_loss={2000 + sid}"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert hashlib.sha256(out.read_bytes()).hexdigest() == entry["streams"][str(sid)]["sha256"]


@pytest.mark.parametrize("family,streams", [("cfg2", range(48, 64)), ("cfg4", range(0, 3)), ("p5_ack32", range(0, 8))])
def test_control_plane_vs_reference_build(harness, tmp_path, family, streams):
    """Whole streams through the control plane against transcripts the reference codec compiled
    from /root/reference (oracle/_ref/golden_gen, built by __graft_entry__.build) writes for the
    same seeds: configs[2] streams 48-63 (stream 56 is the decoder far behind whose thousands of
    failed solves Decoder::decode counts instead of repeating, with the list walks it caches), the
    decoder-stress configs[4] and a 5 %-loss family, in the C ABI's per-call mode with
    encode-ahead and in the batched session's mode."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "golden_gen")
    if not os.path.exists(exe):
        pytest.skip("reference build absent (oracle/_ref)")
    args = {
        "cfg2": "n=4096 pmin=1300 pmax=1300 loss=85899345 ge=0 gb=0 bg=0 lossrec=1 fec=2621 ack=64 ackbytes=256 arq=0 flush=4096",
        "cfg4": "n=65536 pmin=1300 pmax=1300 loss=0 ge=1 gb=56512727 bg=1073741824 lossrec=1 fec=6554 ack=256 ackbytes=256 arq=2048 flush=4096",
        "p5_ack32": "n=4096 pmin=1300 pmax=1300 loss=214748364 ge=0 gb=0 bg=0 lossrec=1 fec=5243 ack=32 ackbytes=256 arq=0 flush=4096",
    }[family].split()
    first = min(streams)
    ref = subprocess.run([exe, "transcripts", str(tmp_path / "r"), "threads=4", f"streams={max(streams) + 1 - first}",
                          f"stream={first}"] + args, capture_output=True, text=True, timeout=600)
    assert ref.returncode == 0, ref.stderr[-2000:]
    modes = [["mode=sync", "dirty=1", "expand=16", "backsub=2", "ahead=15", "short=1"],
             ["mode=batch", "batch=4096", "pipeline=1", "drain=2", "split=48", "contig=1"]]
    for s in streams:
        want = (tmp_path / f"r{s}.txt").read_text()
        for m in modes:
            out = tmp_path / "o.txt"
            r = subprocess.run([harness, str(out)] + m + args + [f"stream={s}", f"seed_data={1000 + s}",
                                                                 f"seed_loss={2000 + s}"],
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            assert out.read_text() == want, f"stream {s} {m}: " + first_diff(want, out.read_text())


@pytest.mark.parametrize("name,mode", [
    ("wrap_p1_ack256_64B", ["mode=sync", "dirty=1", "expand=16", "backsub=2", "ahead=15", "short=1"]),
    ("wrap_p1_ack256_64B", ["mode=batch", "batch=4096", "pipeline=1", "drain=2", "split=48", "contig=1"]),
    ("wrap_p1_full_64B", ["mode=sync", "dirty=1", "expand=16", "backsub=2", "ahead=15", "short=1"]),
    ("full_p3_noack", ["mode=sync", "dirty=1", "expand=16", "backsub=2", "ahead=15", "short=1"]),
    ("full_p1_noack", ["mode=sync", "dirty=0", "expand=4294967295", "backsub=4294967295"]),
    ("full_p1_noack", ["mode=batch", "batch=4096", "pipeline=1", "drain=2", "split=48", "contig=1"]),
    ("full_p1_noack", ["mode=batch", "batch=1000", "dirty=1", "ahead=3"])])
def test_control_plane_long_streams(harness, golden_index, tmp_path, name, mode):
    """The window-full fixtures (full_*: no acks, 50,000 originals, the 16,000-packet window fills
    and a refused add waits for an acknowledgement, siamese.cpp:80-93, SiameseEncoder.cpp:91-96)
    and 4.3 M originals, past the 22-bit packet-number period (SiameseCommon.h:102): windows,
    Siamese sums, Cauchy rows and LDPC pairs straddle column 0x3FFFFF -> 0, in the C ABI's
    per-call mode and the batched session's pipelined contiguous mode.  wrap_p1_ack256: the
    reference decoder disables itself after the wrap and the encoder window fills up (the
    engine must do the same); wrap_p1_full: no acks, the 16,000-packet window fills ~360 times
    and recoveries continue across the wrap.  Transcript digest == the reference codec's.
    (The batched mode of wrap_p1_full takes ~4 minutes on one core: run by hand, not here.)"""
    import hashlib
    e = golden_index["long"].get(name) or golden_index["scenarios"][name]
    sid = e["stream"]
    out = tmp_path / "t.txt"
    r = subprocess.run([harness, str(out)] + mode + ["arena_mb=4096"] + e["args"] +
                       [f"seed_data={1000 + sid}", f"seed_loss={2000 + sid}"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    assert text.splitlines()[-1] == e["summary"]
    assert hashlib.sha256(text.encode()).hexdigest() == e["sha256"]


# ---- the impaired channel (oracle/impaired.h): reordering, duplicates, lost / stale / repeated acks ----

IMPAIRED = ["imp_near", "imp_far", "imp_recfirst", "imp_var_dup", "imp_acks", "imp_burst_arq", "imp_rtx", "imp_all",
            "imp_clip"]
IMP_SEEDS = ["seed_data=1000", "seed_loss=2000"]
# the C ABI's per-call mode, plain per-call programs, and the batched session's pipelined mode with its
# hazard checks on (contig=1 is the in-order Session's layout and is left out)
IMP_MODES = {"capi": ["mode=sync", "dirty=1", "expand=16", "backsub=2", "ahead=15", "short=1"],
             "sync": ["mode=sync"],
             "batch-pipe": ["mode=batch", "batch=1000", "pipeline=1", "drain=2", "split=48"]}


@pytest.fixture(scope="module")
def impaired_index():
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "impaired.json")) as f:
        return json.load(f)["scenarios"]


@pytest.mark.parametrize("name", ["c1_256_p3", "var_1_1500_p2_ack32", "hiloss_p20_arq", "rtx_p5_ack32", "burst8_p5"])
def test_impaired_driver_without_impairments_is_the_old_driver(harness, golden_index, tmp_path, name):
    """With every impairment zero the impaired-channel driver makes Runner's calls: through it the
    control plane writes exactly the existing golden transcripts (this ties the new driver to the
    old one without the reference)."""
    sc = golden_index["scenarios"][name]
    sid = sc["stream"]
    out = tmp_path / "t.txt"
    r = subprocess.run([harness, str(out), "mode=sync", "impaired=1"] + sc["args"] +
                       [f"seed_data={1000 + sid}", f"seed_loss={2000 + sid}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = golden_text(name)
    assert out.read_text() == want, first_diff(want, out.read_text())


@pytest.mark.parametrize("name,mode", [(n, m) for n in IMPAIRED for m in IMP_MODES] +
                         [("imp_far", "lanes"), ("imp_all", "lanes")])
def test_control_plane_impaired_matches_reference(harness, impaired_index, tmp_path, name, mode):
    """Every impaired fixture (late and duplicate originals and recovery packets, dropped, stale and
    repeated acknowledgements; tests/golden/impaired.json) through the control plane: transcript ==
    the reference codec's, bit for bit.  "lanes": eliminations through the lane sums only
    (ddirect=0), for the two scenarios whose packets arrive furthest out of order."""
    margs = ["mode=sync", "ddirect=0"] if mode == "lanes" else IMP_MODES[mode]
    sc = impaired_index[name]
    out = tmp_path / "t.txt"
    r = subprocess.run([harness, str(out), "impaired=1"] + margs + sc["args"] + IMP_SEEDS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want = golden_text(name)
    assert out.read_text() == want, first_diff(want, out.read_text())


def test_control_plane_impaired_vs_reference_build(harness, impaired_index, tmp_path):
    """imp_all's parameters on seeds 1..8 against transcripts the reference build
    (oracle/_ref/golden_gen impaired) writes on the spot, in the C ABI's mode and the batched one."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "golden_gen")
    if not os.path.exists(exe):
        pytest.skip("reference build absent (oracle/_ref)")
    # a reference build made before the driver had this command is brought up to date (oracle/Makefile
    # rebuilds golden_gen when its sources' contents changed), never skipped
    probe = [exe, "impaired", os.devnull, "n=1", "reorder=0"]
    if subprocess.run(probe, capture_output=True).returncode != 0:
        _make(os.path.dirname(os.path.dirname(exe)), "ref")
        r = subprocess.run(probe, capture_output=True, text=True)
        assert r.returncode == 0, "oracle/_ref/golden_gen is older than oracle/golden_gen.cpp: " + r.stderr[-500:]
    base = [a for a in impaired_index["imp_all"]["args"] if not a.startswith("seed_impair=")]
    for s in range(1, 9):
        args = base + [f"seed_data={1000 + s}", f"seed_loss={2000 + s}", f"seed_impair={3000 + s}"]
        ref = tmp_path / "r.txt"
        r = subprocess.run([exe, "impaired", str(ref)] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        want = ref.read_text()
        for m in (IMP_MODES["capi"], IMP_MODES["batch-pipe"]):
            out = tmp_path / "o.txt"
            r = subprocess.run([harness, str(out), "impaired=1"] + m + args, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            assert out.read_text() == want, f"seed {s} {m}: " + first_diff(want, out.read_text())


def test_impaired_fixtures_hold_the_cases(impaired_index):
    """The fixtures themselves (the reference's own lines, nothing run here) contain what they are
    there for.  Event lines of oracle/impaired.h: `H copy col rc` an original arriving late (copy 2:
    a second copy), `Q copy behind rc` a recovery packet arriving late (behind: its ColumnStart +
    SumCount lies below an earlier delivered one's), `L` a dropped, `V` a stale, `P` a repeated
    acknowledgement; `X` / `T` lines are ARQ and retransmitted originals with a non-zero result."""
    import hashlib
    DUPLICATE = 4
    refused = accepted = behind_used = behind_idle = dropped = stale = repeated = multi_after_late = 0
    duped_recovery_scenarios = 0
    summaries = {}
    for name in IMPAIRED:
        sc = impaired_index[name]
        text = golden_text(name)
        assert hashlib.sha256(text.encode()).hexdigest() == sc["sha256"], name
        lines = [ln.split() for ln in text.splitlines()]
        assert " ".join(lines[-1]) == sc["summary"] and lines[-1][0] == "Z"
        summaries[name] = dict(kv.split("=") for kv in lines[-1][1:])
        for i, f in enumerate(lines):
            nxt = lines[i + 1] if i + 1 < len(lines) else ["-"]
            if f[0] == "H":
                refused += int(f[3]) == DUPLICATE
                accepted += f[1] == "1" and f[3] == "0"
            elif f[0] in "XT" and len(f) == 4 and f[1] == str(DUPLICATE):
                refused += 1
            elif f[0] == "Q" and f[2] == "1" and f[3] == "0":
                # a late row that completes a solve is used by it; one followed by no decode is not (yet)
                if nxt[0] == "D" and nxt[1] == "0" and int(nxt[2]) >= 1:
                    behind_used += 1
                elif nxt[0] != "D":
                    behind_idle += 1
            dropped += f[0] == "L"
            stale += f[0] == "V"
            repeated += f[0] == "P"
            if f[0] in "HQ" and nxt[0] == "D" and nxt[1] == "0" and int(nxt[2]) >= 2:
                multi_after_late += 1
        stats = [f for f in lines if f[0] == "S"]
        assert len(stats) == 1
        dec = stats[0][stats[0].index("|") + 1:]
        duped_recovery_scenarios += int(dec[9]) > 0  # SiameseDecoderStats_DupedRecoveryCount
    assert refused > 0 and accepted > 0
    assert behind_used > 0 and behind_idle > 0
    assert duped_recovery_scenarios >= 4
    assert dropped > 0 and stale > 0 and repeated > 0
    assert multi_after_late > 0
    # imp_recfirst: its first originals are all lost or held (they arrive as H lines), so every
    # recovery packet encoded before the first H line that the channel did not lose met a decoder
    # that had seen no original -- and more were encoded than the channel lost in the whole stream
    rf = [ln.split() for ln in golden_text("imp_recfirst").splitlines()]
    hold = int(dict(a.split("=") for a in impaired_index["imp_recfirst"]["args"])["hold_first"])
    first_h = next(i for i, f in enumerate(rf) if f[0] == "H")
    early = sum(1 for f in rf[:first_h] if f[0] == "E" and f[1] == "0")
    assert hold > 0 and early > int(summaries["imp_recfirst"]["lostrec"])
    # the reference recovers what it is sent: nothing wrong anywhere, and at least six of the
    # first eight scenarios end with nothing missing
    assert all(s["bad"] == "0" for s in summaries.values())
    assert sum(summaries[n]["missing"] == "0" for n in IMPAIRED[:8]) >= 6
    for name in IMPAIRED:
        assert impaired_index[name]["decoder_disabled"] == any(
            ln.split()[:2] in (["D", "5"], ["O", "5"], ["R", "5"]) or (ln[0] in "HQ" and ln.split()[3] == "5")
            for ln in golden_text(name).splitlines()), name
