"""GPU parity tests (MI355X): the HIP path must reproduce the reference codec bit for bit.

Every scenario's transcript -- the digest of every recovery packet (data + footer), every
decode result with the digest of each recovered payload, every acknowledgement, the final
stats -- is compared with the golden transcript produced by the REFERENCE codec
(tests/golden, oracle/gen_golden.py).  Two device paths are checked:

* the siamese.h C-ABI (drop-in path): oracle/golden_gen.cpp's driver linked against
  libtonk_amd.so instead of the reference library (tests/native/_build/capi_gen);
* the batched device-resident session (bench path) in record mode.
"""
from __future__ import annotations

import os
import re
import subprocess

import pytest

from conftest import NATIVE, ROOT, first_diff, golden_text, sha256

pytestmark = pytest.mark.gpu

SCEN_CAPI = ["c1_256_p3", "c2_4096_p1_ack64", "c2_4096_p1_noack", "c3_4096_p2_ack64_s0",
             "var_1_1500_p2_ack32", "tiny_1_20_p5_ack16", "big_9000_p3_ack64", "hiloss_p20_arq",
             "norecloss_p5_arq", "single_p0", "burst8_p5", "c5_65536_ge5_b4",
             "rtx_p2_ack64", "rtx_p5_ack32", "rtx_p3_noack",
             "rtx_restart_p1_ack4", "rtx_restart_p2_ack2", "full_p1_noack", "full_p3_noack"]
SCEN_SESSION = ["c1_256_p3", "c2_4096_p1_ack64", "c2_4096_p1_noack", "c3_4096_p2_ack64_s1",
                "c3_4096_p2_ack64_s63", "c4_4096_p1_ack64_s511", "var_1_1500_p2_ack32",
                "tiny_1_20_p5_ack16", "big_9000_p3_ack64", "hiloss_p20_arq", "single_p0",
                "burst8_p5", "c5_65536_ge5_b4", "rtx_p2_ack64", "rtx_p3_noack", "rtx_restart_p1_ack4",
                "full_p1_noack", "full_p3_noack"]


def _args(golden_index, name):
    sc = golden_index["scenarios"][name]
    sid = sc["stream"]
    return sc["args"] + [f"seed_data={1000 + sid}", f"seed_loss={2000 + sid}"], sid


def test_device_gf_selftest():
    import tonk_amd
    tonk_amd.device_selftest(0)


@pytest.mark.parametrize("name", SCEN_CAPI)
def test_capi_matches_reference(golden_index, name):
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    assert os.path.exists(exe), "build tests/native first (make -C tests/native)"
    args, _ = _args(golden_index, name)
    out = subprocess.run([exe, "transcript", "/dev/stdout"] + args, capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = out.stdout.decode()
    want = golden_text(name)
    assert got == want, first_diff(want, got)


def _session_transcript(golden_index, name, threads=1, stage_host=False, step=1000):
    import tonk_amd
    sc = golden_index["scenarios"].get(name) or golden_index["long"][name]
    wp = tonk_amd.WorkloadParams.from_args(sc["args"])
    arena = max(1 << 30, 2 * wp.n * (wp.pmax + 64) + (2 << 30))
    s = tonk_amd.Session(wp, n_streams=1, stream_base=sc["stream"], threads=threads,
                         arena_bytes=arena, record=True, stage_host=stage_host)
    try:
        s.generate()
        n = wp.n
        done = 0
        while done < n:
            s.step(min(step, n - done))
            done += step
        s.finish()
        return s.transcript(0), s.summary()
    finally:
        s.close()


@pytest.mark.parametrize("name", SCEN_SESSION)
def test_session_matches_reference(golden_index, name):
    got, summ = _session_transcript(golden_index, name)
    want = golden_text(name)
    want = "\n".join(l for l in want.splitlines() if not l.startswith("Z ")) + "\n"
    assert got == want, first_diff(want, got)
    assert summ["missing_at_end"] == 0
    assert summ["disabled_codecs"] == 0


@pytest.mark.parametrize("name,mask", [("c2_4096_p1_ack64", 3), ("c3_4096_p2_ack64_s1", 3), ("burst8_p5", 3),
                                       ("c3_4096_p2_ack64_s1", 1), ("c3_4096_p2_ack64_s1", 2)])
def test_session_host_staged_matches_reference(golden_index, name, mask):
    """Packets staged through pinned host memory (the PCIe-inclusive path: H2D of the inputs
    before every step's program, D2H of its outputs) give the same transcript -- with both ends
    of the connection staged (3), the sender's only (1) or the receiver's only (2)."""
    got, summ = _session_transcript(golden_index, name, stage_host=mask)
    want = golden_text(name)
    want = "\n".join(l for l in want.splitlines() if not l.startswith("Z ")) + "\n"
    assert got == want, first_diff(want, got)
    assert summ["h2d_bytes"] > 0 and summ["d2h_bytes"] > 0
    assert summ["d2h_copy_us"] > 0


def _batch_digests(entry, threads=16, step=4096):
    """Run every stream of a golden batch through ONE batched session on one GPU (4096 originals
    per step, as the bench) and return the stream ids whose transcript digest differs."""
    import tonk_amd
    wp = tonk_amd.WorkloadParams.from_args(entry["args"])
    base = int(entry.get("stream_base", 0))
    n_streams = len(entry["streams"])
    arena = 2 * wp.n * n_streams * 1344 + (4 << 30)
    s = tonk_amd.Session(wp, n_streams=n_streams, stream_base=base, threads=threads, arena_bytes=arena, record=True)
    try:
        s.generate()
        done = 0
        while done < wp.n:
            s.step(min(step, wp.n - done))
            done += step
        s.finish()
        bad = []
        for i in range(n_streams):
            t = s.transcript(i)
            want = entry["streams"][str(base + i)]
            # the golden digest covers the transcript plus its Z summary line
            if sha256(t + want["summary"] + "\n") != want["sha256"]:
                bad.append(base + i)
        summ = s.summary()
        # the reference does not always finish: stream 56 of cfg2 keeps 4 originals unrecovered
        # after the 4096-packet end-of-stream flush; the session must agree stream by stream
        want_missing = sum(int(v["summary"].split("missing=")[1].split()[0]) for v in entry["streams"].values())
        assert summ["missing_at_end"] == want_missing and summ["disabled_codecs"] == 0, summ
        return bad
    finally:
        s.close()


def test_session_bench_config_streams(golden_index):
    """Bench configuration (64 streams x 49152 originals, 1% loss, ack 64): every stream's full
    transcript digest equals the reference's, with 16 host threads as in the bench."""
    bad = _batch_digests(golden_index["bench"])
    assert not bad, f"streams differing from the reference: {bad}"


def test_session_one_large_step(golden_index):
    """The bench configuration's 64 streams x 49152 originals as ONE step: the program is ~12x
    what the free-running schedule's staging slots start with, so the session must grow them
    (between programs, nothing in flight) instead of failing; every transcript still equals the
    reference's."""
    bad = _batch_digests(golden_index["bench"], step=49152)
    assert not bad, f"streams differing from the reference: {bad}"


@pytest.mark.parametrize("name", ["cfg2_64x4096_p2_ack64", "cfg3_rank7_64x12288_p1_ack64"])
def test_session_batch_matches_reference(golden_index, name):
    """BASELINE.json configs[2] as specified (64 independent streams x 4096 originals, 2% loss,
    one batched session on one GPU) and the shard rank 7 of 8 runs in configs[3] (streams
    448..511): every stream's transcript digest equals the reference codec's."""
    bad = _batch_digests(golden_index["batches"][name])
    assert not bad, f"streams differing from the reference: {bad}"


def test_capi_concurrent_codecs(golden_index, tmp_path):
    """Sixteen encoder/decoder pairs driven through the siamese.h C ABI from eight threads at
    once (each codec on one thread at a time, as siamese.h:58-59 requires): every stream's
    transcript equals the reference codec's (BASELINE configs[2] streams 0..15)."""
    import hashlib
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    entry = golden_index["batches"]["cfg2_64x4096_p2_ack64"]
    prefix = str(tmp_path / "s")
    out = subprocess.run([exe, "transcripts", prefix, "threads=8", "streams=16", "stream=0"] + entry["args"],
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    bad = [s for s in range(16)
           if hashlib.sha256(open(f"{prefix}{s}.txt", "rb").read()).hexdigest() != entry["streams"][str(s)]["sha256"]]
    assert not bad, f"streams differing from the reference: {bad}"


@pytest.mark.parametrize("name", ["c2_4096_p1_noack", "big_9000_p3_ack64"])
def test_capi_arena_growth(golden_index, name):
    """The C ABI arena starts at 2 MB with 64 KB segments, far below what these streams hold
    (a 4096-packet window; 9000-byte packets): it must grow, not fail, and the transcript must
    still equal the reference's (the reference only refuses past SIAMESE_MAX_PACKETS)."""
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    args, _ = _args(golden_index, name)
    env = dict(os.environ, TONK_AMD_ARENA_MB="2", TONK_AMD_SEGMENT_KB="64")
    out = subprocess.run([exe, "transcript", "/dev/stdout"] + args, capture_output=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    want = golden_text(name)
    assert out.stdout.decode() == want, first_diff(want, out.stdout.decode())


def test_capi_oversize_programs(golden_index, tmp_path):
    """Programs larger than a C ABI staging slot run in the oversize slot (here: 64 KB slots, a
    256 KB oversize slot that must also grow once), with eight threads of codecs sharing the
    device: every stream's transcript still equals the reference codec's."""
    import hashlib
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    entry = golden_index["batches"]["cfg2_64x4096_p2_ack64"]
    prefix = str(tmp_path / "s")
    env = dict(os.environ, TONK_AMD_CAPI_SLOT_KB="64", TONK_AMD_CAPI_OVERSIZE_KB="256")
    out = subprocess.run([exe, "transcripts", prefix, "threads=8", "streams=8", "stream=0"] + entry["args"],
                         capture_output=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    bad = [s for s in range(8)
           if hashlib.sha256(open(f"{prefix}{s}.txt", "rb").read()).hexdigest() != entry["streams"][str(s)]["sha256"]]
    assert not bad, f"streams differing from the reference: {bad}"


def test_capi_device_failure_disables_codec(golden_index):
    """A device failure (injected: every program after the 20th fails to stage) must surface as
    Siamese_Disabled from siamese_encode / siamese_decode -- never as Success with stale bytes:
    the driver memcmp-checks every recovered packet (exit 5 on a wrong one)."""
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    args, _ = _args(golden_index, "c2_4096_p1_ack64")
    env = dict(os.environ, TONK_AMD_FAIL_AFTER_PROGRAMS="20")
    out = subprocess.run([exe, "transcript", "/dev/stdout"] + args, capture_output=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert "E 5" in lines, "encode never reported Siamese_Disabled after the device failure"
    assert lines[-1].endswith("bad=0")


def test_capi_arena_grows_past_many_chunks(golden_index, tmp_path):
    """32 codec pairs alive at once with 48 MB segments each need about 3 GB: the C ABI arena
    (256 MB to start here) maps chunk after chunk of its reserved range, and every stream still
    matches the reference."""
    import hashlib
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    entry = golden_index["batches"]["cfg2_64x4096_p2_ack64"]
    prefix = str(tmp_path / "s")
    env = dict(os.environ, TONK_AMD_SEGMENT_KB=str(48 << 10), TONK_AMD_ARENA_MB="256")
    out = subprocess.run([exe, "transcripts", prefix, "threads=32", "streams=32", "stream=0"] + entry["args"],
                         capture_output=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert b"cannot grow" not in out.stderr and b"disabled" not in out.stderr, out.stderr.decode()[-2000:]
    bad = [s for s in range(32)
           if hashlib.sha256(open(f"{prefix}{s}.txt", "rb").read()).hexdigest() != entry["streams"][str(s)]["sha256"]]
    assert not bad, f"streams differing from the reference: {bad}"


def _capi_transcript(golden_index, name, env_extra, timeout=600):
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    args, _ = _args(golden_index, name)
    env = dict(os.environ, **env_extra)
    out = subprocess.run([exe, "transcript", "/dev/stdout"] + args, capture_output=True, timeout=timeout, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return out.stdout.decode(), out.stderr.decode()


@pytest.mark.parametrize("name", ["c2_4096_p1_ack64", "hiloss_p20_arq", "rtx_restart_p1_ack4", "c5_65536_ge5_b4"])
def test_capi_launch_path_matches_reference(golden_index, name):
    """The C ABI with the persistent executor off (TONK_AMD_SERVE=0): every call takes the kernel
    launch path that commands over 64 KB take with it on, and the transcript is the reference's."""
    got, _ = _capi_transcript(golden_index, name, {"TONK_AMD_SERVE": "0"})
    want = golden_text(name)
    assert got == want, first_diff(want, got)


@pytest.mark.parametrize("name", ["c2_4096_p1_noack", "norecloss_p5_arq", "rtx_p2_ack64"])
def test_capi_no_encode_ahead_matches_reference(golden_index, name):
    """Encode-ahead off (TONK_AMD_CAPI_AHEAD=0): one device round trip per siamese_encode."""
    got, _ = _capi_transcript(golden_index, name, {"TONK_AMD_CAPI_AHEAD": "0"})
    want = golden_text(name)
    assert got == want, first_diff(want, got)


@pytest.mark.parametrize("env", [{"TONK_AMD_WAIT_PARK": "0"}, {"TONK_AMD_WAIT_SPIN_US": "0"}])
def test_capi_wait_modes_match_reference(golden_index, env):
    """Completion waits: the round-5 polling waits (TONK_AMD_WAIT_PARK=0), and every wait parked at
    once (TONK_AMD_WAIT_SPIN_US=0: the poller thread wakes each caller), eight codec pairs on four
    threads: every stream's transcript is the reference's."""
    import hashlib
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    entry = golden_index["batches"]["cfg2_64x4096_p2_ack64"]
    prefix = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"waitmode_{os.getpid()}_")
    out = subprocess.run([exe, "transcripts", prefix, "threads=4", "streams=8", "stream=0"] + entry["args"],
                         capture_output=True, timeout=600, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    for s in range(8):
        text = open(f"{prefix}{s}.txt", "rb").read()
        os.remove(f"{prefix}{s}.txt")
        assert hashlib.sha256(text).hexdigest() == entry["streams"][str(s)]["sha256"], f"stream {s}"


def test_capi_executor_idle_exit_and_relaunch(golden_index):
    """The persistent executor ends after 0.02 ms without a command (TONK_AMD_SERVE_IDLE_MS), so
    it ends and is relaunched between the driver's calls over and over: the transcript is still
    the reference's, and the watchdog shows more than one launch."""
    name = "c3_4096_p2_ack64_s0"
    got, err = _capi_transcript(golden_index, name, {"TONK_AMD_SERVE_IDLE_MS": "0.02", "TONK_AMD_CAPI_WATCH": "0.1"})
    want = golden_text(name)
    assert got == want, first_diff(want, got)
    launches = [int(m.group(1)) for ln in err.splitlines() if "server: posted=" in ln or "executor stop:" in ln
                for m in [re.search(r"launches=(\d+)", ln)] if m]
    assert launches and max(launches) > 1, err[-2000:]


def test_capi_dead_server_falls_back_and_never_reuses(golden_index, tmp_path):
    """A command that times out (TONK_AMD_SERVE_TIMEOUT_US=1: the first wait does) kills the
    persistent executor for the process: its codec is disabled and keeps its buffers and rows
    (the command may still run), every later call takes the launch path.  Sixteen codec pairs on
    eight threads, created and freed around the dead server: no wrong byte anywhere (the driver
    memcmp-checks every recovered packet, exit 5), and every stream whose codecs were not the
    ones caught in flight still matches the reference."""
    import hashlib
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    entry = golden_index["batches"]["cfg2_64x4096_p2_ack64"]
    prefix = str(tmp_path / "s")
    env = dict(os.environ, TONK_AMD_SERVE_TIMEOUT_US="1")
    out = subprocess.run([exe, "transcripts", prefix, "threads=8", "streams=16", "stream=0"] + entry["args"],
                         capture_output=True, timeout=600, env=env)
    err = out.stderr.decode()
    assert out.returncode == 0, err[-2000:]
    assert "persistent executor is off" in err, err[-2000:]
    good = 0
    for s in range(16):
        text = open(f"{prefix}{s}.txt", "rb").read()
        if hashlib.sha256(text).hexdigest() == entry["streams"][str(s)]["sha256"]:
            good += 1
        else:  # a stream caught with a command in flight: disabled, never wrong bytes
            assert re.search(rb"^[A-Z] 5\b", text, re.M), text[-400:]
    assert good >= 8, f"only {good} of 16 streams match the reference after the server died"


@pytest.mark.parametrize("name", ["wrap_p1_ack256_1300B", "wrap_p1_full_1300B"])
def test_session_past_column_wrap(golden_index, name):
    """4.3 M originals of 1300 bytes, past the 22-bit packet-number period (SiameseCommon.h:102):
    windows, Siamese sums, Cauchy rows and LDPC pairs straddle column 0x3FFFFF -> 0 on the
    device.  wrap_p1_ack256: the reference decoder disables itself after the wrap; wrap_p1_full:
    no acks, the window fills ~360 times and recoveries continue across the wrap.  Every
    recovery packet and recovered payload (digested on the device), ack and statistic: the
    transcript's digest equals the reference codec's."""
    e = golden_index["long"][name]
    got, summ = _session_transcript(golden_index, name, step=4096)
    assert sha256(got + e["summary"] + "\n") == e["sha256"], got.splitlines()[-1]
    assert summ["disabled_codecs"] == (1 if "ack256" in name else 0)


@pytest.mark.parametrize("name", ["wrap_p1_ack256_1300B", "wrap_p1_full_1300B"])
def test_capi_past_column_wrap(golden_index, name):
    """The same 4.3 M-original streams through the siamese.h C ABI (the reference's own driver
    relinked against libtonk_amd.so): transcript digest == the reference codec's."""
    e = golden_index["long"][name]
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    sid = e["stream"]
    out = subprocess.run([exe, "transcript", "/dev/stdout"] + e["args"] + [f"seed_data={1000 + sid}", f"seed_loss={2000 + sid}"],
                         capture_output=True, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    text = out.stdout.decode()
    assert text.splitlines()[-1] == e["summary"]
    assert sha256(text) == e["sha256"]


def test_capi_ring_passes_a_stalled_post(golden_index, tmp_path):
    """The executor's ring hands slots on out of order: a poster descheduled between taking its
    ticket and writing its descriptor (test hook: command 100's poster sleeps 300 ms) holds up
    only its own command.  Eight threads of codecs keep completing commands behind it, and
    every stream's transcript still equals the reference codec's."""
    import hashlib
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    entry = golden_index["batches"]["cfg2_64x4096_p2_ack64"]
    prefix = str(tmp_path / "s")
    env = dict(os.environ, TONK_AMD_SERVE_STALL_POST_MS="300")
    out = subprocess.run([exe, "transcripts", prefix, "threads=8", "streams=16", "stream=0"] + entry["args"],
                         capture_output=True, timeout=600, env=env)
    err = out.stderr.decode()
    assert out.returncode == 0, err[-2000:]
    m = re.search(r"(\d+) commands completed behind the stalled post", err)
    assert m and int(m.group(1)) > 0, err[-2000:]
    bad = [s for s in range(16)
           if hashlib.sha256(open(f"{prefix}{s}.txt", "rb").read()).hexdigest() != entry["streams"][str(s)]["sha256"]]
    assert not bad, f"streams differing from the reference: {bad}"


IMPAIRED = ["imp_near", "imp_far", "imp_recfirst", "imp_var_dup", "imp_acks", "imp_burst_arq", "imp_rtx", "imp_all",
            "imp_clip"]


@pytest.mark.parametrize("name", IMPAIRED)
def test_capi_impaired_matches_reference(name):
    """The siamese.h C ABI under the impaired channel (oracle/impaired.h: originals and recovery
    packets late and twice, acknowledgements dropped, stale and repeated): `capi_gen impaired`
    writes the reference codec's transcript (tests/golden/impaired.json), bit for bit."""
    import json
    exe = os.path.join(NATIVE, "_build", "capi_gen")
    assert os.path.exists(exe), "build tests/native first (make -C tests/native)"
    with open(os.path.join(ROOT, "tests", "golden", "impaired.json")) as f:
        sc = json.load(f)["scenarios"][name]
    out = subprocess.run([exe, "impaired", "/dev/stdout"] + sc["args"] + ["seed_data=1000", "seed_loss=2000"],
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = out.stdout.decode()
    want = golden_text(name)
    assert sha256(want) == sc["sha256"]
    assert got == want, first_diff(want, got)
