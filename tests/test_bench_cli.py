"""bench.py's command line: a plain run measures the headline only, --full adds the side legs,
--dump-outputs writes what the timed path returned (float64 .npy files, the same from run to run)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_writes_float64_npy(tmp_path):
    import bench
    import tonk_amd
    out = tmp_path / "d"
    bench.dump_outputs(str(out), {"a": [1, 2**40 + 1], "b": np.arange(6, dtype=np.uint8).reshape(2, 3)})
    bench.dump_outputs(str(out), {"a": [3]}, rank=2)
    assert sorted(os.listdir(out)) == ["a.npy", "a.rank2.npy", "b.npy"]
    a, b = np.load(out / "a.npy"), np.load(out / "b.npy")
    assert a.dtype == b.dtype == np.float64
    assert a.tolist() == [1.0, float(2**40 + 1)] and b.shape == (2, 3)
    assert set(bench.DUMP_FIELDS) <= set(tonk_amd.SUMMARY_FIELDS)


def test_options_are_there():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, TONK_AMD_HUGEPAGE_HEAP="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout, opt


class StubSession:
    """The session's Python surface without a device: counts originals, never past its stream."""
    made: list = []

    def __init__(self, wp, n_streams, **kw):
        self.wp, self.n_streams, self.orig, self.timing, self.launches = wp, n_streams, 0, False, 0
        StubSession.made.append(self)

    def step(self, k):
        self.orig += k
        assert self.orig <= self.wp.n
        self.launches += self.timing

    def summary(self):
        import tonk_amd
        out = dict.fromkeys(tonk_amd.SUMMARY_FIELDS, 0)
        out.update(originals=self.orig * self.n_streams, payload_bytes=self.orig * self.n_streams * 1300,
                   alg_bytes=self.orig * 3000)
        return out

    def host_ms(self):
        import tonk_amd
        return dict.fromkeys(tonk_amd.Session.HOST_PHASES_FR, self.orig * 1e-6)

    def set_timing(self, on):
        self.timing = bool(on)

    def kernel_ms(self):
        return 0.25 * self.launches, self.launches

    generate = wait = finish = close = lambda self: None
    cpus = lambda self: [1, 2]
    arena = lambda self: (1 << 40, 1 << 30)


@pytest.mark.parametrize("steps,warmup,want", [(20, 5, [25]), (55, 5, [60]), (58, 5, [60, 8]), (200, 5, [60, 60, 60, 40])])
def test_steps_past_one_session(monkeypatch, capsys, steps, warmup, want):
    """A stream's packet numbers wrap after 64 steps, so one session runs at most 60 (warm-up
    included, then as before) and a longer run goes on in fresh sessions, each with its own
    warm-up: every timed step is run and counted (host logic, stub session)."""
    import bench
    import tonk_amd
    StubSession.made = []
    StubSession.HOST_PHASES_FR = tonk_amd.Session.HOST_PHASES_FR
    monkeypatch.setattr(tonk_amd, "Session", StubSession)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    assert bench.main() == 0
    j = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert [s.wp.n // 65536 for s in StubSession.made] == want
    assert all(s.orig == s.wp.n for s in StubSession.made)
    assert j["steps"] == steps and j["config"]["sessions"] == len(want)
    assert j["value"] > 0 and j["checks"]["all_recovered"] is True
    assert j["roofline"]["launches"] == steps * bench.PROGRAMS_PER_STEP and j["cpu_baseline"] is None


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeat(tmp_path):
    """Two plain runs of two timed steps: the line holds the headline's keys and none of the side
    legs, `steps` is what was asked, and the dumped arrays are float64 and equal between the runs."""
    dumps = []
    for i in (0, 1):
        d = tmp_path / f"dump{i}"
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        j = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in j, k
        assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
        assert j["cpu_baseline"] is None and "end_to_end" not in j and j["roofline"]["pmc"] is None
        assert "digests_match" not in j["checks"] and j["checks"]["all_recovered"] is True
        arrays = {n: np.load(d / n) for n in sorted(os.listdir(d))}
        assert set(arrays) == {"summary_timed.npy", "summary_timed_delta.npy", "summary_finished.npy",
                               "record_transcript_sha256.npy"}
        assert all(a.dtype == np.float64 for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        # two timed steps of 65536 originals on each of the 64 streams
        assert arrays["summary_timed_delta.npy"][0] == 2 * 65536 * 64
        assert arrays["record_transcript_sha256.npy"].shape == (64, 32)
        dumps.append(arrays)
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n]), n
