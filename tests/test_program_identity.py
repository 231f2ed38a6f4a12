"""The device programs the host control plane emits stay byte-identical.

tests/native/prog_digest runs the seeded bench workload through the encoder and decoder with no
device (cp_bench's backend and loop) and folds every stream-program's instrs(), ops(),
op_levels(), acc_bytes() and store_bytes() into an FNV-1a digest.  tests/golden/program_digests.json
holds the tool's output recorded before the Siamese-row emission path was rewritten: host-side
work on that path (ProgramBuilder's dense emitter, the pair draws, the decoder's run cache) must
reproduce every digest, so the device executes exactly what it executed before.

The cases are the smallest shapes that reach every branch of that path; the counts the tool
prints beside the digests show that a case did reach it (grouped DENSE runs, multi-chunk rows,
ADJ words).  The unchunked case (streams=4: dense_split = 0) cannot form groups or chunks by
construction -- a range longer than kDenseGroupWork / 2 packets is never grouped, and nothing is
split -- so it is held to DENSE runs and ADJ words only.
"""
import json
import os
import subprocess

import pytest

from conftest import NATIVE, ROOT, _make

BASE = ["streams=5", "n=16384", "step=4096"]
# name -> (arguments in cp_bench's spelling, child-only environment, reach counts that must be > 0)
CASES = {
    "headline_chunked": (BASE, {}, ("dense_multi_runs", "chunked_rows", "adj_words")),
    "unchunked": (["streams=4", "n=16384", "step=4096"], {}, ("dense_runs", "adj_words")),
    "cfg2": (BASE + ["loss=85899346", "fec=2621"], {}, ("dense_multi_runs", "chunked_rows", "adj_words")),
    "burst_arq": (["streams=2", "n=16384", "step=4096", "ge=1", "gb=56493284", "bg=1073741824", "fec=6554",
                   "ack=256", "arq=2048"], {}, ("dense_runs", "adj_words")),
    "contig0": (BASE + ["contig=0"], {}, ("dense_runs",)),
    "nobatch": (BASE + ["nobatch=1"], {}, ("dense_runs",)),
    # 2^22 + 16384 originals: sum ranges straddle the 22-bit column wrap
    "column_wrap": (["streams=1", "n=4210688", "step=32768", "list=0"], {}, ("dense_runs", "adj_words")),
    "dec_direct0": (BASE, {"TONK_AMD_DEC_DIRECT": "0"}, ("dense_multi_runs", "chunked_rows", "adj_words")),
}


@pytest.fixture(scope="module")
def tool():
    _make(NATIVE, "-f", "prog_digest.mk", "_build/prog_digest")
    return os.path.join(NATIVE, "_build", "prog_digest")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "program_digests.json")) as f:
        return json.load(f)


def run_case(tool, name):
    args, env, _ = CASES[name]
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("TONK_AMD_")}
    child_env.update(env)
    r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=120, env=child_env)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_fixture_covers_the_cases(recorded):
    assert sorted(recorded) == sorted(CASES)
    for name, (args, env, _) in CASES.items():
        assert recorded[name]["args"] == args and recorded[name]["env"] == env


@pytest.mark.parametrize("name", list(CASES))
def test_program_identity(tool, recorded, name):
    got = run_case(tool, name)
    want = recorded[name]["result"]
    for key in CASES[name][2]:  # the case reaches the path at all (in the recording and now)
        assert want[key] > 0 and got[key] > 0, (key, want[key], got[key])
    if "programs" in want:
        assert len(got["programs"]) == len(want["programs"])
        bad = [i for i, (a, b) in enumerate(zip(got["programs"], want["programs"])) if a != b]
        assert not bad, f"{len(bad)} of {len(want['programs'])} programs differ, first (program, stream) index {bad[0]}"
    assert got == want
