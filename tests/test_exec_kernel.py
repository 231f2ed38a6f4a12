"""The program executor against the program interpreter, case by case.

tests/native/exec_check.cpp builds small programs through ProgramBuilder's op API over a seeded
arena image with guard rows, and compares the device arena after a run -- bit for bit, the whole
image -- with oracle_run_program on the same image.  All three instantiations of the executor
(kernels.hip run_item / run_accr) are covered: tamd_exec24 (the default launch path), tamd_exec16
(TONK_AMD_SLICE=1024) and the persistent executor tamd_serve.

CPU tests: every case is well formed (validate_program, the preconditions of program.h) and runs
on the interpreter; every group reaches the executor paths it is there for (the reach record:
span, full, slices, level, cost class, op_pure, run modes and counts -- facts the product
computes, so a change of thresholds or emitters cannot quietly make a case easier); every case is
sensitive to the parameters it exercises (mutations change the interpreter's image);
validate_program refuses a violation of each precondition.

GPU tests: three child processes (launch, launch with 1024-byte slices, serve), each under its
own time limit, results cached and asserted per case.  GF(2^8) results are exact: no tolerance.
"""
from __future__ import annotations

import json
import os
import subprocess

import pytest

from conftest import NATIVE

EXE = os.path.join(NATIVE, "_build", "exec_check")

L_ALL = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1300, 1302, 1535, 1536, 1537, 2047, 2048,
         2049, 3071, 3072, 3073, 9008]
C_ALL = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 19, 20, 21, 24, 25, 63, 64, 65, 127, 128, 129]
LANE3, CAUCHY, CONST, MULTI, DENSE = 1, 2, 3, 4, 5
GROUPS = ["acc_store", "batching", "acc3_storec", "runs", "multi", "dense1", "dense_multi", "shared", "serve_groups",
          "levels", "merged", "fuzz"]


def _exe() -> str:
    if not os.path.exists(EXE):  # (a tree where build() has not run)
        subprocess.run(["make", "-C", NATIVE, "_build/exec_check"], check=True, stdout=subprocess.DEVNULL)
    return EXE


def _lines(text: str) -> list:
    return [json.loads(l) for l in text.splitlines() if l.startswith("{")]


def _cpu(mode: str, slice_bytes: int = 0):
    env = dict(os.environ)
    env.pop("TONK_AMD_SLICE", None)
    env.pop("TONK_AMD_CLASS", None)
    if slice_bytes:
        env["TONK_AMD_SLICE"] = str(slice_bytes)
    r = subprocess.run([_exe(), mode], capture_output=True, text=True, timeout=300, env=env)
    return r.returncode, _lines(r.stdout), r.stderr


try:
    CASES = _cpu("list")[1]
except Exception:  # the CPU tests below report it
    CASES = []
NAMES = [c["name"] for c in CASES]
MULTI_DENSE = {c["name"] for c in CASES if c["multi_dense"]}
ONE_CONTEXT = [c["name"] for c in CASES if c["nctx"] == 1]

_reach_cache: dict = {}


def reach(slice_bytes: int = 0) -> dict:
    if slice_bytes not in _reach_cache:
        rc, rows, err = _cpu("cpu", slice_bytes)
        assert rc == 0, (rows[:3], err[-2000:])
        _reach_cache[slice_bytes] = {r["name"]: r for r in rows}
    return _reach_cache[slice_bytes]


def group(name: str, slice_bytes: int = 0) -> list:
    g = [r for r in reach(slice_bytes).values() if r["group"] == name]
    assert g, name
    return g


def runs_of(cases, mode):
    return [r for c in cases for r in c["runs"] if r["mode"] == mode]


# ------------------------------------------------------------------------------------------ CPU

def test_case_list():
    assert len(NAMES) == len(set(NAMES)) and NAMES
    assert sorted({c["group"] for c in CASES}) == sorted(GROUPS)
    assert sum(c["group"] == "fuzz" for c in CASES) == 64
    assert {c["name"] for c in CASES if c["group"] == "dense_multi"} <= MULTI_DENSE
    assert any(c["nctx"] == 2 for c in CASES)


@pytest.mark.parametrize("slice_bytes", [0, 1024])
def test_every_case_is_well_formed_and_runs(slice_bytes):
    rows = reach(slice_bytes)
    assert sorted(rows) == sorted(NAMES)
    assert all("error" not in r for r in rows.values())
    assert {r["slice"] for r in rows.values()} == {slice_bytes or 1536}
    if slice_bytes:
        # the programs are the same words under both slice sizes: so are the expected images
        assert {n: r["digest"] for n, r in rows.items()} == {n: r["digest"] for n, r in reach(0).items()}


def test_reach_acc_store():
    g = group("acc_store")
    assert sorted(int(c["name"].split("L")[1]) for c in g) == L_ALL
    for c in g:
        L = int(c["name"].split("L")[1])
        # 27 (footer, cap) variants + the mixed-length op; caps from L + F up to several slices more
        assert len(c["ops"]) == 28 and c["stores"] == 28
        assert any(o["full"] < o["span"] for o in c["ops"])
        assert max(o["slices"] for o in c["ops"]) >= 3 + L // 1536
        assert any(o["pure"] == 1 for o in c["ops"]) and any(o["pure"] == 0 for o in c["ops"])
    big = next(c for c in g if c["name"] == "acc_store/L3073")["ops"][-1]
    assert big["full"] == 1600 and big["slices"] >= 3  # FULL, masked and partial slices in one op
    assert next(c for c in group("acc_store", 1024) if c["name"] == "acc_store/L3073")["ops"][-1]["slices"] >= 5


def test_reach_batching():
    g = group("batching")
    cut5 = cut6 = split5 = split6 = 0
    for c in g:
        cut5 |= c["cut5"]
        cut6 |= c["cut6"]
        split5 += c["split5"]
        split6 += c["split6"]
    assert cut5 & 0x1f == 0x1f and cut6 & 0x3f == 0x3f  # an ACCR at every position of a batch of 5 / of 6
    assert split5 >= 3 and split6 >= 3                  # STOREs whose FOOTER lies in the next batch
    assert {o["words"] for c in g if "plain" in c["name"] for o in c["ops"]} >= set(range(3, 17))
    assert any(c["clear"] for c in g)
    # 1300-byte rows: one masked slice of 1536, a FULL and a masked slice of 1024
    assert all(o["full"] == 1300 and o["slices"] == 1 for c in g for o in c["ops"])
    assert all(o["slices"] == 2 for c in group("batching", 1024) for o in c["ops"])


def test_reach_acc3_storec():
    g = group("acc3_storec")
    lanes = runs_of(g, LANE3)
    assert sorted({r["count"] for r in lanes}) == C_ALL
    assert sum(c["acc3"] for c in g) >= 2 * len(C_ALL) and sum(c["storec"] for c in g) >= 6 * len(C_ALL)
    assert all(o["pure"] == 0 for c in g for o in c["ops"])
    assert any(o["slices"] > 1 for c in g for o in c["ops"])
    assert any(o["level"] == 2 for c in g for o in c["ops"])  # the parts read back


def test_reach_runs():
    g = group("runs")
    for mode in (CONST, CAUCHY):
        assert sorted({r["count"] for r in runs_of(g, mode)}) == C_ALL
    assert {r["scale"] for r in runs_of(g, CAUCHY)} >= {0, 2, 255}
    assert any(r["p"] == 1 for r in runs_of(g, CONST)) and any(r["p"] > 1 for r in runs_of(g, CONST))
    assert any(r["stride"] > (r["len"] + 63) // 64 + 30 for c in g for r in c["runs"])
    assert any(o["pure"] == 1 for c in g for o in c["ops"]) and any(o["pure"] == 0 for c in g for o in c["ops"])


def test_reach_multi():
    g = group("multi")
    m = runs_of(g, MULTI)
    assert sorted({r["count"] for r in m}) == C_ALL
    assert {r["targets"] for r in m} == {1, 2, 3}
    # column steps other than 1 (the executor derives a row's column from col0, the step and the row's index)
    for step in (3, 8):
        assert sorted({r["count"] for r in m if r["cstep"] == step}) == C_ALL
    assert all(o["pure"] == 0 for c in g for o in c["ops"])


def test_reach_dense():
    g = group("dense1")
    d = runs_of(g, DENSE)
    assert all(r["p"] < 2 for r in d)
    assert sorted({r["count"] for r in d} & set(C_ALL)) == C_ALL
    assert {r["scale"] for r in d} >= {0, 2, 255}
    assert {0, 1, 2} <= {r["adj"] for r in d}
    gm = group("dense_multi")
    dm = runs_of(gm, DENSE)
    # (a chunk of a split range that only the longest row reaches is a one-target run: p = 0)
    assert {r["p"] for r in dm} == {0, 2, 3} and all(c["multi_dense"] for c in gm)
    assert any(o["pure"] == 2 for c in gm for o in c["ops"])
    assert any(r["adj"] for r in dm)
    split = [c for c in gm if "split" in c["name"]]
    assert split and all(max(o["level"] for o in c["ops"]) == 2 for c in split)
    # one wave per item (below class 0) and, the long ones, shared by a workgroup (class 0)
    assert any(o["pure"] == 2 and o["cls"] > 0 for c in gm for o in c["ops"])
    assert any(o["pure"] == 2 and o["cls"] == 0 for c in gm for o in c["ops"])


def test_reach_shared():
    g = group("shared")
    for c in g:
        assert any(o["cls"] == 0 and o["pure"] for o in c["ops"]), c["name"]
    by = {c["name"].split("/")[1]: c for c in g}
    assert max(o["pure"] for o in by["dense_p2"]["ops"]) == 2 and by["dense_p2"]["stores"] == 2
    assert max(o["pure"] for o in by["dense_p3"]["ops"]) == 2 and by["dense_p3"]["stores"] == 3
    assert by["runs_mixed"]["ops"][0]["slices"] == 2 and by["runs_mixed"]["ops"][0]["full"] < 2000
    assert {r["mode"] for r in by["runs_mixed"]["runs"]} == {CONST, CAUCHY, DENSE}
    assert all(r["count"] % 20 for r in by["runs_mixed"]["runs"])  # no multiple of 4 * the row batch
    # `apart`: one shared item, single-wave items beside it; and a launch of shared items only
    assert sum(o["cls"] == 0 for o in by["apart"]["ops"]) == 1 and len(by["apart"]["ops"]) == 10
    assert all(o["cls"] == 0 for o in by["two_shared_only"]["ops"])
    assert by["acc_list"]["runs"] == [] and by["acc_list"]["ops"][0]["words"] == 63


def test_reach_serve_groups_and_levels():
    g = group("serve_groups")
    assert {n for c in g for n in c["level_items"]} >= {1, 2, 3, 4, 5, 8, 9}
    assert any(c["level_items"] == [2, 1, 3] for c in g)
    assert any(o["pure"] == 1 for c in g for o in c["ops"]) and any(o["pure"] == 0 for c in g for o in c["ops"])
    lv = group("levels")
    assert {max(o["level"] for o in c["ops"]) for c in lv} == {2, 3}
    assert all(max(o["level"] for o in c["ops"]) <= 3 and len(c["ops"]) <= 12 for c in group("fuzz"))
    fz = group("fuzz")
    assert {r["mode"] for c in fz for r in c["runs"]} == {LANE3, CAUCHY, CONST, MULTI, DENSE}
    assert any(c["multi_dense"] for c in fz) and any(c["clear"] for c in fz)
    assert {max(o["level"] for o in c["ops"]) for c in fz} == {1, 2, 3}


def test_every_case_is_sensitive_to_what_it_covers():
    rc, rows, err = _cpu("mutate")
    assert sorted(r["name"] for r in rows) == sorted(NAMES), err[-2000:]
    bad = [(r["name"], r["insensitive"]) for r in rows if not r["ok"]]
    assert not bad and rc == 0, bad
    total = {}
    for r in rows:
        for k, v in r["tried"].items():
            total[k] = total.get(k, 0) + v
    assert all(total[k] > 0 for k in ("store_len", "footer", "coef", "count", "hi", "adj", "rx", "scale")), total


def test_validate_program_rejects_each_violation():
    rc, rows, err = _cpu("reject")
    assert rc == 0 and all(r["ok"] for r in rows), ([r for r in rows if not r["ok"]], err[-2000:])
    rules = {r["rule"] for r in rows if r["rejected"]}
    assert rules >= {"run count >= 1", "run len >= 1", "LANE3 within the column period", "MULTI hi <= count",
                     "ADJ ascending", "ADJ empty entries last", "DENSE ranges nested", "reads inside an allocated row",
                     "run rows inside an allocated row", "stores inside an allocated row",
                     "no read of a row written in the same level"}
    assert [r["rule"] for r in rows if not r["rejected"]] == ["unchanged"]


# ------------------------------------------------------------------------------------------ GPU

MODES = {"launch": ("launch", 0), "launch1024": ("launch", 1024), "serve": ("serve", 0)}
_gpu_cache: dict = {}
_gpu_broken: list = []  # a child ended with a signal, a time-out or a HIP error: no further child starts


def gpu_results(mode: str) -> dict:
    if mode in _gpu_cache:
        return _gpu_cache[mode]
    if _gpu_broken:
        pytest.skip(f"not started: the {_gpu_broken[0]} child ended with a fault")
    arg, slice_bytes = MODES[mode]
    env = dict(os.environ)
    env.pop("TONK_AMD_SLICE", None)
    if slice_bytes:
        env["TONK_AMD_SLICE"] = str(slice_bytes)
    try:
        r = subprocess.run(["timeout", "-k", "10", "120", _exe(), arg], capture_output=True, text=True, timeout=150, env=env)
        rc, out, err = r.returncode, r.stdout, r.stderr
    except subprocess.TimeoutExpired as e:
        rc, out, err = 124, (e.stdout or b"").decode(errors="replace"), (e.stderr or b"").decode(errors="replace")
    res = {"rc": rc, "cases": {x["name"]: x for x in _lines(out)}, "stderr": err[-1500:]}
    if rc not in (0, 1):
        _gpu_broken.append(mode)
    _gpu_cache[mode] = res
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_child_completes(mode):
    res = gpu_results(mode)
    assert res["rc"] in (0, 1), (res["rc"], res["stderr"])
    want = ONE_CONTEXT if mode == "serve" else NAMES
    assert sorted(res["cases"]) == sorted(want)
    declined = {n for n, x in res["cases"].items() if x["state"] == "declined"}
    assert declined == (MULTI_DENSE & set(ONE_CONTEXT) if mode == "serve" else set())


def _gpu_params():
    return [pytest.param(m, n, id=f"{m}-{n}") for m in MODES for n in (ONE_CONTEXT if m == "serve" else NAMES)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,name", _gpu_params())
def test_gpu_case_is_bit_exact(mode, name):
    res = gpu_results(mode)
    x = res["cases"].get(name)
    assert x is not None, f"the {mode} child ended (rc {res['rc']}) before this case: {res['stderr']}"
    if mode == "serve" and name in MULTI_DENSE:
        assert x["state"] == "declined", "Server::build must decline a multi-target DENSE run"
        return
    assert x["state"] == "run", "declined by Server::build"
    assert x["ok"], x
