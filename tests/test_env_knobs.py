"""The inventory of the library's environment variables (CPU, source text only).

Every `TONK_AMD_*` name the library reads -- inside a `getenv(...)` of the C++ / HIP sources or an
`os.environ` read of the Python package under tonk_amd/ -- must have a row in the first table of
INTEGRATION.md's "Runtime knobs", and every row there must be read somewhere: a new switch cannot
appear unlisted, and a deleted one cannot stay documented.  The variables bench.py and the tests
read for themselves are in INTEGRATION.md's second table and are not the library's.
"""
from __future__ import annotations

import os
import re

from conftest import ROOT

NAME = r"(TONK_AMD_[A-Z0-9_]+)"
READS = [
    re.compile(r"getenv\(\s*\"" + NAME + r"\""),                        # C++ getenv, os.getenv
    re.compile(r"os\.environ(?:\.get\(|\.pop\(|\[)\s*[\"']" + NAME + r"[\"']"),
    re.compile(r"[\"']" + NAME + r"[\"']\s+(?:not\s+)?in\s+os\.environ"),
]


def names_read() -> set:
    found = set()
    for base, dirs, files in os.walk(os.path.join(ROOT, "tonk_amd")):
        dirs[:] = [d for d in dirs if d not in ("build", "__pycache__")]
        for f in files:
            if not f.endswith((".cpp", ".h", ".hip", ".py")):
                continue
            with open(os.path.join(base, f), encoding="utf-8") as fh:
                text = fh.read()
            for rx in READS:
                found.update(rx.findall(text))
    return found


def names_documented() -> set:
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        lines = fh.read().splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("Runtime knobs"))
    at = next(i for i in range(at, len(lines)) if lines[i].startswith("| variable "))
    rows = []
    for ln in lines[at + 2:]:  # (header and separator skipped; the table ends at the first other line)
        if not ln.startswith("|"):
            break
        rows.append(ln)
    names = [re.match(r"\| `" + NAME + r"` \|", ln) for ln in rows]
    assert all(names), [ln for ln, m in zip(rows, names) if not m]
    out = [m.group(1) for m in names]
    assert len(out) == len(set(out)), "a variable has two rows"
    return set(out)


def test_documented_knobs_are_the_knobs_read():
    read, documented = names_read(), names_documented()
    assert read - documented == set(), "read by the library, no row in INTEGRATION.md"
    assert documented - read == set(), "a row in INTEGRATION.md, read nowhere in the library"
    assert "TONK_AMD_DEVICE" in read and "TONK_AMD_LIB" in read  # (both kinds of read are found)
