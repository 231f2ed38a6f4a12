#!/bin/bash
# Regenerates tests/golden/dgram_kat.txt.gz: the output of tests/native/dgram_golden.cpp compiled
# against the reference's header-only frame and footer primitives (into tests/native/_build/, which
# git ignores).  No test runs this.
set -e
cd "$(dirname "$0")/../.."
REF=/root/reference
mkdir -p tests/native/_build
g++ -std=c++14 -O2 -march=x86-64-v3 -I"$REF" -I"$REF/thirdparty" -o tests/native/_build/dgram_golden tests/native/dgram_golden.cpp
tests/native/_build/dgram_golden | gzip -9 -n > tests/golden/dgram_kat.txt.gz
