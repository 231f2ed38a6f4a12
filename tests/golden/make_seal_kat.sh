#!/bin/bash
# Regenerates tests/golden/seal_kat.txt.gz: the output of tests/native/seal_golden.cpp compiled
# with the reference's SimpleCipher.cpp and thirdparty/t1ha.c (into tests/native/_build/, which
# git ignores).  No test runs this.
set -e
cd "$(dirname "$0")/../.."
REF=/root/reference
mkdir -p tests/native/_build
gcc -O2 -c -o tests/native/_build/t1ha_ref.o "$REF/thirdparty/t1ha.c"
g++ -std=c++14 -O2 -march=x86-64-v3 -I"$REF" -o tests/native/_build/seal_golden tests/native/seal_golden.cpp \
    "$REF/SimpleCipher.cpp" tests/native/_build/t1ha_ref.o
tests/native/_build/seal_golden | gzip -9 -n > tests/golden/seal_kat.txt.gz
