#!/bin/bash
# Regenerates tests/golden/recv_kat.txt.gz: the output of tests/native/recv_golden.cpp compiled
# with the reference's StrikeRegister.cpp, Counter.h, SimpleCipher.cpp and thirdparty/t1ha.c (into
# tests/native/_build/, which git ignores).  No test runs this.
set -e
cd "$(dirname "$0")/../.."
REF=/root/reference
mkdir -p tests/native/_build
gcc -O2 -c -o tests/native/_build/t1ha_ref.o "$REF/thirdparty/t1ha.c"
g++ -std=c++14 -O2 -march=x86-64-v3 -I"$REF" -o tests/native/_build/recv_golden tests/native/recv_golden.cpp \
    "$REF/StrikeRegister.cpp" "$REF/SimpleCipher.cpp" tests/native/_build/t1ha_ref.o
tests/native/_build/recv_golden | gzip -9 -n > tests/golden/recv_kat.txt.gz
