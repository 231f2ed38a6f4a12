# Test-only: the placement kernel's byte logic (tonk_amd/csrc/lz_place.h) and the pass planner
# (tonk_amd/csrc/lz_pass.h) of the stateful batched compressor as a stand-alone host program
# (tests/test_cbatch.py); the second target is the same program under the address and
# undefined-behaviour sanitizers (their runtimes linked in), run on its own.
#   make -C tests/native -f cbatch.mk
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/tonk_amd/csrc
CXXFLAGS := -std=c++14 -O2 -g -Wall -Wextra -march=x86-64-v3
DEPS := cbatch_check.cpp $(CSRC)/lz_place.h $(CSRC)/lz_pass.h $(CSRC)/lz.h $(CSRC)/frame.h

all: _build/cbatch_check _build/cbatch_check_san

_build/cbatch_check: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -o $@ cbatch_check.cpp

_build/cbatch_check_san: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -O1 -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ cbatch_check.cpp

_build:
	mkdir -p _build

.PHONY: all
