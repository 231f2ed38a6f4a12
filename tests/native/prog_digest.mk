# Test-only: digests of the emitted device programs, no device (tests/test_program_identity.py).
#   make -C tests/native -f prog_digest.mk _build/prog_digest
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/tonk_amd/csrc
CXXFLAGS := -std=c++14 -O2 -g -Wall -march=x86-64-v3
SRCS := prog_digest.cpp $(CSRC)/engine.cpp $(CSRC)/encoder.cpp $(CSRC)/decoder.cpp $(CSRC)/gf256.cpp
DEPS := $(wildcard $(CSRC)/*.h) resident_streams.h

_build/prog_digest: $(SRCS) $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -o $@ $(SRCS)

_build:
	mkdir -p _build
