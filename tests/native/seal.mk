# Test-only: the byte logic of the datagram cipher and tag (tonk_amd/csrc/seal.h) as a serial host
# walk (tests/test_seal.py); the second target is the same program under the address and
# undefined-behaviour sanitizers (their runtimes linked in), run on its own.
#   make -C tests/native -f seal.mk
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/tonk_amd/csrc
CXXFLAGS := -std=c++14 -O2 -g -Wall -Wextra -march=x86-64-v3
DEPS := seal_check.cpp $(CSRC)/seal.h $(CSRC)/frame.h

all: _build/seal_check _build/seal_check_san

_build/seal_check: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -o $@ seal_check.cpp

_build/seal_check_san: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -O1 -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ seal_check.cpp

_build:
	mkdir -p _build

.PHONY: all
