# Test-only: the byte logic of the datagram frames and footers (tonk_amd/csrc/dgram.h) as a serial host
# walk (tests/test_dgram.py); the second target is the same program under the address and
# undefined-behaviour sanitizers (their runtimes linked in), run on its own.
#   make -C tests/native -f dgram.mk
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/tonk_amd/csrc
CXXFLAGS := -std=c++14 -O2 -g -Wall -Wextra -march=x86-64-v3
DEPS := dgram_check.cpp $(CSRC)/dgram.h $(CSRC)/frame.h

all: _build/dgram_check _build/dgram_check_san

_build/dgram_check: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -o $@ dgram_check.cpp

_build/dgram_check_san: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -O1 -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ dgram_check.cpp

_build:
	mkdir -p _build

.PHONY: all
