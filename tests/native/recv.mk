# Test-only: the byte and state logic of the receive front (tonk_amd/csrc/recv.h) as a serial host
# walk (tests/test_recv.py); the second target is the same program under the address and
# undefined-behaviour sanitizers (their runtimes linked in), run on its own.
#   make -C tests/native -f recv.mk
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/tonk_amd/csrc
CXXFLAGS := -std=c++14 -O2 -g -Wall -Wextra -march=x86-64-v3
DEPS := recv_check.cpp $(CSRC)/recv.h $(CSRC)/seal.h $(CSRC)/frame.h $(CSRC)/kernel_abi.h $(CSRC)/program.h $(CSRC)/serve.h

all: _build/recv_check _build/recv_check_san

_build/recv_check: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -o $@ recv_check.cpp

_build/recv_check_san: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -O1 -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ recv_check.cpp

_build:
	mkdir -p _build

.PHONY: all
