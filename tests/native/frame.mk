# Test-only: the byte logic of the framing kernels (tonk_amd/csrc/frame.h) as a serial host walk
# (tests/test_batch.py); the second target is the same program under the address and
# undefined-behaviour sanitizers (their runtimes linked in), run on its own.
#   make -C tests/native -f frame.mk
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/tonk_amd/csrc
CXXFLAGS := -std=c++14 -O2 -g -Wall -Wextra -march=x86-64-v3
DEPS := frame_check.cpp $(CSRC)/frame.h $(CSRC)/kernel_abi.h $(CSRC)/serial.h

all: _build/frame_check _build/frame_check_san

_build/frame_check: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -o $@ frame_check.cpp

_build/frame_check_san: $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -O1 -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ frame_check.cpp

_build:
	mkdir -p _build

.PHONY: all
