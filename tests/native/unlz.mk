# Test-only: the block reader of the decompression kernel (tonk_amd/csrc/unlz.h) as a serial host
# walk and on 64 emulated lanes against the reference's zstd (tests/test_decompress.py), with the
# generator of the directed blocks; the second target is the same
# program under the address and undefined-behaviour sanitizers (their runtimes linked in), run on
# its own.
#   make -C tests/native -f unlz.mk
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/tonk_amd/csrc
CXXFLAGS := -std=c++14 -O2 -g -Wall -march=x86-64-v3
REF := -L$(ROOT)/oracle/_ref -lmsgcodec_ref -Wl,-rpath,'$$ORIGIN/../../../oracle/_ref' -lpthread

all: _build/unlz_check _build/unlz_check_san

_build/unlz_check: unlz_check.cpp lz_host.h $(CSRC)/unlz.h $(CSRC)/lz.h $(ROOT)/oracle/_ref/libmsgcodec_ref.so | _build
	$(CXX) $(CXXFLAGS) -o $@ unlz_check.cpp $(REF)

_build/unlz_check_san: unlz_check.cpp lz_host.h $(CSRC)/unlz.h $(CSRC)/lz.h $(ROOT)/oracle/_ref/libmsgcodec_ref.so | _build
	$(CXX) $(CXXFLAGS) -O1 -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ unlz_check.cpp $(REF)

_build:
	mkdir -p _build

.PHONY: all
