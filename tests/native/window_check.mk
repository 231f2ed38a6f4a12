# Test-only: the codecs' windows under batched adds against single adds, and the session
# backend's computed input handles, no device (tests/test_window_runs.py).
#   make -C tests/native -f window_check.mk
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/tonk_amd/csrc
CXXFLAGS := -std=c++14 -O2 -g -Wall -march=x86-64-v3
CODEC := $(CSRC)/engine.cpp $(CSRC)/encoder.cpp $(CSRC)/decoder.cpp $(CSRC)/gf256.cpp
DEPS := $(wildcard $(CSRC)/*.h) resident_streams.h

all: _build/window_check _build/handle_check

_build/window_check: window_check.cpp $(CODEC) $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -o $@ window_check.cpp $(CODEC)

_build/handle_check: handle_check.cpp $(CODEC) $(DEPS) | _build
	$(CXX) $(CXXFLAGS) -o $@ handle_check.cpp $(CODEC)

_build:
	mkdir -p _build

.PHONY: all
