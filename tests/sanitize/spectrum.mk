# Sanitizer build of the host geometry of the spectrum meter (csrc/gfdm_spectrum.h: runs of segments, partial rows, plan, origins),
# brute-forced by spectrum_geometry_check.cc -- a stand-alone program with its own main, built the way Makefile builds streamtile_check.cc
# (same compiler, same flags); it needs neither the loop-back HIP layer nor the generated includes, so it has a recipe of its own.
#     make -C tests/sanitize -f spectrum.mk spectrum    AddressSanitizer + UBSan -> build/spectrum_geometry_check_asan
#     make -C tests/sanitize -f spectrum.mk run
# tests/test_spectrum_geometry.py builds and runs it in the `-m "not gpu"` suite.
CXX_SAN ?= /opt/rocm/lib/llvm/bin/clang++
HERE := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
PKG := $(abspath $(HERE)/../../gr-gfdm_amd)
OUT ?= $(HERE)/build

COMMON := -std=c++17 -g -O1 -fno-omit-frame-pointer -ffp-contract=off -Wall -Wno-unused-function -I$(PKG)/csrc
ASAN_FLAGS := -fsanitize=address,undefined,implicit-integer-truncation,implicit-integer-sign-change,float-cast-overflow,nullability -fno-sanitize-recover=all

spectrum: $(OUT)/spectrum_geometry_check_asan

$(OUT)/asan/spectrum_geometry_check.o: $(HERE)/spectrum_geometry_check.cc $(PKG)/csrc/gfdm_spectrum.h
	@mkdir -p $(OUT)/asan
	$(CXX_SAN) $(COMMON) $(ASAN_FLAGS) -c -o $@ $<
$(OUT)/spectrum_geometry_check_asan: $(OUT)/asan/spectrum_geometry_check.o
	$(CXX_SAN) $(ASAN_FLAGS) -o $@ $^

run: spectrum
	ASAN_OPTIONS="detect_leaks=1 detect_stack_use_after_return=1" UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1" $(OUT)/spectrum_geometry_check_asan

.PHONY: spectrum run
