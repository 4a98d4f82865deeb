# ASan + UBSan (host side only) build of the two units the pairwise dot-product interaction lives in (nrx_dot_interact_fwd,
# nrx_dot_interact_bwd) plus a driver of its own that walks their argument-validation paths (dot_interact_validation_driver.cpp).  Run by
# tests/test_dot_interact_cpu.py; no GPU needed (nothing is launched).  Same flags as itemcf.mk beside it, an object directory of its own: they may run at the same time.
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC  := $(ROOT)/news_recsys_amd/csrc
OUT   := $(ROOT)/tests/sanitize/_build/dot_interact
UNITS := nrx_lib nrx_dot_interact
# (the sanitizer flags and -fno-gpu-sanitize stay on one line: the device code is never instrumented)
FLAGS := --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -munsafe-fp-atomics -I$(ROOT)/include -fno-omit-frame-pointer -Wno-unused-function
FLAGS += -fsanitize=address,undefined -fno-sanitize-recover=all -fno-gpu-sanitize
FLAGS += -Xarch_device -O0 -Xarch_device -g0
MAKEFLAGS += -j2
run: $(OUT)/dot_interact_driver
	ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $(OUT)/dot_interact_driver
$(OUT)/%.o: $(CSRC)/%.hip $(CSRC)/nrx_common.h $(CSRC)/nrx_embed_ring.h $(ROOT)/include/nrx_embed.h
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -c $< -o $@
$(OUT)/dot_interact_driver: $(UNITS:%=$(OUT)/%.o) $(ROOT)/tests/sanitize/dot_interact_validation_driver.cpp
	$(HIPCC) $(FLAGS) $^ -o $@
.PHONY: run
