# ASan + UBSan (host side only) build of the two units nrx_sparse_adagrad_step lives in plus a driver of its own that walks its argument-validation
# paths (adagrad_validation_driver.cpp).  Run by tests/test_sparse_adagrad.py; no GPU needed (nothing is launched).  Same flags and object directory as
# the Makefile beside it, so the two runs share the objects.
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC  := $(ROOT)/news_recsys_amd/csrc
OUT   := $(ROOT)/tests/sanitize/_build
UNITS := nrx_lib nrx_row_optim
# (the sanitizer flags and -fno-gpu-sanitize stay on one line: the device code is never instrumented)
FLAGS := --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -munsafe-fp-atomics -I$(ROOT)/include -fno-omit-frame-pointer -Wno-unused-function
FLAGS += -fsanitize=address,undefined -fno-sanitize-recover=all -fno-gpu-sanitize
FLAGS += -Xarch_device -O0 -Xarch_device -g0
MAKEFLAGS += -j2
run: $(OUT)/adagrad_driver
	ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $(OUT)/adagrad_driver
$(OUT)/%.o: $(CSRC)/%.hip $(CSRC)/nrx_common.h $(CSRC)/nrx_embed_ring.h $(ROOT)/include/nrx_embed.h
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -c $< -o $@
$(OUT)/adagrad_driver: $(UNITS:%=$(OUT)/%.o) $(ROOT)/tests/sanitize/adagrad_validation_driver.cpp
	$(HIPCC) $(FLAGS) $^ -o $@
.PHONY: run
