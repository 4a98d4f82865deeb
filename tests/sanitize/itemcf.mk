# ASan + UBSan (host side only) build of the two units the ItemCF entry points live in (nrx_itemcf_similarity, nrx_itemcf_recall_workspace,
# nrx_itemcf_recall) plus a driver of its own that walks their argument-validation paths (itemcf_validation_driver.cpp).  Run by
# tests/test_itemcf.py; no GPU needed (nothing is launched).  Same flags as cand_softmax.mk beside it, an object directory of its own: they may run at the same time.
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC  := $(ROOT)/news_recsys_amd/csrc
OUT   := $(ROOT)/tests/sanitize/_build/itemcf
UNITS := nrx_lib nrx_itemcf
# (the sanitizer flags and -fno-gpu-sanitize stay on one line: the device code is never instrumented)
FLAGS := --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -munsafe-fp-atomics -I$(ROOT)/include -fno-omit-frame-pointer -Wno-unused-function
FLAGS += -fsanitize=address,undefined -fno-sanitize-recover=all -fno-gpu-sanitize
FLAGS += -Xarch_device -O0 -Xarch_device -g0
MAKEFLAGS += -j2
run: $(OUT)/itemcf_driver
	ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $(OUT)/itemcf_driver
$(OUT)/%.o: $(CSRC)/%.hip $(CSRC)/nrx_common.h $(CSRC)/nrx_embed_ring.h $(ROOT)/include/nrx_embed.h
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -c $< -o $@
$(OUT)/itemcf_driver: $(UNITS:%=$(OUT)/%.o) $(ROOT)/tests/sanitize/itemcf_validation_driver.cpp
	$(HIPCC) $(FLAGS) $^ -o $@
.PHONY: run
