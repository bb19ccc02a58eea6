# The presentation loop in C (tests/c/swapchain_loop.c) and the readback timing tool
# (tests/c/bench_swapchain.c, profiles/swapchain_readback.md) against include/, built by
# __graft_entry__.build() next to the programs of tests/c/Makefile.
#     make -f tests/c/swapchain.mk
# The output lands in tests/c/build/ (git-ignored). tests/test_swapchain_abi.py compiles the same
# file against the reference's headers where they are present (compile only).
HERE := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)/../..)
LIBDIR := $(ROOT)/libplacebo_amd
CFLAGS := -std=c11 -O1 -D_GNU_SOURCE -Wall -Wextra -Wno-deprecated-declarations
LDFLAGS := -L$(LIBDIR) -l:libplacebo_hip.so -Wl,-rpath,'$$ORIGIN/../../../libplacebo_amd' -lm

all: $(HERE)/build/swapchain_loop $(HERE)/build/bench_swapchain

$(HERE)/build/swapchain_loop: $(HERE)/swapchain_loop.c $(LIBDIR)/libplacebo_hip.so \
        $(ROOT)/include/libplacebo/swapchain.h $(ROOT)/include/libplacebo/hip_swapchain.h
	mkdir -p $(HERE)/build
	gcc $(CFLAGS) -I$(ROOT)/include $< -o $@ $(LDFLAGS)

$(HERE)/build/bench_swapchain: $(HERE)/bench_swapchain.c $(LIBDIR)/libplacebo_hip.so \
        $(ROOT)/include/libplacebo/swapchain.h $(ROOT)/include/libplacebo/hip_swapchain.h
	mkdir -p $(HERE)/build
	gcc $(CFLAGS) -I$(ROOT)/include $< -o $@ $(LDFLAGS) -lpthread

.PHONY: all
