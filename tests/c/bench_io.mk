# The frame-loop timing tool (tests/c/bench_io.c: `ptr` transfers against a ring of imported
# buffers), built by __graft_entry__.build() next to the programs of tests/c/Makefile.
#     make -f tests/c/bench_io.mk
# The output lands in tests/c/build/ (git-ignored).
HERE := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)/../..)
LIBDIR := $(ROOT)/libplacebo_amd
CFLAGS := -std=c11 -O1 -D_GNU_SOURCE -Wall -Wno-deprecated-declarations
LDFLAGS := -L$(LIBDIR) -l:libplacebo_hip.so -Wl,-rpath,'$$ORIGIN/../../../libplacebo_amd' -lm -ldl

all: $(HERE)/build/bench_io

$(HERE)/build/bench_io: $(HERE)/bench_io.c $(LIBDIR)/libplacebo_hip.so
	mkdir -p $(HERE)/build
	gcc $(CFLAGS) -I$(ROOT)/include $< -o $@ $(LDFLAGS)

.PHONY: all
