# The timing driver of one polar downscaling pass (tests/c/bench_polar_band.c; figures in
# profiles/polar_band.md). Not part of __graft_entry__.build(): built where it is wanted.
#     make -f tests/c/bench_polar_band.mk
# The output lands in tests/c/build/ (git-ignored).
HERE := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)/../..)
LIBDIR := $(ROOT)/libplacebo_amd
CFLAGS := -std=c11 -O1 -D_GNU_SOURCE -Wall -Wno-deprecated-declarations
LDFLAGS := -L$(LIBDIR) -l:libplacebo_hip.so -Wl,-rpath,'$$ORIGIN/../../../libplacebo_amd' -lm

all: $(HERE)/build/bench_polar_band

$(HERE)/build/bench_polar_band: $(HERE)/bench_polar_band.c $(LIBDIR)/libplacebo_hip.so
	mkdir -p $(HERE)/build
	gcc $(CFLAGS) -I$(ROOT)/include $< -o $@ $(LDFLAGS)

.PHONY: all
