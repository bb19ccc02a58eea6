# The colour map's square root against the compiler's, over every non-negative float:
# tests/c/sqrt_exhaustive.hip compiles the header the kernels compile
# (libplacebo_amd/csrc/hip/devmath.hiph) with the library's flags. Needs a GPU to run (a second or
# two); the output lands in tests/c/build/ (git-ignored). profiles/chain_taken_path.md has a run.
HERE  := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT  := $(abspath $(HERE)/../..)
HDR   := $(ROOT)/libplacebo_amd/csrc/hip
HIPCC ?= hipcc
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-function

$(HERE)/build/sqrt_exhaustive: $(HERE)/sqrt_exhaustive.hip $(HDR)/devmath.hiph
	mkdir -p $(HERE)/build
	$(HIPCC) $(HIPFLAGS) -I$(HDR) -I$(ROOT)/include $< -o $@
