# The PQ EOTF's piece position, one product against two, over every bit pattern of a float:
# tests/c/eotf_pos_exhaustive.hip compiles the header the kernels compile
# (libplacebo_amd/csrc/hip/pqseg.hiph) with the library's flags. Needs a GPU to run (under a
# second); the output lands in tests/c/build/ (git-ignored). tests/test_gpu_eotf_pos_exhaustive.py
# builds and runs it; profiles/chain_row_phase.md has a run.
HERE  := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT  := $(abspath $(HERE)/../..)
HDR   := $(ROOT)/libplacebo_amd/csrc/hip
HIPCC ?= hipcc
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-function

$(HERE)/build/eotf_pos_exhaustive: $(HERE)/eotf_pos_exhaustive.hip $(HDR)/pqseg.hiph $(HDR)/pqmath.hiph $(HDR)/devmath.hiph
	mkdir -p $(HERE)/build
	$(HIPCC) $(HIPFLAGS) -I$(HDR) -I$(ROOT)/include $< -o $@
