# The emulated texture formats' arithmetic without the library: tests/c/texel_roundtrip.c compiles
# the header the transfer kernels compile (libplacebo_amd/csrc/hip/plh_texel.h). Run by
# tests/test_texel_formats.py (make -f); the output lands in tests/c/build/ (git-ignored).
# SAN="-fsanitize=address,undefined" builds the sanitized program the same way.
HERE := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)/../..)
HDR  := $(ROOT)/libplacebo_amd/csrc/hip
CFLAGS := -std=c11 -O1 -g -D_GNU_SOURCE -Wall $(SAN)

$(HERE)/build/texel_roundtrip: $(HERE)/texel_roundtrip.c $(HDR)/plh_texel.h
	mkdir -p $(HERE)/build
	gcc $(CFLAGS) -I$(HDR) $< -o $@
