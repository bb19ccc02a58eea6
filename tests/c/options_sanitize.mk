# pl_options under AddressSanitizer + UBSan, on the CPU: tests/c/options_sanitize.c, options.c and
# the pure host files whose tables it walks are compiled with the sanitizers into one program of
# its own; only the preset structs come from the library (which must have been built).
#     make -f tests/c/options_sanitize.mk          # builds and runs it
# The output lands in tests/c/build/ (git-ignored). Not built by build(), not a pytest.
HERE := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)/../..)
LIBDIR := $(ROOT)/libplacebo_amd
HOST := $(LIBDIR)/csrc/host
SRC  := $(HOST)/options.c $(HOST)/log.c $(HOST)/filters.c $(HOST)/tone_mapping.c \
        $(HOST)/gamut_mapping.c $(HOST)/dither.c
CFLAGS := -std=c11 -O1 -g -D_GNU_SOURCE -Wall -Wno-deprecated-declarations -fno-omit-frame-pointer \
          -fsanitize=address,undefined -fno-sanitize-recover=undefined
LDFLAGS := -L$(LIBDIR) -l:libplacebo_hip.so -Wl,-rpath,'$$ORIGIN/../../../libplacebo_amd' -lm -lpthread

run: $(HERE)/build/options_sanitize
	$<

$(HERE)/build/options_sanitize: $(HERE)/options_sanitize.c $(SRC) $(HOST)/options_table.inc $(LIBDIR)/libplacebo_hip.so
	mkdir -p $(HERE)/build
	gcc $(CFLAGS) -I$(ROOT)/include $< $(SRC) -o $@ $(LDFLAGS)

.PHONY: run
