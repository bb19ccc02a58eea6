# The transfer-callback queue (libplacebo_amd/csrc/host/cbq.h) under AddressSanitizer + UBSan, on
# the CPU: tests/c/cbq_sanitize.c is a program of its own around the header, with a clock in place
# of the device. Pure host code; nothing of the library is linked.
#     make -f tests/c/cbq_sanitize.mk          # builds and runs it
# The output lands in tests/c/build/ (git-ignored). Not built by build();
# tests/test_callback_queue.py builds the same file without the sanitizers.
HERE := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)/../..)
HOST := $(ROOT)/libplacebo_amd/csrc/host
CFLAGS := -std=c11 -O1 -g -D_GNU_SOURCE -Wall -Wextra -fno-omit-frame-pointer \
          -fsanitize=address,undefined -fno-sanitize-recover=undefined

run: $(HERE)/build/cbq_sanitize
	$<

$(HERE)/build/cbq_sanitize: $(HERE)/cbq_sanitize.c $(HOST)/cbq.h
	mkdir -p $(HERE)/build
	gcc $(CFLAGS) -I$(HOST) $< -o $@

.PHONY: run
