# The hand-written declarations of libplacebo_amd/csrc/host/lcms_api.h against the installed
# LittleCMS 2 headers: tests/c/lcms_api_check.c includes both and asserts that every constant,
# size and member offset agrees. Run by tests/test_icc.py (make -f); the output lands in
# tests/c/build/ (git-ignored). The library itself needs no header: where none is found the
# target prints why and builds nothing, and the test is skipped.
# LCMS_INC=<dir> names the directory that holds lcms2.h and lcms2_plugin.h.
HERE := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)/../..)
HDR  := $(ROOT)/libplacebo_amd/csrc/host
CFLAGS := -std=c11 -O1 -g -D_GNU_SOURCE -Wall $(SAN)

PYPREFIX := $(shell python3 -c "import sys; print(sys.prefix)" 2>/dev/null)
CANDIDATES := $(LCMS_INC) $(CONDA_PREFIX)/include $(PYPREFIX)/include /usr/include /usr/local/include \
              /opt/conda/include
FOUND := $(firstword $(foreach d,$(CANDIDATES),$(if $(and $(wildcard $(d)/lcms2.h),$(wildcard $(d)/lcms2_plugin.h)),$(d))))

ifeq ($(FOUND),)
check:
	@echo "lcms_api_check: skipped (no lcms2.h / lcms2_plugin.h in: $(CANDIDATES))"
else
check: $(HERE)/build/lcms_api_check

$(HERE)/build/lcms_api_check: $(HERE)/lcms_api_check.c $(HDR)/lcms_api.h
	mkdir -p $(HERE)/build
	gcc $(CFLAGS) -I$(HDR) -idirafter $(FOUND) $< -o $@
endif

.PHONY: check
