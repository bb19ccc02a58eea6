"""plh_host_ptr_round (csrc/host/host_ptr.h), the page rounding pl_buf_create applies to an imported
host pointer, through the plh_test_host_ptr_round hook against the reference's arithmetic
(src/gpu.c:559-588) written out again in Python integers. Pure arithmetic on addresses: nothing is
dereferenced, no GPU."""
import ctypes as C

import pytest

import libplacebo_amd as pl

PAGE = 4096
BASE = 0x7f12_3456_7000          # page aligned


def restated(ptr, offset, size, align):
    base = ptr - ptr % align
    ptr_offset = ptr - base
    ptr_size = -(-(ptr_offset + size) // align) * align
    return base, ptr_offset + offset, ptr_size, base != ptr or ptr_size > size


def rounded(ptr, offset, size, align):
    base, off, sz = C.c_void_p(), C.c_size_t(), C.c_size_t()
    r = pl.lib().plh_test_host_ptr_round(ptr, offset, size, align, C.byref(base), C.byref(off),
                                    C.byref(sz))
    return base.value or 0, off.value, sz.value, r


CASES = [
    # (pointer, offset of the buffer, size of the shared memory)
    (BASE, 0, PAGE),                        # aligned, whole pages: nothing to do
    (BASE, 2048, 2 << 20),                  # the reference's own test: aligned block, offset inside
    (BASE, 0, PAGE + 1),                    # one byte over a page
    (BASE, 0, 16 * PAGE + 1),
    (BASE + 24, 0, PAGE),                   # pointer + 24: one page becomes two
    (BASE + 24, 0, PAGE - 24),              # ... ends exactly on the boundary
    (BASE + 24, 100, 3 * PAGE),
    (BASE + 4095, 0, 1),                    # the last byte of a page
    (BASE + 4095, 0, 2),                    # ... and the first of the next
    (BASE + 4095, 7, PAGE + 1),
    (BASE + 24, PAGE - 20, 2 * PAGE),       # the offset crosses a page
    (BASE + 4000, 200, PAGE),               # pointer + offset cross a page
    (BASE, 5 * PAGE + 3, 8 * PAGE),
]


@pytest.mark.parametrize("ptr,offset,size", CASES)
def test_rounding_matches_the_reference_arithmetic(ptr, offset, size):
    want = restated(ptr, offset, size, PAGE)
    got = rounded(ptr, offset, size, PAGE)
    assert got == want, (hex(ptr), offset, size)
    base, off, sz, _ = got
    # what the numbers are for: whole pages that cover the memory, the buffer at the same address
    assert base % PAGE == 0 and sz % PAGE == 0
    assert base <= ptr and base + sz >= ptr + size and base + sz - (ptr + size) < PAGE
    assert base + off == ptr + offset


def test_rounding_flag_and_other_page_sizes():
    assert rounded(BASE, 0, PAGE, PAGE)[3] is False
    assert rounded(BASE, 2048, 2 << 20, PAGE)[3] is False
    assert rounded(BASE + 24, 0, PAGE, PAGE)[3] is True
    assert rounded(BASE, 0, PAGE + 1, PAGE)[3] is True
    for align in (4096, 16384, 65536):
        b = BASE - BASE % align
        for ptr, offset, size in ((b, 0, align), (b + 24, 0, align), (b + align - 1, 3, align + 1)):
            assert rounded(ptr, offset, size, align) == restated(ptr, offset, size, align)
