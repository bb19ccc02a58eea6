/*
 * libplacebo-hip -- the page rounding of a host pointer import (pl_buf_create with
 * PL_HANDLE_HOST_PTR), after the reference's src/gpu.c:559-588. Pure arithmetic on addresses,
 * nothing is dereferenced: a header of its own so that a program without the library can call it.
 */
#ifndef PLH_HOST_PTR_H_
#define PLH_HOST_PTR_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

// The shared region `ptr` .. `ptr + size` widened to multiples of `align` (a power of two).
// *out_base = `ptr` rounded down, *out_offset = `offset` counted from there, *out_size = the
// region's size from there, rounded up. true = rounding was needed.
static inline bool plh_host_ptr_round(const void *ptr, size_t offset, size_t size, size_t align,
                                      void **out_base, size_t *out_offset, size_t *out_size)
{
    const uintptr_t mask = ~((uintptr_t) align - 1);
    const uintptr_t base = (uintptr_t) ptr & mask;
    const size_t ptr_offset = (uintptr_t) ptr - base;
    const size_t ptr_size = (ptr_offset + size + align - 1) & ~(align - 1);
    *out_base = (void *) base;
    *out_offset = ptr_offset + offset;
    *out_size = ptr_size;
    return base != (uintptr_t) ptr || ptr_size > size;
}

#endif // PLH_HOST_PTR_H_
