/*
 * libplacebo-hip -- the arithmetic of the emulated texture formats (bgra8, rgb10a2, bgr10a2):
 * the only place it exists. Plain C, `static inline`, integer only: the transfer kernels
 * (k_texel.hip), the host test hook (gpu_hip.c: plh_test_texel_convert) and the stand-alone check
 * (tests/c/texel_roundtrip.c) all compile this file.
 *
 * Host layout (the reference's, include/libplacebo/gpu.h `host_bits` / `sample_order`): a texel
 * is one little-endian 32-bit word; component i takes the next host_bits[i] bits from the LSB and
 * is the shader's component sample_order[i]. Storage layout: an ordered rgba8 texel (bgra8) or an
 * ordered rgba16 texel (the 10-bit formats), i.e. shader component order, which is what every
 * kernel of the library reads and writes.
 *
 *   10 -> 16 bits   s = (c * 131070 + 1023) / 2046  = round(c * 65535 / 1023), never a tie
 *    2 -> 16 bits   s = a * 21845
 *   16 -> 10 bits   c = (s * 2046 + 65535) / 131070 = round(s * 1023 / 65535)
 *   16 ->  2 bits   a = (s * 6 + 65535) / 131070    = round(s * 3 / 65535)
 *
 * Every intermediate is below 2^28. pack(unpack(word)) == word for all 2^32 words; a sampled
 * colour value differs from c / 1023 by at most 0.5 / 65535.
 */
#ifndef PLH_TEXEL_H_
#define PLH_TEXEL_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define PLH_TEXEL_FN static inline __host__ __device__
#else
#define PLH_TEXEL_FN static inline
#endif

enum plh_texel_fmt {
    PLH_TEXEL_NONE = 0,     // not an emulated format
    PLH_TEXEL_BGRA8,
    PLH_TEXEL_RGB10A2,
    PLH_TEXEL_BGR10A2,
};

PLH_TEXEL_FN uint32_t plh_unorm10_to_16(uint32_t c) { return (c * 131070u + 1023u) / 2046u; }
PLH_TEXEL_FN uint32_t plh_unorm2_to_16(uint32_t a)  { return a * 21845u; }
PLH_TEXEL_FN uint32_t plh_unorm16_to_10(uint32_t s) { return (s * 2046u + 65535u) / 131070u; }
PLH_TEXEL_FN uint32_t plh_unorm16_to_2(uint32_t s)  { return (s * 6u + 65535u) / 131070u; }

// bgra8 <-> rgba8: bytes [2, 1, 0, 3]; the permutation is its own inverse
PLH_TEXEL_FN uint32_t plh_texel_swap_rb8(uint32_t w)
{
    return (w & 0xff00ff00u) | ((w >> 16) & 0xffu) | ((w & 0xffu) << 16);
}

// one 10-10-10-2 word -> an rgba16 texel as two dwords: lo = ch0 | ch1 << 16, hi = ch2 | ch3 << 16.
// `bgr`: the word's first field is shader component 2 (bgr10a2) instead of 0 (rgb10a2).
PLH_TEXEL_FN void plh_texel_unpack10(uint32_t w, int bgr, uint32_t *lo, uint32_t *hi)
{
    const uint32_t f0 = plh_unorm10_to_16(w & 1023u), f1 = plh_unorm10_to_16((w >> 10) & 1023u),
                   f2 = plh_unorm10_to_16((w >> 20) & 1023u), a = plh_unorm2_to_16(w >> 30);
    *lo = (bgr ? f2 : f0) | (f1 << 16);
    *hi = (bgr ? f0 : f2) | (a << 16);
}

PLH_TEXEL_FN uint32_t plh_texel_pack10(uint32_t lo, uint32_t hi, int bgr)
{
    const uint32_t c0 = plh_unorm16_to_10(lo & 0xffffu), c1 = plh_unorm16_to_10(lo >> 16),
                   c2 = plh_unorm16_to_10(hi & 0xffffu), a = plh_unorm16_to_2(hi >> 16);
    return (bgr ? c2 : c0) | (c1 << 10) | ((bgr ? c0 : c2) << 20) | (a << 30);
}

#endif // PLH_TEXEL_H_
