/*
 * The emulated texture formats' arithmetic (libplacebo_amd/csrc/hip/plh_texel.h), checked on the
 * host without the library: this program compiles the header the transfer kernels compile.
 *   - unpack is round(c * 65535 / 1023) resp. a * 21845, pack is the nearest code, for every input
 *   - pack(unpack(word)) == word: every colour code x every alpha code in every field, both
 *     10-bit formats, then a strided walk over all 2^32 words (`full` as the first argument: every
 *     word), and the same for the bgra8 byte permutation
 * Prints "texel_roundtrip: ok" and returns 0, or the first mismatch and 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "plh_texel.h"

static int fail(const char *what, unsigned long a, unsigned long b)
{
    printf("texel_roundtrip: %s: %#lx -> %#lx\n", what, a, b);
    return 1;
}

static int check_word(uint32_t w)
{
    for (int bgr = 0; bgr < 2; bgr++) {
        uint32_t lo, hi;
        plh_texel_unpack10(w, bgr, &lo, &hi);
        const uint32_t back = plh_texel_pack10(lo, hi, bgr);
        if (back != w)
            return fail(bgr ? "bgr10a2 round trip" : "rgb10a2 round trip", w, back);
    }
    const uint32_t s = plh_texel_swap_rb8(w);
    if (plh_texel_swap_rb8(s) != w)
        return fail("bgra8 round trip", w, plh_texel_swap_rb8(s));
    const uint8_t *b = (const uint8_t *) &w, *o = (const uint8_t *) &s;   // (little-endian host)
    if (o[0] != b[2] || o[1] != b[1] || o[2] != b[0] || o[3] != b[3])
        return fail("bgra8 permutation", w, s);
    return 0;
}

int main(int argc, char **argv)
{
    const int full = argc > 1 && !strcmp(argv[1], "full");

    // the four formulas against their definitions in wider arithmetic
    for (uint32_t c = 0; c < 1024; c++) {
        const uint64_t want = ((uint64_t) c * 65535 * 2 + 1023) / (2 * 1023);  // round to nearest
        if (plh_unorm10_to_16(c) != want)
            return fail("10 -> 16", c, plh_unorm10_to_16(c));
        if (((uint64_t) c * 65535 * 2) % (2 * 1023) == 1023)
            return fail("10 -> 16 tie", c, 0);
        if (plh_unorm16_to_10(plh_unorm10_to_16(c)) != c)
            return fail("10 -> 16 -> 10", c, plh_unorm16_to_10(plh_unorm10_to_16(c)));
    }
    for (uint32_t a = 0; a < 4; a++) {
        if (plh_unorm2_to_16(a) != a * 65535 / 3 || plh_unorm16_to_2(plh_unorm2_to_16(a)) != a)
            return fail("2 -> 16 -> 2", a, plh_unorm2_to_16(a));
    }
    for (uint32_t s = 0; s < 65536; s++) {
        const uint64_t c = ((uint64_t) s * 1023 * 2 + 65535) / (2 * 65535);
        const uint64_t a = ((uint64_t) s * 3 * 2 + 65535) / (2 * 65535);
        if (plh_unorm16_to_10(s) != c || c > 1023)
            return fail("16 -> 10", s, plh_unorm16_to_10(s));
        if (plh_unorm16_to_2(s) != a || a > 3)
            return fail("16 -> 2", s, plh_unorm16_to_2(s));
    }

    // every colour code x every alpha code, the code in each field in turn and in all three
    for (uint32_t c = 0; c < 1024; c++) {
        for (uint32_t a = 0; a < 4; a++) {
            const uint32_t o = 1023 - c, words[] = {
                c | a << 30, c << 10 | a << 30, c << 20 | a << 30, c | c << 10 | c << 20 | a << 30,
                c | o << 10 | (c ^ 0x155u) << 20 | a << 30,
            };
            for (size_t i = 0; i < sizeof(words) / sizeof(words[0]); i++) {
                if (check_word(words[i]))
                    return 1;
            }
        }
    }

    // all 2^32 words, or every 65521st (a prime: every field sees all of its values)
    const uint64_t step = full ? 1 : 65521;
    for (uint64_t w = 0; w < (1ull << 32); w += step) {
        if (check_word((uint32_t) w))
            return 1;
    }
    if (check_word(0xffffffffu))
        return 1;

    printf("texel_roundtrip: ok (%s)\n", full ? "all 2^32 words" : "strided");
    return 0;
}
