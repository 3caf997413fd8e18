// Host arithmetic of the parallel decode of one stream (inflate_parallel.hip): check values combined along a
// chain of pieces, and what a slab call does to the caller's cursor.  Plain C++ without a device call, so that a stand-alone program
// can run it under the sanitizers (tests/cpp/test_check_combine.cpp).
#pragma once
#include <stdint.h>

#include "../../include/compu_hip.h"

namespace chip {

// ---- combining check values: zlib's crc32_combine and adler32_combine
constexpr uint32_t CRC_POLY = 0xedb88320u;
inline uint32_t multmodp(uint32_t a, uint32_t b)  // a(x) * b(x) mod P, reflected
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
inline uint32_t x8nmodp(uint64_t n)  // x^(8 n) mod P
{
    struct Squares {
        uint32_t sq[32];  // x^(2^k)
        Squares()
        {
            sq[0] = 1u << 30;
            for (int k = 1; k < 32; k++) sq[k] = multmodp(sq[k - 1], sq[k - 1]);
        }
    };
    static const Squares t;
    const uint32_t *sq = t.sq;
    uint32_t p = 1u << 31;
    for (unsigned k = 3; n; n >>= 1, k++)
        if (n & 1) p = multmodp(sq[k & 31], p);
    return p;
}
inline uint32_t crc32_append(uint32_t crc1, uint32_t crc2, uint64_t len2) { return multmodp(x8nmodp(len2), crc1) ^ crc2; }
inline uint32_t adler32_append(uint32_t a1, uint32_t a2, uint64_t len2)
{
    constexpr uint32_t BASE = 65521;
    const uint32_t rem = (uint32_t)(len2 % BASE);
    uint32_t s1 = a1 & 0xffffu, s2 = (uint32_t)(((uint64_t)rem * s1) % BASE);
    s1 += (a2 & 0xffffu) + BASE - 1;
    s2 += (a1 >> 16) + (a2 >> 16) + BASE - rem;
    if (s1 >= BASE) s1 -= BASE;
    if (s1 >= BASE) s1 -= BASE;
    if (s2 >= (BASE << 1)) s2 -= BASE << 1;
    if (s2 >= BASE) s2 -= BASE;
    return s1 | (s2 << 16);
}


// ---- the cursor of chip_inflate_parallel_next
// the checks of the delivered pieces appended to the cursor's
inline void append_checks(chip_inflate_cursor &cur, const uint32_t *chk, const uint64_t *size, uint32_t n)
{
    for (uint32_t k = 0; k < n; k++) {
        if (cur.wrap == 1) cur.check = adler32_append(cur.check, chk[k], size[k]);
        else if (cur.wrap == 2) cur.check = crc32_append(cur.check, chk[k], size[k]);
    }
}

// out_len more bytes were delivered
inline void cursor_delivered(chip_inflate_cursor &cur, uint64_t out_len)
{
    cur.out_total += out_len;
    cur.hist = cur.out_total < 32768u ? (uint32_t)cur.out_total : 32768u;
}

// the call ends at bit at_bit of its slab -> in_used, the whole bytes in front of the new cursor byte
inline uint64_t cursor_advance(chip_inflate_cursor &cur, uint64_t at_bit)
{
    cur.in_total += at_bit >> 3;
    cur.bit = (uint32_t)(at_bit & 7u);
    return at_bit >> 3;
}

// the trailer's bytes (4 of zlib: Adler-32, big endian; 8 of gzip: CRC-32 and ISIZE, little endian) against the cursor
inline bool trailer_matches(const chip_inflate_cursor &cur, const uint8_t t[8])
{
    const uint32_t be = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
    const uint32_t le = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    if (cur.wrap == 1) return be == cur.check;
    if (cur.wrap == 2) return le == cur.check && isize == (uint32_t)cur.out_total;
    return true;
}

}  // namespace chip
