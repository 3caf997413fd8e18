// The host arithmetic of the slabbed decode (compu_amd/csrc/check_combine.h) as a stand-alone program, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o test_check_combine test_check_combine.cpp -lz
// It combines the CRC-32 / Adler-32 of pieces along a chain as chip_inflate_parallel_next does, moves a cursor through calls whose
// totals cross 2^32, and compares every step with zlib over the joined bytes (and with zlib's own combine for long lengths).
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <vector>

#include "../../compu_amd/csrc/check_combine.h"

using namespace chip;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            failures++;                                             \
        }                                                           \
    } while (0)

static uint32_t rnd_state = 12345;
static uint32_t rnd()
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

int main()
{
    // pieces of every small length and some long ones, appended one by one
    std::vector<uint8_t> all;
    std::vector<uint64_t> sizes = {0, 1, 2, 3, 0, 255, 256, 5551, 5552, 5553, 65520, 65521, 65522, 100000, 0, 1};
    for (int wrap = 1; wrap <= 2; wrap++) {
        all.clear();
        chip_inflate_cursor cur;
        memset(&cur, 0, sizeof cur);
        cur.wrap = (uint32_t)wrap, cur.phase = CHIP_CUR_BLOCKS, cur.check = wrap == 1 ? 1u : 0u;
        for (uint64_t n : sizes) {
            std::vector<uint8_t> piece(n);
            for (auto &b : piece) b = (uint8_t)rnd();
            const uint32_t own = wrap == 1 ? (uint32_t)adler32(1, piece.data(), (uInt)n) : (uint32_t)crc32(0, piece.data(), (uInt)n);
            append_checks(cur, &own, &n, 1);
            cursor_delivered(cur, n);
            all.insert(all.end(), piece.begin(), piece.end());
            const uint32_t want = wrap == 1 ? (uint32_t)adler32(1, all.data(), (uInt)all.size()) : (uint32_t)crc32(0, all.data(), (uInt)all.size());
            CHECK(cur.check == want);
            CHECK(cur.out_total == all.size());
            CHECK(cur.hist == (all.size() < 32768 ? all.size() : 32768));
        }
        // the trailer as the format writes it
        uint8_t t[8];
        const uint32_t c = cur.check, isize = (uint32_t)cur.out_total;
        if (wrap == 1) t[0] = c >> 24, t[1] = c >> 16, t[2] = c >> 8, t[3] = c, t[4] = t[5] = t[6] = t[7] = 0;
        else t[0] = c, t[1] = c >> 8, t[2] = c >> 16, t[3] = c >> 24, t[4] = isize, t[5] = isize >> 8, t[6] = isize >> 16, t[7] = isize >> 24;
        CHECK(trailer_matches(cur, t));
        t[1] ^= 1;
        CHECK(!trailer_matches(cur, t));
        t[1] ^= 1;
        if (wrap == 2) {
            t[6] ^= 0x80;
            CHECK(!trailer_matches(cur, t));
        }
    }
    // lengths no buffer holds: against zlib's combine
    for (uint64_t len : {1ull << 31, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 70000, 5ull << 30, 1ull << 40}) {
        const uint32_t a = rnd() * 977u, b = rnd() * 131u;
        CHECK(crc32_append(a, b, len) == (uint32_t)crc32_combine64(a, b, (z_off64_t)len));
        const uint32_t a1 = (rnd() % 65521u) << 16 | rnd() % 65521u, a2 = (rnd() % 65521u) << 16 | rnd() % 65521u;
        CHECK(adler32_append(a1, a2, len) == (uint32_t)adler32_combine64(a1, a2, (z_off64_t)len));
    }
    // a cursor through calls that end inside a byte, and totals across 2^32 (gzip's ISIZE is the total mod 2^32)
    {
        chip_inflate_cursor cur;
        memset(&cur, 0, sizeof cur);
        cur.wrap = 2, cur.phase = CHIP_CUR_BLOCKS;
        uint64_t in = 0, out = 0;
        for (int k = 0; k < 1000; k++) {
            const uint64_t at_bit = cur.bit + (uint64_t)(rnd() % (1u << 30)) * 9u, n = (uint64_t)rnd() << 4;
            cursor_delivered(cur, n);
            const uint64_t used = cursor_advance(cur, at_bit);
            CHECK(used == at_bit >> 3 && cur.bit == (at_bit & 7));
            in += used, out += n;
            CHECK(cur.in_total == in && cur.out_total == out && cur.hist == (out < 32768 ? out : 32768));
        }
        CHECK(cur.out_total > 1ull << 32 && cur.in_total > 1ull << 32);
        uint8_t t[8] = {0, 0, 0, 0, (uint8_t)cur.out_total, (uint8_t)(cur.out_total >> 8), (uint8_t)(cur.out_total >> 16), (uint8_t)(cur.out_total >> 24)};
        CHECK(trailer_matches(cur, t));
    }
    printf(failures ? "test result: FAILED (%d)\n" : "test result: ok\n", failures);
    return failures ? 1 : 0;
}
