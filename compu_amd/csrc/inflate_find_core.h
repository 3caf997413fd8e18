#pragma once
// The block finder's candidate rule (include/compu_hip.h, "one large stream: block starts"), one text for the host form and the
// kernel: does a dynamic-Huffman block header that inflate_unit.h's header path accepts start at bit p of in[0 .. len)?  Nothing is
// decoded and no table is built: the header's code lengths are counted per length as they are read, which is all that zlib's
// acceptance rules (inflate_table: over-subscribed, incomplete) look at.
#include <stdint.h>

#ifdef __HIPCC__
#define FIND_FN __host__ __device__ inline
#define FIND_BIG __host__ __device__ inline __attribute__((noinline))
#else
#define FIND_FN inline
#define FIND_BIG inline __attribute__((noinline))
#endif

namespace chip {
namespace find {

// the 25 stream bits from bit p on (first bit in bit 0); bytes at or behind `len` read as zero
FIND_FN uint32_t peek(const uint8_t *in, uint64_t len, uint64_t p)
{
    const uint64_t b = p >> 3;
    uint32_t v = 0;
    if (b + 4 <= len) v = (uint32_t)in[b] | ((uint32_t)in[b + 1] << 8) | ((uint32_t)in[b + 2] << 16) | ((uint32_t)in[b + 3] << 24);
    else
        for (uint32_t k = 0; k < 4 && b + k < len; k++) v |= (uint32_t)in[b + k] << (8 * k);
    return v >> (p & 7);
}

// the 57 stream bits from bit p on, in one round of loads (the code-length code's 19 x 3 bits)
FIND_FN uint64_t peek57(const uint8_t *in, uint64_t len, uint64_t p)
{
    const uint64_t b = p >> 3;
    uint8_t x[9];
    if (b + 9 <= len) {
        for (uint32_t k = 0; k < 9; k++) x[k] = in[b + k];
    } else {
        for (uint32_t k = 0; k < 9; k++) x[k] = b + k < len ? in[b + k] : (uint8_t)0;
    }
    uint64_t lo = 0;
    for (uint32_t k = 0; k < 8; k++) lo |= (uint64_t)x[k] << (8 * k);
    const uint32_t s = (uint32_t)(p & 7);
    return s ? (lo >> s) | ((uint64_t)x[8] << (64 - s)) : lo;
}

// The 13-bit pre-filter on h = the stream bits from p on: BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29.  1 / 8 * (30 / 32)^2 = 11 %
// of random positions pass.
FIND_FN bool prefilter(uint32_t h) { return (h & 7u) == 4u && ((h >> 3) & 31u) <= 29u && ((h >> 8) & 31u) <= 29u; }

// zlib's verdict on a set of code lengths from its counts per length (count[0] is not looked at): false when the set is
// over-subscribed, or incomplete and not the one allowed incomplete set (a single length-1 code; never allowed for the code-length
// alphabet).  A set without any code passes here; the callers say what that means for their alphabet.
FIND_FN bool set_ok(const uint16_t *count, uint32_t maxbits, bool code_lengths)
{
    int32_t left = 1;
    uint32_t maxlen = 0;
    for (uint32_t l = 1; l <= maxbits; l++) {
        left = (left << 1) - (int32_t)count[l];
        if (left < 0) return false;
        if (count[l]) maxlen = l;
    }
    if (maxlen == 0) return true;
    return !(left > 0 && (code_lengths || maxlen != 1));
}

// Is bit p a candidate?  (p + 17 <= 8 len is the caller's to know: the three block bits and HLIT, HDIST, HCLEN lie in the buffer.)
FIND_BIG bool header_ok(const uint8_t *in, uint64_t len, uint64_t p)
{
    const uint64_t end = len * 8;
    if (p + 17 > end) return false;
    const uint32_t h = peek(in, len, p);
    if (!prefilter(h)) return false;
    const uint32_t nlen = ((h >> 3) & 31u) + 257u, ndist = ((h >> 8) & 31u) + 1u, ncode = ((h >> 13) & 15u) + 4u;
    uint64_t q = p + 17;
    if (q + 3 * ncode > end) return false;
    // the code-length alphabet: complete, or the header path stops (a set of only zeros reads on, and ends at lens[256] == 0)
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    uint16_t cc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t s = 0; s < 19; s++) cl[s] = 0;
    uint32_t kraft = 0;
    const uint64_t bits3 = peek57(in, len, q);
    for (uint32_t k = 0; k < ncode; k++) {  // (in registers: nearly every position that came this far ends here)
        const uint32_t l = (uint32_t)(bits3 >> (3 * k)) & 7u;
        if (l) kraft += 128u >> l;
    }
    if (kraft != 128u) return false;  // (exactly 1: neither over-subscribed nor incomplete)
    for (uint32_t k = 0; k < ncode; k++) {
        const uint32_t l = (uint32_t)(bits3 >> (3 * k)) & 7u;
        cl[order[k]] = (uint8_t)l;
        cc[l]++;
    }
    q += 3 * ncode;
    uint8_t sorted[19];               // the symbols in canonical order
    {
        uint32_t at[8], a = 0;
        for (uint32_t l = 1; l < 8; l++) at[l] = a, a += cc[l];
        for (uint32_t s = 0; s < 19; s++)
            if (cl[s]) sorted[at[cl[s]]++] = (uint8_t)s;
    }
    // the code lengths of the two alphabets by zlib's rules, counted per length
    uint16_t lc[16], dc[16];
    for (uint32_t l = 0; l < 16; l++) lc[l] = dc[l] = 0;
    const uint32_t total = nlen + ndist;
    uint32_t have = 0, prev = 0, l256 = 0;
    while (have < total) {
        const uint32_t x = peek(in, len, q);
        // canonical decode, a bit at a time: the code is complete, so a symbol is found within 7 bits
        uint32_t code = 0, first = 0, index = 0, n = 0, sym = 0;
        for (uint32_t l = 1; l < 8; l++) {
            code |= (x >> (l - 1)) & 1u;
            const uint32_t c = cc[l];
            if (code < first + c) {
                sym = sorted[index + (code - first)];
                n = l;
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (n == 0) return false;  // (cannot be)
        const uint32_t eb = sym < 16 ? 0u : sym == 16 ? 2u : sym == 17 ? 3u : 7u;
        if (q + n + eb > end) return false;  // the header runs out of the buffer
        const uint32_t xv = (x >> n) & ((1u << eb) - 1u);
        uint32_t run = 1, v = sym;
        if (sym == 16) {
            if (have == 0) return false;
            run = 3 + xv, v = prev;
        } else if (sym >= 17) {
            run = (sym == 17 ? 3u : 11u) + xv, v = 0;
        }
        if (have + run > total) return false;
        const uint32_t in_lit = have < nlen ? (nlen - have < run ? nlen - have : run) : 0u;
        lc[v] += (uint16_t)in_lit;
        dc[v] += (uint16_t)(run - in_lit);
        if (have <= 256 && 256 < have + run) l256 = v;
        have += run;
        prev = v;
        q += n + eb;
    }
    if (l256 == 0) return false;  // no end-of-block code
    return set_ok(lc, 15, false) && set_ok(dc, 15, false);
}

// chunk k's range of bit positions that may be its start: [lo, hi), empty when lo >= hi
FIND_FN void chunk_range(uint64_t len, uint64_t first_bit, uint32_t chunk_bytes, uint64_t k, uint64_t &lo, uint64_t &hi)
{
    lo = 8 * k * chunk_bytes;
    hi = lo + 8ull * chunk_bytes;
    if (lo <= first_bit) lo = first_bit + 1;
    const uint64_t last = len * 8 >= 17 ? len * 8 - 17 : 0;  // the last position whose 17 header bits lie in the buffer
    if (len * 8 < 17) hi = 0;
    else if (hi > last + 1) hi = last + 1;
}

}  // namespace find
}  // namespace chip
