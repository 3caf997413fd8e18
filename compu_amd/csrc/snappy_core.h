// Snappy on the host and on the device (include/compu_hip.h, "Snappy: blocks and framed streams"): the preamble varint, the parse of
// one element, the hop over a framed stream's chunk headers and CRC-32C -- one statement of each rule, which the kernels of
// snappy_unit.h, the walk of snappy_chunks.hip and the host decoder below all run -- and the host block decoder.  Plain C++ where no
// HIP compiler is at work: tests/cpp/test_snappy_core.cpp includes this file with g++ alone.  Bytes are read through a reader R:
// `uint32_t byte(uint64_t pos)` and `uint64_t head(uint64_t pos)`, the five bytes from pos on, little-endian, in the low 40 bits
// (those behind the reader's end are unspecified: parse_element looks at none it has not counted) -- host memory, device memory, or
// the kernel's staged LDS window, where head() is one round trip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/compu_hip.h"

#if defined(__HIPCC__)
#define SNAPPY_HD __host__ __device__
#else
#define SNAPPY_HD
#endif

namespace chip {
namespace snappy {

constexpr int32_t OK = 0x7fffffff;          // preamble, parse_element, stream_start: accepted;  chunk_header: a data chunk
constexpr int32_t CHUNK_SKIP = 0x7ffffffe;  // chunk_header: a chunk that is stepped over
constexpr uint64_t NO_LIMIT = ~0ull;
constexpr uint32_t CHUNK_MAX = 65536;       // bytes of content a chunk of the framing format may hold
constexpr uint32_t CRC32C_POLY = 0x82F63B78u;

struct MemReader {
    const uint8_t *p;
    uint64_t len;  // head() reads no byte at or behind it
    SNAPPY_HD uint32_t byte(uint64_t pos) const { return p[pos]; }
    SNAPPY_HD uint64_t head(uint64_t pos) const
    {
        uint64_t v = 0;
        for (uint32_t k = 0; k < 5 && pos + k < len; k++) v |= (uint64_t)p[pos + k] << (8 * k);
        return v;
    }
};

template <class R>
SNAPPY_HD inline uint32_t le32(R &rd, uint64_t pos)
{
    return rd.byte(pos) | (rd.byte(pos + 1) << 8) | (rd.byte(pos + 2) << 16) | (rd.byte(pos + 3) << 24);
}

// ---- CRC-32C ----------------------------------------------------------------------------------------------------------------------
SNAPPY_HD inline uint32_t crc32c_byte(uint32_t c, uint32_t b)
{
    c ^= b;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? CRC32C_POLY : 0u);
    return c;
}

// CRC-32C of n bytes at pos, one byte after the other (the kernels use wave_crc32c of snappy_unit.h)
template <class R>
SNAPPY_HD inline uint32_t crc32c(R &rd, uint64_t pos, uint64_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t k = 0; k < n; k++) c = crc32c_byte(c, rd.byte(pos + k));
    return ~c;
}

// what a data chunk stores
SNAPPY_HD inline uint32_t mask(uint32_t x) { return ((x >> 15) | (x << 17)) + 0xa282ead8u; }

// ---- a block: the preamble and one element ----------------------------------------------------------------------------------------
// The varint at p of a block that ends at `end`: OK (p behind it, n the stated length), CHIP_NEED_INPUT or CHIP_SNAPPY_E_PREAMBLE.
template <class R>
SNAPPY_HD inline int32_t preamble(R &rd, uint32_t end, uint32_t &p, uint64_t &n)
{
    n = 0;
    for (uint32_t i = 0; i < 5; i++) {
        if (p == end) return CHIP_NEED_INPUT;
        const uint32_t b = rd.byte(p++);
        if (i == 4 && b >= 16) return CHIP_SNAPPY_E_PREAMBLE;
        n |= (uint64_t)(b & 0x7fu) << (7 * i);
        if (!(b & 0x80u)) break;
    }
    return OK;
}

struct Elem {
    uint64_t n;    // bytes it produces
    uint32_t src;  // a literal: the position of its first byte in the input
    uint32_t off;  // a copy: its offset
    bool lit;
};

// The element whose tag sits at p, of a block that ends at `end` (both positions of the reader), has produced o bytes and states n.
// Answers OK (p moved behind the element), CHIP_FINISHED / CHIP_NEED_INPUT at the block's end, or the status that stops the block,
// with p still at the tag.
template <class R>
SNAPPY_HD inline int32_t parse_element(R &rd, uint32_t end, uint32_t &p, uint64_t o, uint64_t n, Elem &e)
{
    e.n = 0;
    e.src = e.off = 0;
    e.lit = false;
    if (p == end) return o == n ? CHIP_FINISHED : CHIP_NEED_INPUT;
    if (o == n) return CHIP_SNAPPY_E_LENGTH;
    const uint64_t h = rd.head(p);
    const uint32_t tag = (uint32_t)h & 0xffu, kind = tag & 3u, b4 = (uint32_t)(h >> 8);
    const uint32_t avail = end - p - 1;  // bytes behind the tag
    if (kind == 0) {
        uint64_t len = tag >> 2;
        uint32_t nb = 0;
        if (len >= 60) {
            nb = (uint32_t)len - 59u;
            if (avail < nb) return CHIP_NEED_INPUT;
            len = b4 & (0xFFFFFFFFu >> (32u - 8u * nb));
        }
        len += 1;
        if (len > avail - nb) return CHIP_NEED_INPUT;
        if (len > n - o) return CHIP_SNAPPY_E_LENGTH;
        e.lit = true;
        e.n = len;
        e.src = p + 1 + nb;
        p += 1 + nb + (uint32_t)len;
        return OK;
    }
    const uint32_t nb = kind == 3 ? 4u : kind;
    if (avail < nb) return CHIP_NEED_INPUT;
    const uint32_t m = kind == 1 ? 4u + ((tag >> 2) & 7u) : (tag >> 2) + 1u;
    const uint32_t off = kind == 1 ? ((tag >> 5) << 8) | (b4 & 0xffu) : kind == 2 ? (b4 & 0xffffu) : b4;
    if (off == 0 || off > o) return CHIP_SNAPPY_E_OFFSET;
    if (m > n - o) return CHIP_SNAPPY_E_LENGTH;
    e.n = m;
    e.off = off;
    p += 1 + nb;
    return OK;
}

// ---- the framing format: the stream identifier and the hop over one chunk header ----------------------------------------------------
SNAPPY_HD inline uint32_t ident_byte(uint32_t k)  // ff 06 00 00 "sNaPpY"
{
    return (uint32_t)((k < 8 ? 0x50614e73000006ffull >> (8 * k) : 0x5970ull >> (8 * (k - 8))) & 0xffu);
}

// the first chunk: OK, CHIP_NEED_INPUT or CHIP_SNAPPY_E_HEADER
template <class R>
SNAPPY_HD inline int32_t stream_start(R &rd, uint64_t len)
{
    if (len < 4) return CHIP_NEED_INPUT;
    for (uint32_t k = 0; k < 10 && k < len; k++)
        if (rd.byte(k) != ident_byte(k)) return CHIP_SNAPPY_E_HEADER;
    return len < 10 ? CHIP_NEED_INPUT : OK;
}

// The chunk whose header sits at q, of a stream of `len` bytes.  OK: a data chunk (type 0 / 1, s >= 4, crc the stored value);
// CHUNK_SKIP: one that is stepped over; both are followed by q += 4 + s.  Else the verdict: CHIP_FINISHED (q == len),
// CHIP_NEED_INPUT, CHIP_SNAPPY_E_HEADER, _CHUNK, _CHUNK_SIZE.
template <class R>
SNAPPY_HD inline int32_t chunk_header(R &rd, uint64_t len, uint64_t q, uint32_t &type, uint32_t &s, uint32_t &crc)
{
    type = s = crc = 0;
    if (q == len) return CHIP_FINISHED;
    if (len - q < 4) return CHIP_NEED_INPUT;
    const uint32_t w = le32(rd, q);
    type = w & 0xffu;
    s = w >> 8;
    if (len - q - 4 < s) return CHIP_NEED_INPUT;
    if (type == 0xff) {
        if (s != 6) return CHIP_SNAPPY_E_HEADER;
        for (uint32_t k = 4; k < 10; k++)
            if (rd.byte(q + k) != ident_byte(k)) return CHIP_SNAPPY_E_HEADER;
        return CHUNK_SKIP;
    }
    if (type >= 0x80) return CHUNK_SKIP;
    if (type >= 2) return CHIP_SNAPPY_E_CHUNK;
    if (s < 4) return CHIP_SNAPPY_E_CHUNK_SIZE;
    crc = le32(rd, q + 4);
    return OK;
}

// ---- the walk over a framed buffer's chunk headers (chip_snappy_chunks[_host]) -----------------------------------------------------
template <class R>
SNAPPY_HD inline chip_snappy_chunks_summary walk_chunks(R &rd, uint64_t len, uint64_t max_chunks, chip_snappy_chunk *chunks)
{
    chip_snappy_chunks_summary r = {0, 0, 0, CHIP_ZPLAN_TRUNCATED, 0};
    const int32_t sv = stream_start(rd, len);
    if (sv != OK) {
        r.status = sv == CHIP_NEED_INPUT ? CHIP_ZPLAN_TRUNCATED : CHIP_ZPLAN_BAD_HEADER;
        return r;
    }
    uint64_t q = 10;
    for (;;) {
        r.in_used = q;
        uint32_t type, s, crc;
        const int32_t v = chunk_header(rd, len, q, type, s, crc);
        if (v == CHIP_FINISHED) return r.status = CHIP_ZPLAN_OK, r;
        if (v == CHIP_NEED_INPUT) return r;  // (TRUNCATED)
        if (v == CHUNK_SKIP) {  // (capped as well: a buffer of empty padding chunks would keep one lane hopping for minutes)
            if (r.n_skipped + 1 > CHIP_ZPLAN_MAX_BLOCKS) return r.status = CHIP_ZPLAN_TOO_LARGE, r;
            r.n_skipped++;
        } else if (v == OK) {
            if (r.n_chunks + 1 > CHIP_ZPLAN_MAX_BLOCKS) return r.status = CHIP_ZPLAN_TOO_LARGE, r;
            if (r.n_chunks < max_chunks) {
                const chip_snappy_chunk c = {q, s, type, crc, 0};
                chunks[r.n_chunks] = c;
            }
            r.n_chunks++;
        } else {
            return r.status = CHIP_ZPLAN_BAD_HEADER, r;
        }
        q += 4 + (uint64_t)s;
    }
}

// ---- the host block decoder: the block rules, and their definition ---------------------------------------------------------------
inline int32_t block_decode_host(const uint8_t *in, uint32_t len, uint8_t *out, uint64_t cap, uint64_t &out_len, uint64_t &in_used)
{
    MemReader rd{in, len};
    uint32_t p = 0;
    uint64_t o = 0, n;
    out_len = in_used = 0;
    int32_t st = preamble(rd, len, p, n);
    if (st != OK) return st;
    if (n > cap) return CHIP_NEED_OUTPUT;
    for (;;) {
        Elem e;
        st = parse_element(rd, len, p, o, n, e);
        if (st != OK) break;
        if (e.lit)
            for (uint64_t i = 0; i < e.n; i++) out[o + i] = in[e.src + i];
        else
            for (uint64_t i = 0; i < e.n; i++) out[o + i] = out[o + i - e.off];
        o += e.n;
    }
    out_len = o;
    in_used = p;
    return st;
}

}  // namespace snappy
}  // namespace chip
