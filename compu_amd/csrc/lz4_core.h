// LZ4 on the host and on the device (include/compu_hip.h, "LZ4: blocks and frames"): XXH32, the frame header parse, the hop over a
// frame's block headers, the parse of one sequence -- the rules of the block format, which the kernels of lz4_unit.h and the host
// decoder below both run -- and the host block decoder.  Plain C++ where no HIP compiler is at work: tests/cpp/test_lz4_core.cpp
// includes this file with g++ alone.  Bytes are read through a reader R with `uint32_t byte(uint64_t pos)`: host memory, device
// memory, or the kernel's staged LDS window.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/compu_hip.h"

#if defined(__HIPCC__)
#define LZ4_HD __host__ __device__
#else
#define LZ4_HD
#endif

namespace chip {
namespace lz4 {

constexpr uint32_t MAGIC = 0x184D2204u;
constexpr uint32_t XP1 = 2654435761u, XP2 = 2246822519u, XP3 = 3266489917u, XP4 = 668265263u, XP5 = 374761393u;
constexpr int32_t SEQ_OK = 0x7fffffff;   // parse_seq: literals and match accepted
constexpr int32_t HDR_OK = 0x7fffffff;   // frame_header: accepted
constexpr uint64_t NO_LIMIT = ~0ull;

LZ4_HD inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

struct MemReader {
    const uint8_t *p;
    LZ4_HD uint32_t byte(uint64_t pos) const { return p[pos]; }
};

template <class R>
LZ4_HD inline uint32_t le32(R &rd, uint64_t pos)
{
    return rd.byte(pos) | (rd.byte(pos + 1) << 8) | (rd.byte(pos + 2) << 16) | (rd.byte(pos + 3) << 24);
}

// what follows the stripes: `h` is the converged accumulators (or seed + P5) plus the total length, the tail is < 16 bytes
template <class R>
LZ4_HD inline uint32_t xxh32_tail(R &rd, uint64_t pos, uint32_t tail_n, uint32_t h)
{
    uint32_t k = 0;
    for (; k + 4 <= tail_n; k += 4) h = rotl32(h + le32(rd, pos + k) * XP3, 17) * XP4;
    for (; k < tail_n; k++) h = rotl32(h + rd.byte(pos + k) * XP5, 11) * XP1;
    h ^= h >> 15;
    h *= XP2;
    h ^= h >> 13;
    h *= XP3;
    h ^= h >> 16;
    return h;
}

// XXH32 of n bytes at pos, one byte stream front to back
template <class R>
LZ4_HD inline uint32_t xxh32(R &rd, uint64_t pos, uint64_t n, uint32_t seed)
{
    uint32_t h;
    uint64_t k = 0;
    if (n >= 16) {
        uint32_t v[4] = {seed + XP1 + XP2, seed + XP2, seed, seed - XP1};
        for (; k + 16 <= n; k += 16)
            for (uint32_t c = 0; c < 4; c++) v[c] = rotl32(v[c] + le32(rd, pos + k + 4 * c) * XP2, 13) * XP1;
        h = rotl32(v[0], 1) + rotl32(v[1], 7) + rotl32(v[2], 12) + rotl32(v[3], 18);
    } else {
        h = seed + XP5;
    }
    return xxh32_tail(rd, pos + k, (uint32_t)(n - k), h + (uint32_t)n);
}

// ---- the frame header -----------------------------------------------------------------------------------------------------------
struct FrameHeader {
    uint32_t flg = 0, bd = 0, header_bytes = 0, block_max = 0;
    uint64_t content_size = CHIP_LZ4BLOCKS_UNSIZED;
    LZ4_HD bool indep() const { return (flg >> 5) & 1u; }
    LZ4_HD bool block_checksum() const { return (flg >> 4) & 1u; }
    LZ4_HD bool has_size() const { return (flg >> 3) & 1u; }
    LZ4_HD bool content_checksum() const { return (flg >> 2) & 1u; }
};

// HDR_OK, CHIP_NEED_INPUT, CHIP_LZ4_E_HEADER or CHIP_LZ4_E_DICT, in the header's order of checks; `h` is filled with HDR_OK only
template <class R>
LZ4_HD inline int32_t frame_header(R &rd, uint64_t len, FrameHeader &h)
{
    if (len < 7) return CHIP_NEED_INPUT;
    if (le32(rd, 0) != MAGIC) return CHIP_LZ4_E_HEADER;
    const uint32_t flg = rd.byte(4), bd = rd.byte(5);
    if ((flg >> 6) != 1u || (flg & 2u) || (bd & 0x8fu) || ((bd >> 4) & 7u) < 4u) return CHIP_LZ4_E_HEADER;
    const uint32_t hs = 7u + ((flg & 8u) ? 8u : 0u) + ((flg & 1u) ? 4u : 0u);
    if (len < hs) return CHIP_NEED_INPUT;
    if (rd.byte(hs - 1) != ((xxh32(rd, 4, hs - 5u, 0) >> 8) & 0xffu)) return CHIP_LZ4_E_HEADER;
    if (flg & 1u) return CHIP_LZ4_E_DICT;
    h.flg = flg;
    h.bd = bd;
    h.header_bytes = hs;
    h.block_max = 1u << (8u + 2u * ((bd >> 4) & 7u));
    h.content_size = (flg & 8u) ? ((uint64_t)le32(rd, 6) | ((uint64_t)le32(rd, 10) << 32)) : CHIP_LZ4BLOCKS_UNSIZED;
    return HDR_OK;
}

// ---- the hop over a frame's block headers (chip_lz4_blocks[_host]) --------------------------------------------------------------
template <class R>
LZ4_HD inline chip_lz4_blocks_summary walk_blocks(R &rd, uint64_t len, uint64_t max_blocks, chip_lz4_block *blocks)
{
    chip_lz4_blocks_summary r = {0, 0, CHIP_LZ4BLOCKS_UNSIZED, 0, 0, 0, 0, 0, CHIP_ZPLAN_TRUNCATED};
    FrameHeader h;
    const int32_t hv = frame_header(rd, len, h);
    if (hv != HDR_OK) {
        r.status = hv == CHIP_NEED_INPUT ? CHIP_ZPLAN_TRUNCATED : CHIP_ZPLAN_BAD_HEADER;
        return r;
    }
    r.content_size = h.content_size;
    r.block_max = h.block_max;
    r.flg = h.flg;
    r.bd = h.bd;
    r.header_bytes = h.header_bytes;
    const uint32_t extra = h.block_checksum() ? 4u : 0u;
    uint64_t q = h.header_bytes, n = 0;
    for (;;) {
        r.n_blocks = n;
        if (len - q < 4) return r;  // (TRUNCATED)
        const uint32_t w = le32(rd, q);
        if (w == 0) {
            if (n && n <= max_blocks) blocks[n - 1].flags |= CHIP_LZ4BLOCK_LAST;
            q += 4;
            break;
        }
        const uint32_t size = w & 0x7fffffffu;
        if (size > h.block_max) return r.status = CHIP_ZPLAN_BAD_HEADER, r;
        if (n + 1 > CHIP_ZPLAN_MAX_BLOCKS) return r.status = CHIP_ZPLAN_TOO_LARGE, r;
        if (len - q - 4 < (uint64_t)size + extra) return r;
        if (n < max_blocks) {
            chip_lz4_block b = {q, size, (w >> 31) ? (uint32_t)CHIP_LZ4BLOCK_STORED : 0u, extra ? le32(rd, q + 4 + size) : 0u, 0};
            blocks[n] = b;
        }
        n++;
        q += 4 + (uint64_t)size + extra;
    }
    if (h.content_checksum()) {
        if (len - q < 4) return r;
        r.content_checksum = le32(rd, q);
        q += 4;
    }
    r.in_used = q;
    r.status = CHIP_ZPLAN_OK;
    return r;
}

// ---- one sequence of a block ----------------------------------------------------------------------------------------------------
struct Seq {
    uint64_t ll, ml;   // accepted literal run (to be copied and counted whatever the verdict) and match (0: none)
    uint32_t lit_pos;  // of the run's first byte in the input
    uint32_t off;
};

// The sequence whose token sits at p, of a block that ends at `end` (both positions of the reader).  hist: the bytes an offset
// may reach in front of the sequence's first literal.  room: bytes of output left; blk_room: bytes the block may still grow by
// (NO_LIMIT for a lone block), beyond which the verdict is e_size.  Answers SEQ_OK (p moved behind the sequence), CHIP_FINISHED
// (the literal run ended the block, p == end) or the status that stops the block, with p still at the token.
template <class R>
LZ4_HD inline int32_t parse_seq(R &rd, uint32_t end, uint32_t &p, uint64_t hist, uint64_t room, uint64_t blk_room, int32_t e_size, Seq &s)
{
    s.ll = s.ml = 0;
    s.off = s.lit_pos = 0;
    uint32_t q = p;
    if (q >= end) return CHIP_NEED_INPUT;
    const uint32_t token = rd.byte(q++);
    uint64_t ll = token >> 4;
    if (ll == 15) {
        uint32_t b;
        do {
            if (q >= end) return CHIP_NEED_INPUT;
            b = rd.byte(q++);
            ll += b;
        } while (b == 255);
    }
    if (ll > end - q) return CHIP_NEED_INPUT;
    if (ll > blk_room) return e_size;
    if (ll > room) return CHIP_NEED_OUTPUT;
    s.lit_pos = q;
    s.ll = ll;
    q += (uint32_t)ll;
    if (q == end) {
        p = q;
        return CHIP_FINISHED;
    }
    if (end - q < 2) return CHIP_NEED_INPUT;
    const uint32_t off = rd.byte(q) | (rd.byte(q + 1) << 8);
    q += 2;
    if (off == 0 || off > hist + ll) return CHIP_LZ4_E_OFFSET;
    uint64_t ml = token & 15u;
    if (ml == 15) {
        uint32_t b;
        do {
            if (q >= end) return CHIP_NEED_INPUT;
            b = rd.byte(q++);
            ml += b;
        } while (b == 255);
    }
    ml += 4;
    if (blk_room != NO_LIMIT && ml > blk_room - ll) return e_size;
    if (room != NO_LIMIT && ml > room - ll) return CHIP_NEED_OUTPUT;
    s.off = off;
    s.ml = ml;
    p = q;
    return SEQ_OK;
}

// ---- the host block decoder: the block rules, and their definition ---------------------------------------------------------------
inline int32_t block_decode_host(const uint8_t *in, uint32_t len, uint8_t *out, uint64_t cap, uint64_t &out_len, uint64_t &in_used)
{
    MemReader rd{in};
    uint32_t p = 0;
    uint64_t o = 0;
    int32_t st;
    for (;;) {
        Seq s;
        st = parse_seq(rd, len, p, o, cap - o, NO_LIMIT, 0, s);
        for (uint64_t i = 0; i < s.ll; i++) out[o + i] = in[s.lit_pos + i];
        o += s.ll;
        if (st != SEQ_OK) break;
        for (uint64_t i = 0; i < s.ml; i++) out[o + i] = out[o + i - s.off];
        o += s.ml;
    }
    out_len = o;
    in_used = p;
    return st;
}

}  // namespace lz4
}  // namespace chip
