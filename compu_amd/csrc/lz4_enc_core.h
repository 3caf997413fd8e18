// LZ4 encoder (include/compu_hip.h, "LZ4: encoding"): the match finder, the emission of a block and the frame
// around blocks, stated ONCE for the host and the device.  block_encode / frame_encode are templates over a `Lanes` policy:
// HostLanes runs every per-lane step in a loop over the 64 lanes (chip_lz4_block_encode_host, chip_lz4_frame_encode_host: the
// definition of the bytes), the kernel's policy (lz4_enc.hip) runs them on the lanes of a wavefront with an LDS wait between the
// steps.  Plain C++ where no HIP compiler is at work: tests/cpp/test_lz4_enc_core.cpp includes this file with g++ alone.
//
// The match finder is the chunked one of zstd_enc_core.h: 64 positions per chunk, per-lane steps hash -> read candidates ->
// update table -> measure, then a wave-uniform walk over the 64 results.  The rule where several lanes of a chunk share a slot:
// a lane's first candidate is the latest EARLIER lane of the chunk with the same hash, else the table; only the LAST lane of
// each hash writes the slot (a two-way slot keeps the lane before it, else the former first way, as its second way).  Nothing
// depends on the order in which lanes run.
// The table holds the low 16 bits of positions: a slot names the latest position in front of the current one with those bits,
// which reaches 65 536 back; the 4-byte compare rejects aliases and chunk_match rejects the one distance (65 536) LZ4 cannot state.
//
// The duties of the block format that liblz4's decoders rely on:
//   - a match starts at p only with p + 12 <= n, and ends at or before n - 5: the last 5 bytes are literals
//   - a block of fewer than 13 bytes is one literal run; n == 0 is the one byte 0x00
//   - offsets are 1 .. 65 535, and never reach in front of the block (positions are block-relative, the table is cleared per block)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lz4_core.h"
#include "zstd_enc_core.h"

#if defined(__HIPCC__)
#define LE_FN __host__ __device__ inline
#else
#define LE_FN inline
#endif

namespace chip {
namespace lz4enc {

using zenc::Out;

constexpr uint32_t HLOG = 13;  // 8192 entries of 16 bits: one way of 8192 slots or two of 4096
constexpr uint32_t HSIZE = 1u << HLOG;
constexpr uint32_t CHUNK = 64;
constexpr uint32_t NOHASH = 0xffffffffu;
constexpr uint32_t MIN_MATCH = 4, LAST_LITERALS = 5, MF_LIMIT = 12, MAX_OFFSET = 65535;
constexpr uint32_t MAX_UNIT = 0x7E000000u;  // LZ4_MAX_INPUT_SIZE: a larger unit is CHIP_ENC_ERROR
constexpr uint32_t FRAME_HEADER = 15;       // magic, FLG, BD, Content_Size, HC

// level groups: 0 (levels 1-2) greedy, one position per slot, a growing skip; 1 (3-5) greedy, two positions per slot;
// 2 (6-12) two positions per slot and a one-step lazy choice
struct Cfg {
    uint32_t group;
    uint32_t skip_shift;  // group 0: step = 1 + (bytes since the last match >> skip_shift)
};

// level -1 .. 12 (-1 and 0 mean 1); false: out of range
LE_FN bool level_cfg(int level, Cfg &c)
{
    if (level < -1 || level > 12) return false;
    if (level < 1) level = 1;
    c.group = level < 3 ? 0u : level < 6 ? 1u : 2u;
    c.skip_shift = level == 1 ? 6u : 8u;
    return true;
}

// frame options (chip_encode_batch_ex's strategy for CHIP_FMT_LZ4): false = CHIP_E_INVALID
LE_FN bool frame_opts_ok(int strategy)
{
    if (strategy & ~(CHIP_LZ4_S_BLOCK_CHECKSUM | CHIP_LZ4_S_NO_CONTENT_CHECKSUM | CHIP_LZ4_S_BLOCK_ID_MASK)) return false;
    const uint32_t id = ((uint32_t)strategy & CHIP_LZ4_S_BLOCK_ID_MASK) >> CHIP_LZ4_S_BLOCK_ID_SHIFT;
    return id == 0 || (id >= 4 && id <= 7);
}
LE_FN uint32_t opts_block_id(uint32_t opts)
{
    const uint32_t id = (opts & CHIP_LZ4_S_BLOCK_ID_MASK) >> CHIP_LZ4_S_BLOCK_ID_SHIFT;
    return id ? id : 4u;
}

struct Chunk {
    uint32_t hs[CHUNK];    // hash (NOHASH: no match may start at this position)
    uint32_t c0[CHUNK];    // candidates, position + 1 (0 = none)
    uint32_t c1[CHUNK];
    uint32_t pl[CHUNK];    // [7:0] latest earlier lane with the same hash (0xff none), [8] a later lane has it
    uint32_t mlen[CHUNK];  // longest match found at the position (0 = none)
    uint32_t moff[CHUNK];  // its offset
};

// ---- the per-lane steps of a chunk that starts at cs, in a block of n bytes ---------------------------------------------------------
LE_FN void chunk_hash(const Cfg &c, const uint8_t *src, uint32_t cs, uint32_t n, uint32_t l, Chunk &k)
{
    const uint32_t p = cs + l;
    k.hs[l] = (uint64_t)p + MF_LIMIT <= n ? zenc::hash4(zenc::rd32(src + p), c.group ? HLOG - 1 : HLOG) : NOHASH;
}
LE_FN void chunk_read(const Cfg &c, const uint16_t *ht, uint32_t cs, uint32_t l, Chunk &k)
{
    const uint32_t h = k.hs[l];
    if (h == NOHASH) { k.c0[l] = k.c1[l] = 0; k.pl[l] = 0x1ff; return; }
    uint32_t prev = 0xff, later = 0;
    for (uint32_t j = 0; j < CHUNK; j++)
        if (k.hs[j] == h) {
            if (j < l) prev = j;
            else if (j > l) later = 0x100;
        }
    const uint32_t idx = c.group ? 2 * h : h;
    const uint32_t p = cs + l;
    if (prev != 0xff) {
        k.c0[l] = cs + prev + 1;
        k.c1[l] = c.group ? zenc::slot_pos(ht[idx], cs) : 0;
    } else {
        k.c0[l] = zenc::slot_pos(ht[idx], p);
        k.c1[l] = c.group ? zenc::slot_pos(ht[idx + 1], p) : 0;
    }
    k.pl[l] = prev | later;
}
LE_FN void chunk_update(const Cfg &c, uint16_t *ht, uint32_t cs, uint32_t l, const Chunk &k)
{
    const uint32_t h = k.hs[l], pl = k.pl[l];
    if (h == NOHASH || (pl & 0x100)) return;  // only the last lane of a hash writes its slot
    const uint32_t idx = c.group ? 2 * h : h;
    if (c.group) ht[idx + 1] = (pl & 0xff) != 0xff ? (uint16_t)(cs + (pl & 0xff)) : ht[idx];
    ht[idx] = (uint16_t)(cs + l);
}
LE_FN void chunk_match(const uint8_t *src, uint32_t cs, uint32_t n, uint32_t l, Chunk &k)
{
    const uint32_t p = cs + l;
    uint32_t best = 0, off = 0;
    if (k.hs[l] != NOHASH) {
        const uint32_t v = zenc::rd32(src + p);
        for (int t = 0; t < 2; t++) {
            const uint32_t e = t ? k.c1[l] : k.c0[l];
            if (!e) continue;
            const uint32_t q = e - 1;
            if (q >= p || p - q > MAX_OFFSET || zenc::rd32(src + q) != v) continue;
            const uint32_t len = 4 + zenc::match_len(src + p + 4, src + q + 4, src + n - LAST_LITERALS);
            if (len > best) { best = len; off = p - q; }
        }
    }
    k.mlen[l] = best;
    k.moff[l] = off;
}

// The wave-uniform walk over one chunk from ip (== cs): returns where it stopped; emit(anchor, start, length, offset) takes each
// match (after it is extended backwards into the pending literals).
template <class Emit>
LE_FN uint32_t chunk_walk(const Cfg &c, const uint8_t *src, const Chunk &k, uint32_t cs, uint32_t n, uint32_t &anchor, Emit &emit)
{
    uint32_t ip = cs;
    const uint32_t ce = cs + CHUNK;
    while (ip < ce && (uint64_t)ip + MF_LIMIT <= n) {
        const uint32_t len = k.mlen[ip - cs];
        if (len < MIN_MATCH) {
            ip += c.group == 0 ? 1 + ((ip - anchor) >> c.skip_shift) : 1;
            continue;
        }
        if (c.group == 2 && ip + 1 < ce && k.mlen[ip + 1 - cs] > len) {  // lazy: a longer match one byte on wins
            ip++;
            continue;
        }
        const uint32_t off = k.moff[ip - cs];
        uint32_t p = ip, ml = len;
        while (p > anchor && p > off && src[p - 1] == src[p - 1 - off]) { p--; ml++; }
        emit(anchor, p, ml, off);
        ip = p + ml;
        anchor = ip;
    }
    return ip;
}

// ---- emission -----------------------------------------------------------------------------------------------------------------------
// Everything below is called by all lanes alike with wave-uniform arguments; `lane` of `stride` lanes stores its share of the
// bytes (the host: lane 0 of 1).  The positions are computed by every lane; no byte is stored at or past o.cap.

// n bytes between disjoint ranges
LE_FN void copy_run(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane, uint32_t stride)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef u32x4 u128u __attribute__((aligned(1)));  // 16 bytes at any address (gfx950 does unaligned global accesses)
    const uint32_t whole = n & ~15u;
    for (uint32_t j = 16u * lane; j < whole; j += 16u * stride) {
        const u128u v = *(const u128u *)(src + j);
        *(u128u *)(dst + j) = v;
    }
    for (uint32_t j = whole + lane; j < n; j += stride) dst[j] = src[j];
#else
    for (uint32_t j = lane; j < n; j += stride) dst[j] = src[j];
#endif
}
// the extension bytes of a length whose nibble is 15: v = length - 15 as 255, 255, .., v % 255
LE_FN uint32_t ext_count(uint32_t v) { return v / 255u + 1u; }
LE_FN void put_ext(uint8_t *p, uint32_t cnt, uint32_t v, uint32_t lane, uint32_t stride)
{
    for (uint32_t j = lane; j < cnt; j += stride) p[j] = (uint8_t)(j + 1 < cnt ? 255u : v - 255u * (cnt - 1));
}
// One sequence: token, literal-length extension, ll literals, and with ml != 0 the offset and the match-length extension.  One lane
// per byte of token, extensions and offset; the literals wave-wide, 16 bytes per lane.
LE_FN void put_seq(Out &o, const uint8_t *lit, uint32_t ll, uint32_t ml, uint32_t off, uint32_t lane, uint32_t stride)
{
    const uint32_t el = ll >= 15 ? ext_count(ll - 15) : 0;
    const uint32_t mc = ml ? ml - MIN_MATCH : 0;
    const uint32_t em = mc >= 15 ? ext_count(mc - 15) : 0;
    const uint64_t need = 1ull + el + ll + (ml ? 2u + em : 0u);
    if (o.ovf || o.pos + need > o.cap) {
        o.ovf = true;
        return;
    }
    uint8_t *p = o.p + o.pos;
    if (lane == 0) p[0] = (uint8_t)(((ll < 15 ? ll : 15u) << 4) | (mc < 15 ? mc : 15u));
    if (el) put_ext(p + 1, el, ll - 15, lane, stride);
    copy_run(p + 1 + el, lit, ll, lane, stride);
    if (ml) {
        uint8_t *q = p + 1 + el + ll;
        if (lane == 0) {
            q[0] = (uint8_t)off;
            q[1] = (uint8_t)(off >> 8);
        }
        if (em) put_ext(q + 2, em, mc - 15, lane, stride);
    }
    o.pos += (uint32_t)need;
}
LE_FN void put_le32(Out &o, uint32_t v, uint32_t lane)
{
    if (o.ovf || (uint64_t)o.pos + 4 > o.cap) {
        o.ovf = true;
        return;
    }
    if (lane == 0)
        for (uint32_t i = 0; i < 4; i++) o.p[o.pos + i] = (uint8_t)(v >> (8 * i));
    o.pos += 4;
}

// ---- the lanes on the host ----------------------------------------------------------------------------------------------------------
struct HostLanes {
    static constexpr uint32_t stride = 1;
    uint32_t lane() const { return 0; }
    template <class F>
    void each(F f) const
    {
        for (uint32_t l = 0; l < CHUNK; l++) f(l);
    }
    uint32_t uni(uint32_t v) const { return v; }
    void sync() const {}   // between steps that hand LDS from some lanes to others
    void fence() const {}  // before the wave reads back bytes it stored to memory
    uint32_t xxh32(const uint8_t *p, uint64_t n) const
    {
        lz4::MemReader rd{p};
        return lz4::xxh32(rd, 0, n, 0);
    }
};

// ---- one block ----------------------------------------------------------------------------------------------------------------------
// src[0 .. n) as one raw block at o.pos (n <= MAX_UNIT); on return o.ovf says that the room did not hold it.  ht: HSIZE entries.
template <class L>
LE_FN void block_encode(const L &ln, const Cfg &c, uint16_t *ht, Chunk &k, const uint8_t *src, uint32_t n, Out &o)
{
    const uint32_t lane = ln.lane();
    for (uint32_t i = lane; i < HSIZE; i += L::stride) ht[i] = 0;
    ln.sync();
    uint32_t anchor = 0, ip = 0;
    auto emit = [&](uint32_t anc, uint32_t p, uint32_t ml, uint32_t off) { put_seq(o, src + anc, p - anc, ml, off, lane, L::stride); };
    while (n > MF_LIMIT && (uint64_t)ip + MF_LIMIT <= n && !o.ovf) {
        ln.each([&](uint32_t l) { chunk_hash(c, src, ip, n, l, k); });
        ln.each([&](uint32_t l) { chunk_read(c, ht, ip, l, k); });
        ln.each([&](uint32_t l) {
            chunk_update(c, ht, ip, l, k);
            chunk_match(src, ip, n, l, k);
        });
        ip = ln.uni(chunk_walk(c, src, k, ip, n, anchor, emit));
        anchor = ln.uni(anchor);
        o.pos = ln.uni(o.pos);
        o.ovf = ln.uni(o.ovf);
        ln.sync();  // the next chunk overwrites k
    }
    put_seq(o, src + anchor, n - anchor, 0, 0, lane, L::stride);
}

// ---- one frame ----------------------------------------------------------------------------------------------------------------------
// The 15 header bytes of a frame of n content bytes with the options `opts` (CHIP_LZ4_S_* bits): version 01, independent blocks,
// Content_Size always.
LE_FN void frame_header(uint8_t *h, uint32_t opts, uint64_t n)
{
    const uint32_t flg = 0x40u | 0x20u | ((opts & CHIP_LZ4_S_BLOCK_CHECKSUM) ? 0x10u : 0u) | 0x08u | ((opts & CHIP_LZ4_S_NO_CONTENT_CHECKSUM) ? 0u : 0x04u);
    for (uint32_t i = 0; i < 4; i++) h[i] = (uint8_t)(lz4::MAGIC >> (8 * i));
    h[4] = (uint8_t)flg;
    h[5] = (uint8_t)(opts_block_id(opts) << 4);
    for (uint32_t i = 0; i < 8; i++) h[6 + i] = (uint8_t)(n >> (8 * i));
    lz4::MemReader rd{h};
    h[14] = (uint8_t)(lz4::xxh32(rd, 4, 10, 0) >> 8);
}

// src[0 .. n) as one frame at o.pos: header, independent blocks of at most the block maximum (one that does not come out smaller
// than its content is stored), end mark, content checksum.  A block's attempt gets the room of its content less one byte, so an
// attempt that runs out is the block that is stored.
template <class L>
LE_FN void frame_encode(const L &ln, const Cfg &c, uint32_t opts, uint16_t *ht, Chunk &k, const uint8_t *src, uint32_t n, Out &o)
{
    const uint32_t lane = ln.lane();
    uint8_t h[FRAME_HEADER];
    frame_header(h, opts, n);
    if ((uint64_t)o.pos + FRAME_HEADER > o.cap) {
        o.ovf = true;
        return;
    }
    if (lane == 0)
        for (uint32_t i = 0; i < FRAME_HEADER; i++) o.p[o.pos + i] = h[i];
    o.pos += FRAME_HEADER;
    const uint32_t bmax = 1u << (8 + 2 * opts_block_id(opts));
    const bool bchk = opts & CHIP_LZ4_S_BLOCK_CHECKSUM;
    for (uint32_t bs = 0; bs < n; bs += bmax) {
        const uint32_t bn = n - bs < bmax ? n - bs : bmax;
        const uint32_t hpos = o.pos;
        if ((uint64_t)hpos + 4 > o.cap) {
            o.ovf = true;
            return;
        }
        const uint64_t lim = (uint64_t)hpos + 4 + bn - 1;  // the attempt may take bn - 1 bytes
        Out b = {o.p, hpos + 4, lim < o.cap ? (uint32_t)lim : o.cap, false};
        block_encode(ln, c, ht, k, src + bs, bn, b);
        uint32_t size = b.pos - (hpos + 4), word = size;
        if (b.ovf) {  // stored
            if ((uint64_t)hpos + 4 + bn > o.cap) {
                o.ovf = true;
                return;
            }
            ln.fence();  // the attempt's stores to the same bytes come first
            copy_run(o.p + hpos + 4, src + bs, bn, lane, L::stride);
            size = bn;
            word = bn | 0x80000000u;
        }
        put_le32(o, word, lane);
        o.pos += size;
        if (bchk) {
            ln.fence();
            put_le32(o, ln.xxh32(o.p + hpos + 4, size), lane);
            if (o.ovf) return;
        }
    }
    put_le32(o, 0, lane);
    if (!(opts & CHIP_LZ4_S_NO_CONTENT_CHECKSUM)) put_le32(o, ln.xxh32(src, n), lane);
}

// ---- the host forms -----------------------------------------------------------------------------------------------------------------
struct HostScratch {
    uint16_t ht[HSIZE];
    Chunk k;
};

// CHIP_ENC_FINISHED / CHIP_ENC_NEED_OUTPUT (out_len 0) / CHIP_ENC_ERROR (len > MAX_UNIT)
inline int32_t block_encode_host(const uint8_t *in, uint64_t len, const Cfg &c, uint8_t *out, uint64_t cap, uint64_t &out_len)
{
    out_len = 0;
    if (len > MAX_UNIT) return CHIP_ENC_ERROR;
    HostScratch *s = new HostScratch;
    Out o = {out, 0, cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap, false};
    block_encode(HostLanes{}, c, s->ht, s->k, in, (uint32_t)len, o);
    delete s;
    if (o.ovf) return CHIP_ENC_NEED_OUTPUT;
    out_len = o.pos;
    return CHIP_ENC_FINISHED;
}
inline int32_t frame_encode_host(const uint8_t *in, uint64_t len, const Cfg &c, uint32_t opts, uint8_t *out, uint64_t cap, uint64_t &out_len)
{
    out_len = 0;
    if (len > MAX_UNIT) return CHIP_ENC_ERROR;
    HostScratch *s = new HostScratch;
    Out o = {out, 0, cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap, false};
    frame_encode(HostLanes{}, c, opts, s->ht, s->k, in, (uint32_t)len, o);
    delete s;
    if (o.ovf) return CHIP_ENC_NEED_OUTPUT;
    out_len = o.pos;
    return CHIP_ENC_FINISHED;
}

// chip_encode_bound: the format's own worst case for a block; for a frame the header, end mark and content checksum (23 bytes) and
// per 64 KiB block a header and a block checksum around the stored bytes (larger blocks only need less)
LE_FN uint64_t block_bound(uint64_t n) { return n + n / 255 + 16; }
LE_FN uint64_t frame_bound(uint64_t n) { return n + 8 * ((n + 65535) / 65536) + 23; }

}  // namespace lz4enc
}  // namespace chip
