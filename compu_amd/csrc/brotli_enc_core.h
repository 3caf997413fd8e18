// brotli stream encoder (RFC 7932): the zstd encoder's chunked match finder (zstd_enc_core.h), commands with the distance ring,
// three prefix codes per metablock (literal, insert-and-copy, distance), simple and complex code descriptions, compressed or
// uncompressed metablocks, the WBITS header, closing and flush.  The match finder's per-lane steps take a lane index:
// brotli_enc.hip runs them on the 64 lanes of a wavefront, compress_segment below runs them in a loop over the lanes, and the
// serial stages are the same functions on both sides, so the host form and the kernel write the same bytes.  Builds for the host
// too (BE_FN = inline) so that a CPU harness can exercise it without a GPU.
#pragma once
#include "zstd_enc_core.h"

#define BE_FN ZE_FN
#define BE_BIG ZE_BIG

namespace benc {

using zenc::Cfg;
using zenc::Chunk;
using zenc::CHUNK;
using zenc::Out;

// ---- limits -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t MB_MAX = 128u << 10;          // input bytes per metablock
constexpr uint32_t MAX_CMD = MB_MAX / 4 + 2;     // matches are at least 4 bytes long, plus a closing literal-only command
constexpr uint32_t NLIT = 256, NIC = 704, NDIST = 64;  // alphabets (distance: 16 short codes + 48, NPOSTFIX = NDIRECT = 0)
constexpr uint32_t MAXBITS = 15;                 // longest code length
constexpr uint32_t MAX_DIST = 65536;             // the hash table's reach (16-bit positions)
constexpr uint8_t NO_DIST = 0xff;                // a command without a distance symbol (implicit code 0, or the metablock ends)

// The quality -> match finder group of compu's BrotliOptions quality (0 = unset = libbrotlienc's default 11): DESIGN.md sec. 4.8
BE_FN uint32_t quality_group(uint32_t q)
{
    if (q == 0 || q > 11) q = 11;
    return q == 1 ? 0u : q <= 4 ? 1u : q <= 9 ? 2u : 3u;
}

struct Cmd {
    uint32_t ins, len, dist;  // literal count, copy length (0: literals only, the metablock's last command), distance in bytes
    uint32_t dextra;          // distance extra bits
    uint16_t ic;              // insert-and-copy symbol
    uint8_t dsym;             // distance symbol, NO_DIST when none is written
    uint8_t dnb;              // number of distance extra bits
};

// per-unit working memory (everything except the hash table and the metablock's literals / commands)
struct Work {
    uint32_t cnt_l[NLIT], cnt_ic[NIC], cnt_d[NDIST];
    uint16_t code_l[NLIT], code_ic[NIC], code_d[NDIST];  // bit-reversed canonical codes (written LSB first)
    uint8_t len_l[NLIT], len_ic[NIC], len_d[NDIST];
    uint32_t key[NIC];        // Huffman: (count << 10 | symbol) of the used symbols, sorted
    uint32_t node_w[2 * NIC];
    uint16_t node_p[2 * NIC];
    uint8_t depth[2 * NIC];
    uint32_t jd[2][2 * NIC];  // the kernel's pointer jumping over the tree: depth so far and ancestor, double-buffered
    uint16_t jp[2][2 * NIC];
    uint8_t tok[NIC], tok_x[NIC];  // code-length tokens of a complex code (0..17) and their extra bits
    uint32_t cl_cnt[18];
    uint8_t cl_len[18], cl_bits[18];
    uint16_t cl_code[18];
};

// ---- LSB-first bit writer over the bounded byte output --------------------------------------------------------------------------
struct Bits {
    Out *o;
    uint64_t acc;
    uint32_t n;  // pending bits in acc (< 8 between calls)
    BE_FN void add(uint32_t v, uint32_t nb)  // nb <= 32
    {
        acc |= ((uint64_t)v & ((1ull << nb) - 1ull)) << n;
        n += nb;
        while (n >= 8) {
            o->put((uint32_t)acc & 0xff);
            acc >>= 8;
            n -= 8;
        }
    }
    BE_FN void align()  // zero padding up to the next byte
    {
        if (n) o->put((uint32_t)acc & 0xff);
        acc = 0;
        n = 0;
    }
    BE_FN uint64_t bitpos() const { return (uint64_t)o->pos * 8 + n; }
};

BE_FN uint32_t rev_bits(uint32_t v, uint32_t nb)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < nb; i++) r |= ((v >> i) & 1u) << (nb - 1 - i);
    return r;
}

// ---- stream framing (RFC 7932 9.1, 9.2) -------------------------------------------------------------------------------------------
BE_FN void write_wbits(Bits &b, uint32_t lgwin)
{
    if (lgwin == 16) b.add(0, 1);
    else if (lgwin == 17) b.add(1, 7);
    else if (lgwin > 17) b.add(((lgwin - 17) << 1) | 1u, 4);
    else b.add(((lgwin - 8) << 4) | 1u, 7);
}
// ISLAST (+ ISLASTEMPTY = 0), MNIBBLES (the fewest that hold MLEN - 1), MLEN - 1, ISUNCOMPRESSED (not for a last metablock)
BE_FN void mlen_header(Bits &b, uint32_t mlen, bool islast, bool uncompressed)
{
    b.add(islast ? 1u : 0u, 1);
    if (islast) b.add(0, 1);
    const uint32_t m = mlen - 1, nib = m < (1u << 16) ? 4u : m < (1u << 20) ? 5u : 6u;
    b.add(nib - 4, 2);
    b.add(m, 4 * nib);
    if (!islast) b.add(uncompressed ? 1u : 0u, 1);
}
BE_FN uint32_t uncompressed_header_bits(uint32_t mlen) { return 4 + 4 * ((mlen - 1) < (1u << 16) ? 4u : (mlen - 1) < (1u << 20) ? 5u : 6u); }
BE_FN void empty_metadata(Bits &b)  // ISLAST = 0, MNIBBLES = 0 (metadata), reserved 0, MSKIPBYTES = 0, zero padding
{
    b.add(0, 1);
    b.add(3, 2);
    b.add(0, 1);
    b.add(0, 2);
    b.align();
}

// ---- insert-and-copy and distance codes (RFC 7932 5, 4) -----------------------------------------------------------------------------
// (arithmetic, not tables: the kernel's lanes call these in their loops, where a local table would live in scratch memory)
BE_FN uint32_t ins_code(uint32_t v, uint32_t &nb, uint32_t &base)
{
    if (v < 6) { nb = 0; base = v; return v; }
    if (v < 130) {
        const uint32_t k = zenc::highbit(v - 2) - 1, q = (v - 2) >> k;
        nb = k;
        base = (q << k) + 2;
        return (k << 1) + q + 2;
    }
    if (v < 2114) {
        const uint32_t h = zenc::highbit(v - 66);
        nb = h;
        base = (1u << h) + 66;
        return h + 10;
    }
    if (v < 6210) { nb = 12; base = 2114; return 21; }
    if (v < 22594) { nb = 14; base = 6210; return 22; }
    nb = 24;
    base = 22594;
    return 23;
}
BE_FN uint32_t copy_code(uint32_t v, uint32_t &nb, uint32_t &base)  // v >= 2
{
    if (v < 10) { nb = 0; base = v; return v - 2; }
    if (v < 134) {
        const uint32_t k = zenc::highbit(v - 6) - 1, q = (v - 6) >> k;
        nb = k;
        base = (q << k) + 6;
        return (k << 1) + q + 4;
    }
    if (v < 2118) {
        const uint32_t h = zenc::highbit(v - 70);
        nb = h;
        base = (1u << h) + 70;
        return h + 12;
    }
    nb = 24;
    base = 2118;
    return 23;
}
// the insert-and-copy symbol of an insert code and a copy code; `implicit` = distance code 0 without a distance symbol.  The
// explicit cells 128, 192, 384 / 256, 320, 512 / 448, 576, 640 (rows: insert code / 8, columns: copy code / 8) come from one
// packed constant.
BE_FN uint32_t ic_symbol(uint32_t insc, uint32_t copc, bool implicit)
{
    const uint32_t low = (copc & 7u) | ((insc & 7u) << 3);
    if (implicit) return (copc < 8 ? 0u : 64u) | low;
    const uint32_t k = 2 * ((copc >> 3) + 3 * (insc >> 3));
    return ((k << 5) + 0x40u + ((0x520D40u >> k) & 0xC0u)) | low;
}
// a distance of NPOSTFIX = NDIRECT = 0: symbol 16 + 2 (nb - 1) + prefix, nb extra bits
BE_FN uint32_t dist_symbol(uint32_t d, uint32_t &nb, uint32_t &extra)
{
    const uint32_t x = d + 3, k = zenc::highbit(x) - 1, prefix = (x >> k) & 1u;
    nb = k;
    extra = x - ((2u + prefix) << k);
    return 16 + 2 * (k - 1) + prefix;
}

// The serial part of the command codes: which ring entry (0..3, 4 = none) each command's distance hits.  ring[] (last distance
// first) is advanced as the decoder will: short code 0 does not push.  Kept in Cmd::dsym until cmd_code_one replaces it.
BE_BIG void ring_codes(Cmd *cmd, uint32_t nc, uint32_t *ring)
{
    for (uint32_t i = 0; i < nc; i++) {
        Cmd &c = cmd[i];
        if (c.len == 0) continue;
        uint32_t sc = 4;
        for (uint32_t r = 0; r < 4 && sc == 4; r++)
            if (c.dist == ring[r]) sc = r;
        c.dsym = (uint8_t)sc;
        if (sc != 0) {
            ring[3] = ring[2];
            ring[2] = ring[1];
            ring[1] = ring[0];
            ring[0] = c.dist;
        }
    }
}
// The rest of one command's codes (independent of the other commands): a ring hit takes short code 0..3, code 0 implicitly where
// the insert-and-copy cell allows it
BE_FN void cmd_code_one(Cmd &c)
{
    uint32_t nb, base;
    const uint32_t insc = ins_code(c.ins, nb, base);
    const uint32_t copc = copy_code(c.len ? c.len : 4u, nb, base);
    const uint32_t sc = c.len ? c.dsym : 0u;
    bool implicit = false;
    c.dsym = NO_DIST;
    c.dnb = 0;
    c.dextra = 0;
    if (c.len == 0) {
        implicit = insc < 8;  // no distance follows either way
    } else if (sc == 0 && insc < 8 && copc < 16) {
        implicit = true;
    } else if (sc < 4) {
        c.dsym = (uint8_t)sc;
    } else {
        uint32_t dnb, dx;
        c.dsym = (uint8_t)dist_symbol(c.dist, dnb, dx);
        c.dnb = (uint8_t)dnb;
        c.dextra = dx;
    }
    c.ic = (uint16_t)ic_symbol(insc, copc, implicit);
}
// bits of a command without its literals: insert-and-copy symbol and extra bits, and the distance
BE_FN uint32_t cmd_bits(const Work &w, const Cmd &c)
{
    uint32_t inb, cnb, base;
    ins_code(c.ins, inb, base);
    copy_code(c.len ? c.len : 4u, cnb, base);
    return w.len_ic[c.ic] + inb + cnb + (c.dsym == NO_DIST ? 0u : w.len_d[c.dsym] + c.dnb);
}

// Codes of the metablock's commands and their symbol counts (the host form; the kernel runs ring_codes on lane 0 and the rest on
// the lanes)
inline void cmd_codes(Work &w, Cmd *cmd, uint32_t nc, uint32_t *ring)
{
    for (uint32_t s = 0; s < NIC; s++) w.cnt_ic[s] = 0;
    for (uint32_t s = 0; s < NDIST; s++) w.cnt_d[s] = 0;
    ring_codes(cmd, nc, ring);
    for (uint32_t i = 0; i < nc; i++) {
        cmd_code_one(cmd[i]);
        w.cnt_ic[cmd[i].ic]++;
        if (cmd[i].dsym != NO_DIST) w.cnt_d[cmd[i].dsym]++;
    }
}

// ---- prefix codes (RFC 7932 3) --------------------------------------------------------------------------------------------------
// Huffman code lengths in four steps, so that the kernel can run the sort and the depths on its lanes (brotli_enc.hip
// huff_lengths_wave) and the merge and the length limit on lane 0, with the same result as the host's huff_lengths.
// 1. w.key[0 .. n) = (count << 10 | symbol) of the used symbols, ascending (the keys are distinct)
// 2. huff_merge: two-queue Huffman; leaves 0..n-1 in key order, internal nodes n.. appended in order of creation (w.node_p)
BE_BIG void huff_merge(Work &w, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) w.node_w[i] = w.key[i] >> 10;
    uint32_t li = 0, ni = n, nn = n;
    for (uint32_t k = 0; k + 1 < n; k++) {
        uint32_t pick[2];
        for (int t = 0; t < 2; t++) {
            if (li < n && (ni >= nn || w.node_w[li] <= w.node_w[ni])) pick[t] = li++;
            else pick[t] = ni++;
        }
        w.node_w[nn] = w.node_w[pick[0]] + w.node_w[pick[1]];
        w.node_p[pick[0]] = (uint16_t)nn;
        w.node_p[pick[1]] = (uint16_t)nn;
        nn++;
    }
    w.node_p[nn - 1] = (uint16_t)(nn - 1);  // the root is its own parent
}
// 3. w.depth[i] = min(depth of node i, 255)
// 4. huff_limit: lengths of the leaves, limited to maxbits, the code made complete again (Kraft sum exactly 2^maxbits)
BE_BIG void huff_limit(Work &w, uint32_t n, uint32_t maxbits, uint8_t *len)
{
    const int32_t full = 1 << maxbits;
    int32_t kraft = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t d = w.depth[i] > maxbits ? maxbits : w.depth[i];
        len[w.key[i] & 1023u] = (uint8_t)d;
        kraft += 1 << (maxbits - d);
    }
    while (kraft > full)  // over-full: lengthen the rarest codes not yet at the limit
        for (uint32_t i = 0; i < n && kraft > full; i++) {
            const uint32_t s = w.key[i] & 1023u;
            if (len[s] < maxbits) {
                kraft -= 1 << (maxbits - len[s] - 1);
                len[s]++;
            }
        }
    while (kraft < full)  // under-full: shorten the most frequent codes that still fit
        for (int32_t i = (int32_t)n - 1; i >= 0 && kraft < full; i--) {
            const uint32_t s = w.key[i] & 1023u;
            const int32_t gain = 1 << (maxbits - len[s]);
            if (len[s] > 1 && kraft + gain <= full) {
                kraft += gain;
                len[s]--;
            }
        }
}
// The host form of all four: code lengths (<= maxbits) of cnt[0 .. nsym); returns the number of used symbols (one used symbol
// gets length 0)
BE_FN uint32_t huff_lengths(Work &w, const uint32_t *cnt, uint32_t nsym, uint32_t maxbits, uint8_t *len)
{
    uint32_t n = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        len[s] = 0;
        if (cnt[s]) w.key[n++] = (cnt[s] << 10) | s;
    }
    if (n < 2) return n;
    uint32_t gap = 1;  // Shell sort, gaps 1, 4, 13, 40, ...
    while (gap < n / 3) gap = 3 * gap + 1;
    for (; gap; gap /= 3)
        for (uint32_t i = gap; i < n; i++) {
            const uint32_t v = w.key[i];
            uint32_t j = i;
            while (j >= gap && w.key[j - gap] > v) { w.key[j] = w.key[j - gap]; j -= gap; }
            w.key[j] = v;
        }
    huff_merge(w, n);
    const uint32_t nn = 2 * n - 1;
    w.depth[nn - 1] = 0;
    for (int32_t i = (int32_t)nn - 2; i >= 0; i--) {  // internal nodes come after their children
        const uint32_t d = w.depth[w.node_p[i]] + 1u;
        w.depth[i] = (uint8_t)(d > 255 ? 255 : d);
    }
    huff_limit(w, n, maxbits, len);
    return n;
}

// canonical codes (shorter first, then by symbol), bit-reversed for the LSB-first stream
BE_FN void canon_codes(const uint8_t *len, uint32_t nsym, uint16_t *code)
{
    uint32_t blc[MAXBITS + 1] = {0}, next[MAXBITS + 1] = {0};
    for (uint32_t s = 0; s < nsym; s++) blc[len[s]]++;
    blc[0] = 0;
    uint32_t c = 0;
    for (uint32_t b = 1; b <= MAXBITS; b++) {
        c = (c + blc[b - 1]) << 1;
        next[b] = c;
    }
    for (uint32_t s = 0; s < nsym; s++) code[s] = len[s] ? (uint16_t)rev_bits(next[len[s]]++, len[s]) : (uint16_t)0;
}

// a run of `r` (>= 3) code lengths as a chain of repeat codes (16: previous length, 2 extra bits; 17: zeros, 3 extra bits); a
// chain of k codes means ((e1 + 3 - 2) << B ... ) + ek + 3, so the digits of r - 3 are written most significant first
BE_FN uint32_t repeat_chain(Work &w, uint32_t t, uint32_t sym, uint32_t r)
{
    const uint32_t bits = sym == 16 ? 2u : 3u, mask = (1u << bits) - 1u;
    const uint32_t start = t;
    r -= 3;
    for (;;) {
        w.tok[t] = (uint8_t)sym;
        w.tok_x[t] = (uint8_t)(r & mask);
        t++;
        r >>= bits;
        if (r == 0) break;
        r--;
    }
    for (uint32_t a = start, e = t - 1; a < e; a++, e--) {
        const uint8_t x = w.tok_x[a];
        w.tok_x[a] = w.tok_x[e];
        w.tok_x[e] = x;
    }
    return t;
}

// The description of the code with lengths len[0 .. nsym) of `used` symbols (abits: bits of a symbol in a simple code) and its
// canonical codes.
BE_BIG void write_code(Work &w, Bits &b, const uint32_t *cnt, uint32_t nsym, uint32_t abits, uint8_t *len, uint16_t *code, uint32_t used)
{
    if (used <= 4) {  // simple code: NSYM - 1, the symbols (shortest code first), for four symbols the tree select
        uint32_t sy[4] = {0, 0, 0, 0}, k = 0;
        for (uint32_t s = 0; s < nsym && k < 4; s++)
            if (cnt[s]) sy[k++] = s;
        if (k == 0) k = 1;  // nothing coded with it: one symbol of length 0
        for (uint32_t i = 1; i < k; i++)
            for (uint32_t j = i; j > 0 && len[sy[j - 1]] > len[sy[j]]; j--) {
                const uint32_t x = sy[j];
                sy[j] = sy[j - 1];
                sy[j - 1] = x;
            }
        b.add(1, 2);
        b.add(k - 1, 2);
        for (uint32_t i = 0; i < k; i++) b.add(sy[i], abits);
        if (k == 4) b.add(len[sy[0]] == 1 ? 1u : 0u, 1);
        canon_codes(len, nsym, code);
        return;
    }
    // complex code: the lengths up to the last used symbol as tokens (a complete code needs nothing behind it)
    uint32_t last = nsym - 1;
    while (!len[last]) last--;
    uint32_t t = 0, prev = 8;  // the decoder's initial "previous non-zero length"
    for (uint32_t i = 0; i <= last;) {
        const uint32_t v = len[i];
        uint32_t r = 1;
        while (i + r <= last && len[i + r] == v) r++;
        i += r;
        if (v == 0) {
            if (r < 3) {
                for (uint32_t j = 0; j < r; j++) { w.tok[t] = 0; w.tok_x[t++] = 0; }
            } else {
                t = repeat_chain(w, t, 17, r);
            }
            continue;
        }
        if (v != prev) {
            w.tok[t] = (uint8_t)v;
            w.tok_x[t++] = 0;
            prev = v;
            r--;
        }
        if (r < 3) {
            for (uint32_t j = 0; j < r; j++) { w.tok[t] = (uint8_t)v; w.tok_x[t++] = 0; }
        } else {
            t = repeat_chain(w, t, 16, r);
        }
    }
    for (uint32_t s = 0; s < 18; s++) w.cl_cnt[s] = 0;
    for (uint32_t i = 0; i < t; i++) w.cl_cnt[w.tok[i]]++;
    const uint32_t cl_used = huff_lengths(w, w.cl_cnt, 18, 5, w.cl_len);
    canon_codes(w.cl_len, 18, w.cl_code);
    for (uint32_t s = 0; s < 18; s++) w.cl_bits[s] = w.cl_len[s];
    if (cl_used == 1)  // one code-length symbol: the decoder reads it with 0 bits, whatever (non-zero) length it is given
        for (uint32_t s = 0; s < 18; s++)
            if (w.cl_cnt[s]) { w.cl_len[s] = 1; w.cl_bits[s] = 0; }
    const uint8_t ORDER[18] = {1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    const uint8_t FIX_V[6] = {0, 7, 3, 2, 1, 15}, FIX_N[6] = {2, 4, 3, 2, 2, 4};
    uint32_t skip = 0;
    if (!w.cl_len[ORDER[0]] && !w.cl_len[ORDER[1]]) skip = w.cl_len[ORDER[2]] ? 2u : 3u;
    uint32_t count = 18;  // with one symbol the decoder reads all 18 lengths; otherwise it stops when the code is complete
    if (cl_used > 1)
        while (!w.cl_len[ORDER[count - 1]]) count--;
    b.add(skip, 2);
    for (uint32_t i = skip; i < count; i++) b.add(FIX_V[w.cl_len[ORDER[i]]], FIX_N[w.cl_len[ORDER[i]]]);
    for (uint32_t i = 0; i < t; i++) {
        const uint32_t s = w.tok[i];
        b.add(w.cl_code[s], w.cl_bits[s]);
        if (s == 16) b.add(w.tok_x[i], 2);
        else if (s == 17) b.add(w.tok_x[i], 3);
    }
    canon_codes(len, nsym, code);
}

// ---- metablocks ---------------------------------------------------------------------------------------------------------------
// Header and prefix codes of a compressed metablock of mlen bytes (w.cnt_* hold the counts, w.len_* the code lengths of used[3]
// symbols): one block type per category, NPOSTFIX = NDIRECT = 0, context mode LSB6, one literal and one distance tree.
BE_BIG void metablock_head(Work &w, Bits &b, uint32_t mlen, bool islast, const uint32_t *used)
{
    mlen_header(b, mlen, islast, false);
    b.add(0, 3);  // NBLTYPESL = NBLTYPESI = NBLTYPESD = 1
    b.add(0, 6);  // NPOSTFIX = 0, NDIRECT = 0
    b.add(0, 2);  // context mode of literal block type 0: LSB6
    b.add(0, 2);  // NTREESL = 1, NTREESD = 1
    write_code(w, b, w.cnt_l, NLIT, 8, w.len_l, w.code_l, used[0]);
    write_code(w, b, w.cnt_ic, NIC, 10, w.len_ic, w.code_ic, used[1]);
    write_code(w, b, w.cnt_d, NDIST, 6, w.len_d, w.code_d, used[2]);
}

// The bits of one command without its literals: insert-and-copy symbol and extra bits (head, <= 15 + 24 + 24) and the distance
BE_FN void cmd_emit_head(const Work &w, Bits &b, const Cmd &c)
{
    uint32_t inb, ibase, cnb, cbase;
    ins_code(c.ins, inb, ibase);
    copy_code(c.len ? c.len : 4u, cnb, cbase);
    b.add(w.code_ic[c.ic], w.len_ic[c.ic]);
    b.add(c.ins - ibase, inb);
    b.add((c.len ? c.len : 4u) - cbase, cnb);
}
BE_FN void cmd_emit_dist(const Work &w, Bits &b, const Cmd &c)
{
    if (c.dsym == NO_DIST) return;
    b.add(w.code_d[c.dsym], w.len_d[c.dsym]);
    b.add(c.dextra, c.dnb);
}
BE_BIG void emit_commands(const Work &w, Bits &b, const Cmd *cmd, uint32_t nc, const uint8_t *lit)
{
    uint32_t li = 0;
    for (uint32_t i = 0; i < nc; i++) {
        const Cmd &c = cmd[i];
        cmd_emit_head(w, b, c);
        for (uint32_t j = 0; j < c.ins; j++) {
            const uint32_t l = lit[li++];
            b.add(w.code_l[l], w.len_l[l]);
        }
        cmd_emit_dist(w, b, c);
    }
}

struct Scratch {
    uint16_t *ht;  // zenc::HSIZE entries
    Cmd *cmd;      // MAX_CMD
    uint8_t *lit;  // MB_MAX
    Work *w;
};

// The match finder's configuration for a segment: a window of 2^lgwin - 16 bytes, and no further than the hash table reaches
BE_FN Cfg make_cfg(uint32_t group, uint32_t lgwin)
{
    Cfg c;
    c.group = group;
    c.skip_shift = 8;
    const uint32_t win = (1u << lgwin) - 16;
    c.maxdist = win < MAX_DIST ? win : MAX_DIST;
    c.block_max = MB_MAX;
    return c;
}

// The host form of the kernel's segment encoder (brotli_enc.hip encode_segment_wave), step for step and byte for byte: writes
// src[0 .. n) (sc.ht cleared by the caller) into the bit stream `b` (the WBITS field first if `first`) as metablocks of at most
// MB_MAX bytes, each compressed or uncompressed, whichever is smaller; `last` closes the stream, otherwise the segment ends byte
// aligned (an empty metadata metablock pads it when needed).  ring[] (last distance first) is carried between segments.  Returns
// false when `o` ran out of room.
inline bool compress_segment(const Cfg &c, const Scratch &sc, Chunk &k, const uint8_t *src, uint32_t n, bool first, bool last,
                             uint32_t lgwin, uint32_t *ring, Out &o)
{
    Bits b = {&o, 0, 0};
    if (first) write_wbits(b, lgwin);
    Work &w = *sc.w;
    for (uint32_t bs = 0; bs < n; bs += MB_MAX) {
        const uint32_t be = n - bs > MB_MAX ? bs + MB_MAX : n, bn = be - bs;
        const bool islast = last && be == n;
        for (uint32_t s = 0; s < NLIT; s++) w.cnt_l[s] = 0;
        uint32_t nc = 0, nl = 0, anchor = bs, rep0 = ring[0], ip = bs;
        auto lits = [&](uint32_t a, uint32_t e) {
            for (uint32_t i = a; i < e; i++) { sc.lit[nl++] = src[i]; w.cnt_l[src[i]]++; }
        };
        auto emit = [&](uint32_t anc, uint32_t p, uint32_t ml, uint32_t off) {
            lits(anc, p);
            sc.cmd[nc].ins = p - anc;
            sc.cmd[nc].len = ml;
            sc.cmd[nc].dist = off;
            nc++;
        };
        while ((uint64_t)ip + 8 <= be) {
            for (uint32_t l = 0; l < CHUNK; l++) zenc::chunk_hash(c, src, ip, be, l, k);
            for (uint32_t l = 0; l < CHUNK; l++) zenc::chunk_read(c, sc.ht, ip, l, k);
            for (uint32_t l = 0; l < CHUNK; l++) zenc::chunk_update(c, sc.ht, ip, l, k);
            for (uint32_t l = 0; l < CHUNK; l++) zenc::chunk_match(c, src, ip, be, rep0, l, k);
            ip = zenc::chunk_walk(c, src, k, ip, be, anchor, rep0, emit);
        }
        if (anchor < be) {  // the closing literal-only command
            sc.cmd[nc].ins = be - anchor;
            sc.cmd[nc].len = 0;
            sc.cmd[nc].dist = 0;
            nc++;
            lits(anchor, be);
        }
        uint32_t nring[4] = {ring[0], ring[1], ring[2], ring[3]};
        cmd_codes(w, sc.cmd, nc, nring);
        const uint32_t used[3] = {huff_lengths(w, w.cnt_l, NLIT, MAXBITS, w.len_l), huff_lengths(w, w.cnt_ic, NIC, MAXBITS, w.len_ic),
                                  huff_lengths(w, w.cnt_d, NDIST, MAXBITS, w.len_d)};
        // the end of the uncompressed form, and of the compressed one: its header and codes, then the commands' bits
        const uint64_t raw_end = ((b.bitpos() + uncompressed_header_bits(bn) + 7) & ~7ull) + 8ull * bn + (islast ? 2u : 0u);
        const Bits b0 = b;
        const uint32_t pos0 = o.pos;
        metablock_head(w, b, bn, islast, used);
        uint64_t body = 0;
        for (uint32_t i = 0; i < nc; i++) body += cmd_bits(w, sc.cmd[i]);
        for (uint32_t i = 0; i < nl; i++) body += w.len_l[sc.lit[i]];
        if (!o.ovf && b.bitpos() + body < raw_end) {
            emit_commands(w, b, sc.cmd, nc, sc.lit);
            for (int r = 0; r < 4; r++) ring[r] = nring[r];
        } else {  // uncompressed: the ring stays as it was; a last one is followed by an empty last metablock
            o.pos = pos0;
            o.ovf = false;
            b = b0;
            mlen_header(b, bn, false, true);
            b.align();
            for (uint32_t i = bs; i < be; i++) o.put(src[i]);
            if (islast) b.add(3, 2);
        }
        if (o.ovf) return false;
    }
    if (last) {
        if (n == 0) b.add(3, 2);
        b.align();
    } else if (b.n) {
        empty_metadata(b);
    }
    return !o.ovf;
}

}  // namespace benc
