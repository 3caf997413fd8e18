// zstd frame encoder (RFC 8878): match finding, Huffman literals, FSE sequences, blocks, frame header, XXH64.  The match finder's
// per-lane steps take a lane index: zstd_enc.hip runs them on the 64 lanes of a wavefront, compress_segment below runs them in a
// loop over the lanes, with the same result.  The serial stages (Huffman code and bits, the FSE chain, headers) run on one lane.
// The same source builds for the host (ZE_FN = inline) so that a CPU harness can exercise it without a GPU.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ZE_FN __host__ __device__ inline
// the serial entropy stages are separate functions on the device: inlined into the kernel they would share one register allocation
#define ZE_BIG __host__ __device__ inline __attribute__((noinline))
#else
#define ZE_FN inline
#define ZE_BIG inline
#endif

namespace zenc {

// ---- limits and parameters -----------------------------------------------------------------------------------------------
constexpr uint32_t BLOCK_MAX = 128u << 10;       // Block_Maximum_Size cap (RFC 8878 3.1.1.2.4)
// hash table: 8192 entries of the low 16 bits of a position (16 KiB): one way of 8192 slots or two of 4096.  A slot names the latest
// position before the current one with those low bits, so the table reaches 65 536 bytes back (the 4-byte compare rejects aliases).
constexpr uint32_t HLOG = 13;
constexpr uint32_t HSIZE = 1u << HLOG;
constexpr uint32_t MAX_SEQ = BLOCK_MAX / 4 + 1;  // matches are at least 4 bytes long
constexpr uint32_t HUF_MAXBITS = 11;
constexpr uint32_t MAX_DIST_LOG = 27;            // the window batch frames declare above 2^27 bytes (zstd's default window_log)

// level groups: 0 greedy with a growing skip over incompressible runs, 1 greedy + repeat-offset probe,
// 2 lazy (one step), 3 lazy with two positions per hash slot
struct Cfg {
    uint32_t group;
    uint32_t skip_shift;  // group 0: step = 1 + (bytes since the last match >> skip_shift)
    uint32_t maxdist;     // longest match distance (<= window size)
    uint32_t block_max;   // Block_Maximum_Size
};

struct Seq {
    uint32_t ll, ml, off;  // literal length, match length, offset in bytes (before repeat-offset coding)
    uint32_t ofv;          // Offset_Value
    uint8_t llc, mlc, ofc, pad;
};

// FSE encoding table (libzstd's layout: state values are tableSize + position)
struct FseCT {
    uint16_t state[512];
    int32_t dfs[64];   // deltaFindState per symbol
    uint32_t dnb[64];  // deltaNbBits per symbol
    uint32_t tl;
};

// per-unit working memory (everything except the hash table and the block's literals / sequences)
struct Work {
    uint32_t cnt[256];
    uint32_t hcode[256];
    uint8_t hlen[256];
    int16_t norm[64];
    uint8_t tsym[512];
    uint32_t cumul[66];
    uint16_t order[256];
    uint32_t hnode_w[512];
    uint16_t hnode_p[512];
    uint8_t weights[256];
    uint32_t scnt[3][64];
    int16_t snorm[3][64];
    uint32_t stl[3];
    uint32_t smode[3];
    uint32_t srle[3];
    uint32_t lit_nsym, lit_present;  // of the block's literals (lit_prepare)
    FseCT ct[3];  // LL, OF, ML
    FseCT wct;    // Huffman weights
};

// ---- predefined distributions (RFC 8878 3.1.1.3.2.2) --------------------------------------------------------------------
ZE_FN int16_t def_norm(int k, uint32_t s)
{
    const int16_t LL[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    const int16_t OF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    const int16_t ML[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                            1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    if (k == 0) return s < 36 ? LL[s] : 0;
    if (k == 1) return s < 29 ? OF[s] : 0;
    return s < 53 ? ML[s] : 0;
}
constexpr uint32_t DEF_TL[3] = {6, 5, 6};
constexpr uint32_t MAX_TL[3] = {9, 8, 9};
constexpr uint32_t NSYM[3] = {36, 32, 53};

ZE_FN uint32_t highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

ZE_FN uint32_t ll_code(uint32_t ll, uint32_t &nb, uint32_t &base)
{
    const uint16_t B[20] = {16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65535};
    const uint8_t NB[20] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    if (ll < 16) { nb = 0; base = ll; return ll; }
    uint32_t c;
    if (ll >= 64) c = highbit(ll) - 6 + 25;
    else { c = 8; while (c > 0 && B[c] > ll) c--; c += 16; }
    nb = NB[c - 16];
    base = c == 35 ? 65536u : B[c - 16];
    return c;
}

ZE_FN uint32_t ml_code(uint32_t ml, uint32_t &nb, uint32_t &base)  // ml = match length (>= 3)
{
    const uint16_t B[21] = {35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65535};
    const uint8_t NB[21] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    const uint32_t m = ml - 3;
    if (m < 32) { nb = 0; base = ml; return m; }
    uint32_t c;
    if (m >= 128) c = highbit(m) - 7 + 43;
    else { c = 10; while (c > 0 && B[c] > ml) c--; c += 32; }
    nb = NB[c - 32];
    base = c == 52 ? 65539u : B[c - 32];
    return c;
}

// ---- bounded byte output: nothing is ever stored at or past `cap` ----------------------------------------------------------
struct Out {
    uint8_t *p;
    uint32_t pos, cap;
    bool ovf;
    ZE_FN void put(uint32_t b)
    {
        if (pos < cap) p[pos] = (uint8_t)b;
        else ovf = true;
        pos++;
    }
    ZE_FN void put_le(uint64_t v, uint32_t nbytes)
    {
        for (uint32_t i = 0; i < nbytes; i++) put((uint32_t)(v >> (8 * i)) & 0xff);
    }
    ZE_FN void set(uint32_t at, uint32_t b)
    {
        if (at < cap) p[at] = (uint8_t)b;
    }
};

// forward bit writer (LSB first): FSE table descriptions
struct FBits {
    Out *o;
    uint64_t acc;
    uint32_t n;
    ZE_FN void add(uint32_t v, uint32_t nb)
    {
        acc |= (uint64_t)(v & ((nb < 32) ? ((1u << nb) - 1u) : 0xffffffffu)) << n;
        n += nb;
        while (n >= 8) { o->put((uint32_t)acc & 0xff); acc >>= 8; n -= 8; }
    }
    ZE_FN void close()
    {
        if (n) o->put((uint32_t)acc & 0xff);
        acc = 0;
        n = 0;
    }
};
// backward bitstream writer (RFC 8878 4.1): the same byte order; the decoder starts from the closing 1 bit
typedef FBits BBits;
ZE_FN void bb_close(BBits &b)
{
    b.add(1, 1);
    b.close();
}

// ---- XXH64 (streaming state, carried between the segments of a stream) -----------------------------------------------------
constexpr uint64_t XP1 = 11400714785074694791ULL, XP2 = 14029467366897019727ULL, XP3 = 1609587929392839161ULL,
                   XP4 = 9650029242287828579ULL, XP5 = 2870177450012600261ULL;
struct Xxh {
    uint64_t v[4];
    uint64_t total;
    uint8_t mem[32];
    uint32_t memsize, pad;
};
ZE_FN uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
ZE_FN uint64_t rd64(const uint8_t *p)
{
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}
ZE_FN uint32_t rd32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
ZE_FN uint64_t xround(uint64_t acc, uint64_t in) { return rotl64(acc + in * XP2, 31) * XP1; }
ZE_FN uint64_t xmerge(uint64_t acc, uint64_t v) { return (acc ^ xround(0, v)) * XP1 + XP4; }
ZE_FN void xxh_init(Xxh &s)
{
    s.v[0] = XP1 + XP2;
    s.v[1] = XP2;
    s.v[2] = 0;
    s.v[3] = 0 - XP1;
    s.total = 0;
    s.memsize = 0;
    s.pad = 0;
}
ZE_BIG void xxh_update(Xxh &s, const uint8_t *p, uint32_t n)
{
    s.total += n;
    if (s.memsize + n < 32) {
        for (uint32_t i = 0; i < n; i++) s.mem[s.memsize + i] = p[i];
        s.memsize += n;
        return;
    }
    if (s.memsize) {
        const uint32_t k = 32 - s.memsize;
        for (uint32_t i = 0; i < k; i++) s.mem[s.memsize + i] = p[i];
        for (int j = 0; j < 4; j++) s.v[j] = xround(s.v[j], rd64(s.mem + 8 * j));
        p += k;
        n -= k;
        s.memsize = 0;
    }
    uint64_t v0 = s.v[0], v1 = s.v[1], v2 = s.v[2], v3 = s.v[3];
    while (n >= 32) {
        v0 = xround(v0, rd64(p));
        v1 = xround(v1, rd64(p + 8));
        v2 = xround(v2, rd64(p + 16));
        v3 = xround(v3, rd64(p + 24));
        p += 32;
        n -= 32;
    }
    s.v[0] = v0; s.v[1] = v1; s.v[2] = v2; s.v[3] = v3;
    for (uint32_t i = 0; i < n; i++) s.mem[i] = p[i];
    s.memsize = n;
}
ZE_FN uint64_t xxh_digest(const Xxh &s)
{
    uint64_t h;
    if (s.total >= 32) {
        h = rotl64(s.v[0], 1) + rotl64(s.v[1], 7) + rotl64(s.v[2], 12) + rotl64(s.v[3], 18);
        for (int j = 0; j < 4; j++) h = xmerge(h, s.v[j]);
    } else {
        h = s.v[2] + XP5;
    }
    h += s.total;
    const uint8_t *p = s.mem, *end = s.mem + s.memsize;
    while (p + 8 <= end) { h ^= xround(0, rd64(p)); h = rotl64(h, 27) * XP1 + XP4; p += 8; }
    if (p + 4 <= end) { h ^= (uint64_t)rd32(p) * XP1; h = rotl64(h, 23) * XP2 + XP3; p += 4; }
    while (p < end) { h ^= (*p++) * XP5; h = rotl64(h, 11) * XP1; }
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    return h;
}

// ---- frame header (RFC 8878 3.1.1.1) -----------------------------------------------------------------------------------------
// single segment: Frame_Content_Size = fcs (< 2^32), no Window_Descriptor; otherwise a one-byte Window_Descriptor of 2^wlog
ZE_FN void frame_header(Out &o, bool single, uint32_t fcs, uint32_t wlog)
{
    o.put_le(0xFD2FB528u, 4);
    if (single) {
        const uint32_t fl = fcs < 256 ? 0u : fcs < 65536u + 256u ? 1u : 2u;
        o.put((fl << 6) | (1u << 5) | (1u << 2));
        if (fl == 0) o.put(fcs);
        else if (fl == 1) o.put_le(fcs - 256, 2);
        else o.put_le(fcs, 4);
    } else {
        o.put(1u << 2);
        o.put((wlog - 10) << 3);
    }
}

// ---- FSE (RFC 8878 4.1) ------------------------------------------------------------------------------------------------------
// normalise counts of symbols 0..nsym-1 (total > 0) to 2^tl, every present symbol >= 1
ZE_FN void fse_normalize(const uint32_t *cnt, uint32_t nsym, uint32_t total, uint32_t tl, int16_t *norm)
{
    const uint32_t size = 1u << tl;
    int32_t sum = 0;
    uint32_t big = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        if (!cnt[s]) { norm[s] = 0; continue; }
        uint32_t v = (uint32_t)(((uint64_t)cnt[s] * size + total / 2) / total);
        if (v < 1) v = 1;
        norm[s] = (int16_t)v;
        sum += (int32_t)v;
        if (cnt[s] > cnt[big] || !cnt[big]) big = s;
    }
    int32_t d = (int32_t)size - sum;
    if (d >= 0 || norm[big] + d >= 1) {
        norm[big] = (int16_t)(norm[big] + d);
        return;
    }
    // too many slots handed out: take them back one at a time from the symbols with the most slots
    while (d < 0) {
        uint32_t m = 0;
        for (uint32_t s = 1; s < nsym; s++)
            if (norm[s] > norm[m]) m = s;
        norm[m]--;
        d++;
    }
}

// the table description (RFC 8878 4.1.1), libzstd's FSE_writeNCount bit for bit
ZE_FN void fse_write_ncount(Out &o, const int16_t *norm, uint32_t nsym, uint32_t tl)
{
    FBits b = {&o, 0, 0};
    b.add(tl - 5, 4);
    int32_t remaining = (1 << tl) + 1, threshold = 1 << tl;
    uint32_t nbits = tl + 1, s = 0;
    bool prev0 = false;
    while (s < nsym && remaining > 1) {
        if (prev0) {
            uint32_t start = s;
            while (s < nsym && !norm[s]) s++;
            while (s >= start + 24) { start += 24; b.add(0xffff, 16); }
            while (s >= start + 3) { start += 3; b.add(3, 2); }
            b.add(s - start, 2);
        }
        int32_t count = norm[s++];
        const int32_t max = (2 * threshold - 1) - remaining;
        remaining -= count < 0 ? -count : count;
        count++;
        if (count >= threshold) count += max;
        b.add((uint32_t)count, nbits - (count < max ? 1u : 0u));
        prev0 = count == 1;
        while (remaining < threshold) { nbits--; threshold >>= 1; }
    }
    b.close();
}

ZE_FN void fse_build_ct(Work &w, FseCT &ct, const int16_t *norm, uint32_t nsym, uint32_t tl)
{
    const uint32_t size = 1u << tl, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint32_t high = size - 1;
    w.cumul[0] = 0;
    for (uint32_t u = 1; u <= nsym; u++) {
        if (norm[u - 1] == -1) {
            w.cumul[u] = w.cumul[u - 1] + 1;
            w.tsym[high--] = (uint8_t)(u - 1);
        } else {
            w.cumul[u] = w.cumul[u - 1] + (uint32_t)norm[u - 1];
        }
    }
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; s++)
        for (int32_t k = 0; k < norm[s]; k++) {
            w.tsym[pos] = (uint8_t)s;
            pos = (pos + step) & mask;
            while (pos > high) pos = (pos + step) & mask;
        }
    for (uint32_t u = 0; u < size; u++) ct.state[w.cumul[w.tsym[u]]++] = (uint16_t)(size + u);
    int32_t total = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t c = norm[s];
        if (c == 0) {
            ct.dnb[s] = ((tl + 1) << 16) - size;
        } else if (c == -1 || c == 1) {
            ct.dnb[s] = (tl << 16) - size;
            ct.dfs[s] = total - 1;
            total++;
        } else {
            const uint32_t mbo = tl - highbit((uint32_t)c - 1), msp = (uint32_t)c << mbo;
            ct.dnb[s] = (mbo << 16) - msp;
            ct.dfs[s] = total - c;
            total += c;
        }
    }
    ct.tl = tl;
}

ZE_FN uint32_t fse_init_state(const FseCT &ct, uint32_t s)
{
    const uint32_t nbo = (ct.dnb[s] + (1u << 15)) >> 16;
    const uint32_t v = (nbo << 16) - ct.dnb[s];
    return ct.state[(int32_t)(v >> nbo) + ct.dfs[s]];
}
ZE_FN void fse_encode(BBits &b, const FseCT &ct, uint32_t &state, uint32_t s)
{
    const uint32_t nbo = (state + ct.dnb[s]) >> 16;
    b.add(state, nbo);
    state = ct.state[(int32_t)(state >> nbo) + ct.dfs[s]];
}
ZE_FN void fse_flush_state(BBits &b, const FseCT &ct, uint32_t state) { b.add(state, ct.tl); }

// approximate cost in 1/16 bits of coding cnt[] with norm[] at accuracy tl (no symbol may be missing from norm)
ZE_FN uint32_t fse_cost(const uint32_t *cnt, const int16_t *norm, uint32_t nsym, uint32_t tl, bool &ok)
{
    uint64_t c = 0;
    ok = true;
    for (uint32_t s = 0; s < nsym; s++) {
        if (!cnt[s]) continue;
        const uint32_t p = norm[s] == -1 ? 1u : (uint32_t)(norm[s] > 0 ? norm[s] : 0);
        if (!p) { ok = false; return 0xffffffffu; }
        // -log2(p / 2^tl) in 1/16 bits: 16 * tl - 16 * log2(p), log2 by the high bit and a linear fraction
        const uint32_t hb = highbit(p);
        const uint32_t frac = ((p << 4) >> hb) - 16;  // 0..15
        c += (uint64_t)cnt[s] * (16 * tl - 16 * hb - frac);
    }
    return c > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)c;
}

// ---- Huffman (RFC 8878 4.2) ----------------------------------------------------------------------------------------------------
// code lengths (<= HUF_MAXBITS) for the present symbols of w.cnt[0..nsym); returns the longest length; at least two symbols present
ZE_FN uint32_t huf_lengths(Work &w, uint32_t nsym)
{
    uint32_t n = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        w.hlen[s] = 0;
        if (w.cnt[s]) w.order[n++] = (uint16_t)s;
    }
    // sort by count ascending (insertion sort, ties by symbol)
    for (uint32_t i = 1; i < n; i++) {
        const uint16_t v = w.order[i];
        uint32_t j = i;
        while (j > 0 && w.cnt[w.order[j - 1]] > w.cnt[v]) { w.order[j] = w.order[j - 1]; j--; }
        w.order[j] = v;
    }
    // two-queue Huffman: leaves 0..n-1 in order, internal nodes n.. appended in order of creation
    for (uint32_t i = 0; i < n; i++) w.hnode_w[i] = w.cnt[w.order[i]];
    uint32_t li = 0, ni = n, nn = n;
    for (uint32_t k = 0; k + 1 < n; k++) {
        uint32_t pick[2];
        for (int t = 0; t < 2; t++) {
            if (li < n && (ni >= nn || w.hnode_w[li] <= w.hnode_w[ni])) pick[t] = li++;
            else pick[t] = ni++;
        }
        w.hnode_w[nn] = w.hnode_w[pick[0]] + w.hnode_w[pick[1]];
        w.hnode_p[pick[0]] = (uint16_t)nn;
        w.hnode_p[pick[1]] = (uint16_t)nn;
        nn++;
    }
    // depths: the root is nn-1; internal nodes are created after their children, so walk downwards
    uint8_t *depth = w.tsym;  // 2n - 1 <= 511 entries
    if (!nn) return 0;
    depth[nn - 1] = 0;
    for (int32_t i = (int32_t)nn - 2; i >= 0; i--) {
        const uint32_t d = depth[w.hnode_p[i]] + 1u;
        depth[i] = (uint8_t)(d > 255 ? 255 : d);
    }
    // limit to HUF_MAXBITS and make the code complete again (Kraft sum exactly 2^HUF_MAXBITS)
    const int32_t full = 1 << HUF_MAXBITS;
    int32_t kraft = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t d = depth[i] > HUF_MAXBITS ? HUF_MAXBITS : depth[i];
        w.hlen[w.order[i]] = (uint8_t)d;
        kraft += 1 << (HUF_MAXBITS - d);
    }
    // over-full: lengthen the rarest codes that are not yet at the limit (order[] is rarest first)
    while (kraft > full) {
        for (uint32_t i = 0; i < n && kraft > full; i++) {
            const uint32_t s = w.order[i];
            if (w.hlen[s] < HUF_MAXBITS) {
                kraft -= 1 << (HUF_MAXBITS - w.hlen[s] - 1);
                w.hlen[s]++;
            }
        }
    }
    // under-full: shorten the most frequent codes that still fit
    while (kraft < full) {
        for (int32_t i = (int32_t)n - 1; i >= 0 && kraft < full; i--) {
            const uint32_t s = w.order[i];
            const int32_t gain = 1 << (HUF_MAXBITS - w.hlen[s]);
            if (w.hlen[s] > 1 && kraft + gain <= full) {
                kraft += gain;
                w.hlen[s]--;
            }
        }
    }
    uint32_t maxl = 0;
    for (uint32_t s = 0; s < nsym; s++) maxl = w.hlen[s] > maxl ? w.hlen[s] : maxl;
    // canonical values (libzstd HUF_buildCTable: longest codes get the lowest values, symbols ascending)
    uint32_t nper[HUF_MAXBITS + 2] = {0}, val[HUF_MAXBITS + 2];
    for (uint32_t s = 0; s < nsym; s++) nper[w.hlen[s]]++;
    uint32_t m = 0;
    for (uint32_t l = maxl; l >= 1; l--) {
        val[l] = m;
        m += nper[l];
        m >>= 1;
    }
    for (uint32_t s = 0; s < nsym; s++)
        if (w.hlen[s]) w.hcode[s] = val[w.hlen[s]]++;
    return maxl;
}

// the Huffman tree description (weights of symbols 0..nw-1; the last symbol's weight is implied); false if it does not fit
// the FSE-compressed form (< 128 bytes) and the direct form is not allowed (more than 128 weights)
ZE_FN bool huf_write_tree(Work &w, Out &o, uint32_t nw, uint32_t maxl, uint32_t &form)
{
    for (uint32_t s = 0; s < nw; s++) w.weights[s] = (uint8_t)(w.hlen[s] ? maxl + 1 - w.hlen[s] : 0);
    if (nw <= 128) {
        form = 0;
        o.put(127 + nw);
        for (uint32_t i = 0; i < nw; i += 2) o.put(((uint32_t)w.weights[i] << 4) | (i + 1 < nw ? w.weights[i + 1] : 0u));
        return true;
    }
    form = 1;
    uint32_t wc[13] = {0}, distinct = 0;
    for (uint32_t s = 0; s < nw; s++) wc[w.weights[s]]++;
    for (uint32_t k = 0; k < 13; k++) distinct += wc[k] ? 1 : 0;
    if (distinct < 2) return false;  // one value only: FSE cannot code it (libzstd's HUF_compressWeights declines too)
    uint32_t nsym = 13;
    while (!wc[nsym - 1]) nsym--;
    const uint32_t tl = 6;
    int16_t norm[13] = {0};
    fse_normalize(wc, nsym, nw, tl, norm);
    fse_build_ct(w, w.wct, norm, nsym, tl);
    const uint32_t hdr = o.pos;
    o.put(0);
    const uint32_t start = o.pos;
    fse_write_ncount(o, norm, nsym, tl);
    // two interleaved states, libzstd's FSE_compress_usingCTable order
    BBits b = {&o, 0, 0};
    int32_t i = (int32_t)nw;
    uint32_t s1, s2;
    if (nw & 1) {
        s1 = fse_init_state(w.wct, w.weights[--i]);
        s2 = fse_init_state(w.wct, w.weights[--i]);
        fse_encode(b, w.wct, s1, w.weights[--i]);
    } else {
        s2 = fse_init_state(w.wct, w.weights[--i]);
        s1 = fse_init_state(w.wct, w.weights[--i]);
    }
    while (i > 0) {
        fse_encode(b, w.wct, s2, w.weights[--i]);
        fse_encode(b, w.wct, s1, w.weights[--i]);
    }
    fse_flush_state(b, w.wct, s2);
    fse_flush_state(b, w.wct, s1);
    bb_close(b);
    const uint32_t size = o.pos - start;
    if (size >= 128) return false;
    o.set(hdr, size);
    return true;
}

ZE_FN void huf_stream(Work &w, Out &o, const uint8_t *lit, uint32_t n)
{
    BBits b = {&o, 0, 0};
    for (int32_t i = (int32_t)n - 1; i >= 0; i--) b.add(w.hcode[lit[i]], w.hlen[lit[i]]);
    bb_close(b);
}
ZE_FN uint32_t huf_stream_size(const Work &w, const uint8_t *lit, uint32_t n)
{
    uint64_t bits = 1;
    for (uint32_t i = 0; i < n; i++) bits += w.hlen[lit[i]];
    return (uint32_t)((bits + 7) >> 3);
}

// ---- literals section (RFC 8878 3.1.1.3.1) -------------------------------------------------------------------------------------
ZE_FN void lit_raw_header(Out &o, uint32_t type, uint32_t n)
{
    if (n < 32) o.put(type | (n << 3));
    else if (n < 4096) { o.put(type | (1u << 2) | ((n & 15) << 4)); o.put(n >> 4); }
    else { o.put(type | (3u << 2) | ((n & 15) << 4)); o.put((n >> 4) & 0xff); o.put(n >> 12); }
}
ZE_FN uint32_t lit_raw_header_size(uint32_t n) { return n < 32 ? 1 : n < 4096 ? 2 : 3; }

// The literals section in three steps, so that the parts over all literals can be shared by a wave: with w.cnt holding the
// histogram, lit_prepare builds the Huffman code (returns its longest length, 0 = Raw or RLE literals); lit_bits sums the code
// lengths of the four stream segments (bits[4] = the whole); lit_emit writes the section.  With copy_raw false, Raw literals get their
// header and their room (*raw_at) but the caller copies the bytes.
ZE_BIG uint32_t lit_prepare(Work &w, const uint8_t *lit, uint32_t n)
{
    uint32_t nsym = 256, present = 0;
    while (nsym > 0 && !w.cnt[nsym - 1]) nsym--;
    for (uint32_t s = 0; s < nsym; s++) present += w.cnt[s] ? 1 : 0;
    w.lit_nsym = nsym;
    w.lit_present = present;
    if (n < 16 || present < 2) return 0;
    return huf_lengths(w, nsym);
}
ZE_FN void lit_bits(const Work &w, const uint8_t *lit, uint32_t n, uint32_t *bits)
{
    const uint32_t seg = (n + 3) / 4;
    for (uint32_t k = 0; k < 4; k++) {
        bits[k] = 0;
        const uint32_t a = k * seg, e = k == 3 ? n : (a + seg < n ? a + seg : n);
        for (uint32_t i = a; i < e; i++) bits[k] += w.hlen[lit[i]];
    }
    bits[4] = bits[0] + bits[1] + bits[2] + bits[3];
}
ZE_BIG void lit_emit(Work &w, Out &o, const uint8_t *lit, uint32_t n, uint32_t maxl, const uint32_t *bits, bool copy_raw, uint32_t *raw_at)
{
    const uint32_t start = o.pos;
    const bool ov = o.ovf;
    const uint32_t raw_size = lit_raw_header_size(n) + n;
    *raw_at = 0xffffffffu;
    if (n == 0) { o.put(0); return; }
    if (w.lit_present == 1) {  // RLE literals
        lit_raw_header(o, 1, n);
        o.put(lit[0]);
        return;
    }
    if (maxl) {
        const uint32_t nsym = w.lit_nsym;
        // exact sizes of both layouts: a stream is its bits, the closing 1 bit, rounded up to bytes
        const uint32_t seg = (n + 3) / 4;
        uint32_t s4 = 6;
        for (uint32_t k = 0; k < 4; k++) s4 += (bits[k] + 8) >> 3;
        const uint32_t s1 = (bits[4] + 8) >> 3;
        // the tree description goes right behind the (largest possible) header; its size fixes the header
        const uint32_t hpos = o.pos;
        o.pos += 5;
        uint32_t form = 0;
        const uint32_t tstart = o.pos;
        if (huf_write_tree(w, o, nsym - 1, maxl, form)) {
            const uint32_t tsize = o.pos - tstart;
            const bool single = n <= 1023 && tsize + s1 <= 1023;
            const uint32_t csize = tsize + (single ? s1 : s4);
            const uint32_t big = n > csize ? n : csize;
            const uint32_t sf = single ? 0u : big < 1024 ? 1u : big < 16384 ? 2u : 3u;
            const uint32_t hsize = sf <= 1 ? 3u : sf == 2 ? 4u : 5u;
            if (hsize + csize < raw_size) {
                // move the tree description down behind the real header size
                const uint32_t dst = hpos + hsize;
                for (uint32_t i = 0; i < tsize; i++)
                    if (tstart + i < o.cap) o.set(dst + i, o.p[tstart + i]);
                o.pos = hpos;
                const uint32_t hb = sf <= 1 ? 10u : sf == 2 ? 14u : 18u;
                const uint64_t h = 2u | (sf << 2) | ((uint64_t)n << 4) | ((uint64_t)csize << (4 + hb));
                o.put_le(h, hsize);
                o.pos += tsize;
                if (single) {
                    huf_stream(w, o, lit, n);
                } else {
                    const uint32_t jt = o.pos;
                    o.pos += 6;
                    uint32_t sz[4];
                    for (uint32_t k = 0; k < 4; k++) {
                        const uint32_t a = k * seg, e = k == 3 ? n : a + seg, p0 = o.pos;
                        huf_stream(w, o, lit + a, e - a);
                        sz[k] = o.pos - p0;
                    }
                    for (uint32_t k = 0; k < 3; k++) { o.set(jt + 2 * k, sz[k] & 0xff); o.set(jt + 2 * k + 1, sz[k] >> 8); }
                }
                return;
            }
        }
        o.pos = start;
        o.ovf = ov;
    }
    lit_raw_header(o, 0, n);
    if (copy_raw) {
        for (uint32_t i = 0; i < n; i++) o.put(lit[i]);
    } else {
        *raw_at = o.pos;
        if (o.pos + (uint64_t)n > o.cap) o.ovf = true;
        o.pos += n;
    }
}

ZE_FN void write_literals(Work &w, Out &o, const uint8_t *lit, uint32_t n)
{
    for (uint32_t s = 0; s < 256; s++) w.cnt[s] = 0;
    for (uint32_t i = 0; i < n; i++) w.cnt[lit[i]]++;
    const uint32_t maxl = lit_prepare(w, lit, n);
    uint32_t bits[5] = {0, 0, 0, 0, 0}, raw_at;
    if (maxl) lit_bits(w, lit, n, bits);
    lit_emit(w, o, lit, n, maxl, bits, true, &raw_at);
}

// ---- sequences section (RFC 8878 3.1.1.3.2) -------------------------------------------------------------------------------------
ZE_BIG void write_sequences(Work &w, Out &o, Seq *seq, uint32_t ns)
{
    if (ns < 128) o.put(ns);
    else if (ns < 0x7f00) { o.put((ns >> 8) + 0x80); o.put(ns & 0xff); }
    else { o.put(0xff); o.put_le(ns - 0x7f00, 2); }
    if (!ns) return;
    for (int k = 0; k < 3; k++)
        for (uint32_t s = 0; s < 64; s++) w.scnt[k][s] = 0;
    for (uint32_t i = 0; i < ns; i++) {
        w.scnt[0][seq[i].llc]++;
        w.scnt[1][seq[i].ofc]++;
        w.scnt[2][seq[i].mlc]++;
    }
    const uint32_t mpos = o.pos;
    o.put(0);
    uint32_t modes = 0;
    for (int k = 0; k < 3; k++) {
        const uint32_t nsym = NSYM[k];
        uint32_t last = 0, present = 0;
        for (uint32_t s = 0; s < nsym; s++)
            if (w.scnt[k][s]) { last = s; present++; }
        int16_t *norm = w.snorm[k];
        // Predefined
        for (uint32_t s = 0; s < nsym; s++) norm[s] = def_norm(k, s);
        bool ok;
        uint32_t best = fse_cost(w.scnt[k], norm, nsym, DEF_TL[k], ok), mode = 0;
        if (!ok) best = 0xffffffffu;
        // RLE: one byte, no bits per sequence
        if (present == 1 && 16 * 8 < best) { best = 16 * 8; mode = 1; }
        // FSE_Compressed
        uint32_t tl = MAX_TL[k];
        const uint32_t lim = ns > 1 ? highbit(ns - 1) + 1 : 1;  // no more accuracy than the count supports
        if (tl > lim) tl = lim;
        const uint32_t need = last ? highbit(last) + 1 : 1;  // every present symbol needs a slot
        if (tl < need) tl = need;
        if (tl < 5) tl = 5;
        if (mode != 1 && present > 1) {
            int16_t tn[64];
            fse_normalize(w.scnt[k], last + 1, ns, tl, tn);
            // size of the description: write it at the current position and roll back
            const uint32_t p0 = o.pos;
            const bool ov = o.ovf;
            fse_write_ncount(o, tn, last + 1, tl);
            const uint32_t dsize = o.pos - p0;
            o.pos = p0;
            o.ovf = ov;
            bool ok2;
            const uint32_t c = fse_cost(w.scnt[k], tn, last + 1, tl, ok2) + 16 * 8 * dsize;
            if (ok2 && c < best) {
                best = c;
                mode = 2;
                for (uint32_t s = 0; s < 64; s++) norm[s] = s <= last ? tn[s] : 0;
            }
        }
        if (mode == 0) {
            for (uint32_t s = 0; s < nsym; s++) norm[s] = def_norm(k, s);
            w.stl[k] = DEF_TL[k];
            fse_build_ct(w, w.ct[k], norm, nsym, DEF_TL[k]);
        } else if (mode == 1) {
            w.srle[k] = last;
            w.stl[k] = 0;
        } else {
            w.stl[k] = tl;
            fse_build_ct(w, w.ct[k], norm, last + 1, tl);
        }
        w.smode[k] = mode;
        modes |= mode << (6 - 2 * k);
    }
    o.set(mpos, modes);
    for (int k = 0; k < 3; k++) {
        if (w.smode[k] == 1) o.put(w.srle[k]);
        else if (w.smode[k] == 2) {
            uint32_t last = 0;
            for (uint32_t s = 0; s < NSYM[k]; s++)
                if (w.scnt[k][s]) last = s;
            fse_write_ncount(o, w.snorm[k], last + 1, w.stl[k]);
        }
    }
    // the bitstream: states of the last sequence first, then the sequences backwards (libzstd's ZSTD_encodeSequences)
    BBits b = {&o, 0, 0};
    const bool rl = w.smode[0] == 1, ro = w.smode[1] == 1, rm = w.smode[2] == 1;
    const Seq &z = seq[ns - 1];
    uint32_t sm = rm ? 0 : fse_init_state(w.ct[2], z.mlc);
    uint32_t so = ro ? 0 : fse_init_state(w.ct[1], z.ofc);
    uint32_t sl = rl ? 0 : fse_init_state(w.ct[0], z.llc);
    uint32_t nb, base;
    ll_code(z.ll, nb, base);
    b.add(z.ll - base, nb);
    ml_code(z.ml, nb, base);
    b.add(z.ml - base, nb);
    b.add(z.ofv - (1u << z.ofc), z.ofc);
    for (int32_t i = (int32_t)ns - 2; i >= 0; i--) {
        const Seq &q = seq[i];
        if (!ro) fse_encode(b, w.ct[1], so, q.ofc);
        if (!rm) fse_encode(b, w.ct[2], sm, q.mlc);
        if (!rl) fse_encode(b, w.ct[0], sl, q.llc);
        ll_code(q.ll, nb, base);
        b.add(q.ll - base, nb);
        ml_code(q.ml, nb, base);
        b.add(q.ml - base, nb);
        b.add(q.ofv - (1u << q.ofc), q.ofc);
    }
    if (!rm) fse_flush_state(b, w.ct[2], sm);
    if (!ro) fse_flush_state(b, w.ct[1], so);
    if (!rl) fse_flush_state(b, w.ct[0], sl);
    bb_close(b);
}

// ---- match finding ----------------------------------------------------------------------------------------------------------------
ZE_FN uint32_t hash4(uint32_t v, uint32_t bits) { return (v * 2654435761u) >> (32 - bits); }

// length of the common prefix of a and b, at most end - a: 16 bytes per step
ZE_FN uint32_t match_len(const uint8_t *a, const uint8_t *b, const uint8_t *end)
{
    const uint8_t *s = a;
    while (a + 16 <= end) {
        const uint64_t x0 = rd64(a) ^ rd64(b);
        if (x0) return (uint32_t)(a - s) + ((uint32_t)__builtin_ctzll(x0) >> 3);
        const uint64_t x1 = rd64(a + 8) ^ rd64(b + 8);
        if (x1) return (uint32_t)(a - s) + 8 + ((uint32_t)__builtin_ctzll(x1) >> 3);
        a += 16;
        b += 16;
    }
    while (a < end && *a == *b) { a++; b++; }
    return (uint32_t)(a - s);
}

// The match finder works on chunks of 64 positions, one per lane (the deflate encoder's scheme): every lane hashes its position,
// finds its candidates (the latest earlier lane of the chunk with the same hash, else the table), the last lane of each hash
// updates the table, every lane measures its candidates; then a scalar walk picks greedy / lazy matches from the 64 results and
// the next chunk starts where the walk stopped.  The per-lane steps take the lane index; the host runs them in a loop over the
// lanes, the kernel on the lanes themselves (with an LDS barrier between the steps).
constexpr uint32_t CHUNK = 64;
constexpr uint32_t NOHASH = 0xffffffffu;
struct Chunk {
    uint32_t hs[CHUNK];    // hash (NOHASH: no candidate at this position)
    uint32_t c0[CHUNK];    // candidates, position + 1 (0 = none)
    uint32_t c1[CHUNK];
    uint32_t pl[CHUNK];    // [7:0] latest earlier lane with the same hash (0xff none), [8] a later lane has it
    uint32_t mlen[CHUNK];  // longest match found at the position (0 = none)
    uint32_t moff[CHUNK];  // its offset
};

ZE_FN void chunk_hash(const Cfg &c, const uint8_t *src, uint32_t cs, uint32_t be, uint32_t l, Chunk &k)
{
    const uint32_t p = cs + l;
    k.hs[l] = (uint64_t)p + 8 <= be ? hash4(rd32(src + p), c.group == 3 ? HLOG - 1 : HLOG) : NOHASH;
}
// a table entry (low 16 bits of a position) -> the latest position before p with those bits, + 1 (0 = none)
ZE_FN uint32_t slot_pos(uint32_t e, uint32_t p)
{
    if (p == 0) return 0;
    const uint32_t d = (p - 1 - e) & 0xffffu;
    return d <= p - 1 ? p - d : 0;
}
ZE_FN void chunk_read(const Cfg &c, const uint16_t *ht, uint32_t cs, uint32_t l, Chunk &k)
{
    const uint32_t h = k.hs[l];
    if (h == NOHASH) { k.c0[l] = k.c1[l] = 0; k.pl[l] = 0x1ff; return; }
    uint32_t prev = 0xff, later = 0;
    for (uint32_t j = 0; j < CHUNK; j++)
        if (k.hs[j] == h) {
            if (j < l) prev = j;
            else if (j > l) later = 0x100;
        }
    const uint32_t idx = c.group == 3 ? 2 * h : h;
    const uint32_t p = cs + l;
    if (prev != 0xff) {
        k.c0[l] = cs + prev + 1;
        k.c1[l] = c.group == 3 ? slot_pos(ht[idx], cs) : 0;
    } else {
        k.c0[l] = slot_pos(ht[idx], p);
        k.c1[l] = c.group == 3 ? slot_pos(ht[idx + 1], p) : 0;
    }
    k.pl[l] = prev | later;
}
ZE_FN void chunk_update(const Cfg &c, uint16_t *ht, uint32_t cs, uint32_t l, const Chunk &k)
{
    const uint32_t h = k.hs[l], pl = k.pl[l];
    if (h == NOHASH || (pl & 0x100)) return;  // only the last lane of a hash writes its slot
    const uint32_t idx = c.group == 3 ? 2 * h : h;
    if (c.group == 3) ht[idx + 1] = (pl & 0xff) != 0xff ? (uint16_t)(cs + (pl & 0xff)) : ht[idx];
    ht[idx] = (uint16_t)(cs + l);
}
ZE_FN void chunk_match(const Cfg &c, const uint8_t *src, uint32_t cs, uint32_t be, uint32_t rep0, uint32_t l, Chunk &k)
{
    const uint32_t p = cs + l;
    uint32_t best = 0, off = 0;
    if (k.hs[l] != NOHASH) {
        const uint32_t v = rd32(src + p);
        if (c.group >= 1 && rep0 <= p && rep0 <= c.maxdist && rd32(src + p - rep0) == v) {
            best = 4 + match_len(src + p + 4, src + p + 4 - rep0, src + be);
            off = rep0;
        }
        for (int t = 0; t < 2; t++) {
            const uint32_t e = t ? k.c1[l] : k.c0[l];
            if (!e) continue;
            const uint32_t q = e - 1;
            if (q >= p || p - q > c.maxdist || rd32(src + q) != v) continue;
            const uint32_t len = 4 + match_len(src + p + 4, src + q + 4, src + be);
            if (len > best) { best = len; off = p - q; }
        }
    }
    k.mlen[l] = best;
    k.moff[l] = off;
}

// The scalar walk over one chunk from ip (== cs): returns where it stopped; emit(anchor, start, length, offset) takes each match
// (after it is extended backwards into the pending literals).
template <class Emit>
ZE_FN uint32_t chunk_walk(const Cfg &c, const uint8_t *src, const Chunk &k, uint32_t cs, uint32_t be, uint32_t &anchor, uint32_t &rep0,
                          Emit &emit)
{
    uint32_t ip = cs;
    const uint32_t ce = cs + CHUNK;
    while (ip < ce && (uint64_t)ip + 8 <= be) {
        const uint32_t len = k.mlen[ip - cs];
        if (len < 4) {
            ip += c.group == 0 ? 1 + ((ip - anchor) >> c.skip_shift) : 1;
            continue;
        }
        if (c.group >= 2 && ip + 1 < ce && k.mlen[ip + 1 - cs] > len) {  // lazy: a longer match one byte on wins
            ip++;
            continue;
        }
        const uint32_t off = k.moff[ip - cs];
        uint32_t p = ip, ml = len;
        while (p > anchor && p - off > 0 && src[p - 1] == src[p - 1 - off]) { p--; ml++; }
        emit(anchor, p, ml, off);
        rep0 = off;
        ip = p + ml;
        anchor = ip;
    }
    return ip;
}

// Offset_Value and the repeat-offset history, RFC 8878 3.1.2.5 (rep is updated as the decoder will)
ZE_FN uint32_t offset_value(uint32_t *rep, uint32_t off, uint32_t ll)
{
    uint32_t idx;  // repeat index as the decoder resolves it: 0, 1, 2, or 3 = rep0 - 1
    uint32_t ofv;
    if (ll > 0) {
        if (off == rep[0]) { ofv = 1; idx = 0; }
        else if (off == rep[1]) { ofv = 2; idx = 1; }
        else if (off == rep[2]) { ofv = 3; idx = 2; }
        else { ofv = off + 3; idx = 4; }
    } else {
        if (off == rep[1]) { ofv = 1; idx = 1; }
        else if (off == rep[2]) { ofv = 2; idx = 2; }
        else if (rep[0] > 1 && off == rep[0] - 1) { ofv = 3; idx = 3; }
        else { ofv = off + 3; idx = 4; }
    }
    if (idx == 0) return ofv;
    if (idx == 1) { rep[1] = rep[0]; rep[0] = off; return ofv; }
    rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = off;
    return ofv;
}

// ---- blocks ---------------------------------------------------------------------------------------------------------------------
struct Scratch {
    uint16_t *ht;  // HSIZE entries
    Seq *seq;      // MAX_SEQ
    uint8_t *lit;  // BLOCK_MAX
    Work *w;
};

// phase cycle counters of a diagnostic build: [0] match finding, [1] literals, [2] sequences / FSE, [3] frame + blocks
#if defined(CHIP_STATS) && defined(__HIP_DEVICE_COMPILE__)
#define ZE_CLK() __builtin_readcyclecounter()
#else
#define ZE_CLK() 0ull
#endif

// Offset_Value and codes of the block's sequences; rep[] is advanced as the decoder will
ZE_FN void seq_codes(Seq *seq, uint32_t ns, uint32_t *rep)
{
    for (uint32_t i = 0; i < ns; i++) {
        Seq &s = seq[i];
        s.ofv = offset_value(rep, s.off, s.ll);
        uint32_t nb, base;
        s.llc = (uint8_t)ll_code(s.ll, nb, base);
        s.mlc = (uint8_t)ml_code(s.ml, nb, base);
        s.ofc = (uint8_t)highbit(s.ofv);
    }
}

// The host form of the kernel's segment encoder (zstd_enc.hip encode_segment_wave), step for step and byte for byte: compresses
// src[0 .. n) (sc.ht cleared by the caller) as blocks of at most c.block_max bytes (the last one marked last if `last`; with n == 0
// and `last`, one empty raw block); rep[] carries the repeat offsets between segments.  Returns false when `o` ran out of room.
inline bool compress_segment(const Cfg &c, const Scratch &sc, Chunk &k, const uint8_t *src, uint32_t n, bool last, uint32_t *rep, Out &o)
{
    if (n == 0) {
        if (last) o.put_le(1u, 3);
        return !o.ovf;
    }
    for (uint32_t bs = 0; bs < n; bs += c.block_max) {
        const uint32_t be = n - bs > c.block_max ? bs + c.block_max : n, bn = be - bs;
        const uint32_t lastbit = (last && be == n) ? 1u : 0u;
        const uint32_t hpos = o.pos;
        bool rle = bn > 1;
        for (uint32_t i = bs + 1; i < be && rle; i++) rle = src[i] == src[bs];
        if (rle) {
            o.put_le(lastbit | (1u << 1) | (bn << 3), 3);
            o.put(src[bs]);
            if (o.ovf) return false;
            continue;
        }
        Work &w = *sc.w;
        for (uint32_t s = 0; s < 256; s++) w.cnt[s] = 0;
        uint32_t ns = 0, nl = 0, anchor = bs, rep0 = rep[0], ip = bs;
        auto lits = [&](uint32_t a, uint32_t e) {
            for (uint32_t i = a; i < e; i++) { sc.lit[nl++] = src[i]; w.cnt[src[i]]++; }
        };
        auto emit = [&](uint32_t anc, uint32_t p, uint32_t ml, uint32_t off) {
            lits(anc, p);
            sc.seq[ns].ll = p - anc;
            sc.seq[ns].ml = ml;
            sc.seq[ns].off = off;
            ns++;
        };
        while ((uint64_t)ip + 8 <= be) {
            for (uint32_t l = 0; l < CHUNK; l++) chunk_hash(c, src, ip, be, l, k);
            for (uint32_t l = 0; l < CHUNK; l++) chunk_read(c, sc.ht, ip, l, k);
            for (uint32_t l = 0; l < CHUNK; l++) chunk_update(c, sc.ht, ip, l, k);
            for (uint32_t l = 0; l < CHUNK; l++) chunk_match(c, src, ip, be, rep0, l, k);
            ip = chunk_walk(c, src, k, ip, be, anchor, rep0, emit);
        }
        lits(anchor, be);
        uint32_t nrep[3] = {rep[0], rep[1], rep[2]};
        seq_codes(sc.seq, ns, nrep);
        const uint32_t maxl = lit_prepare(w, sc.lit, nl);
        uint32_t bits[5] = {0, 0, 0, 0, 0}, raw_at;
        if (maxl) lit_bits(w, sc.lit, nl, bits);
        o.pos = hpos + 3;
        lit_emit(w, o, sc.lit, nl, maxl, bits, true, &raw_at);
        write_sequences(w, o, sc.seq, ns);
        const uint32_t csize = o.pos - hpos - 3;
        if (!o.ovf && csize < bn) {
            o.set(hpos, (lastbit | (2u << 1) | (csize << 3)) & 0xff);
            o.set(hpos + 1, (csize << 3 >> 8) & 0xff);
            o.set(hpos + 2, (csize << 3 >> 16) & 0xff);
            rep[0] = nrep[0];
            rep[1] = nrep[1];
            rep[2] = nrep[2];
        } else {  // raw block: the repeat offsets stay as they were
            o.pos = hpos;
            o.ovf = false;
            o.put_le(lastbit | (bn << 3), 3);
            for (uint32_t i = bs; i < be; i++) o.put(src[i]);
            if (o.ovf) return false;
        }
    }
    return !o.ovf;
}

}  // namespace zenc
