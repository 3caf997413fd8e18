// Brotli decoder (RFC 7932) for gfx950: one wavefront per unit on a persistent grid.
//
// The bit stream is walked by the whole wave with wave-uniform state (a literal's context depends on the two bytes in front
// of it, so literal decoding is serial); the lanes zero and fill the Huffman tables, copy back-references, uncompressed
// metablocks and dictionary words.  Output is written straight into the unit's range: the window is the output, and a
// distance beyond min(position, 2^WBITS - 16) is a static-dictionary reference whatever a streaming caller still holds.
//
// Tables.  Every prefix code is a two-level table of 16-bit entries (4 bits length, 12 bits symbol or subtable offset) with an
// 8-bit root, built in a per-wave slot of HBM together with the context maps (layout below).  A metablock may carry 256 trees
// in each category, about 1.35 MB of tables; common encoder output needs a few KB to a few hundred.  The first launch gives
// every wave SLOT_SMALL bytes.  A unit whose metablock does not fit is appended to an overflow list and left; a second launch
// of the same kernel, always enqueued behind the first, takes that list on a small grid with SLOT_LARGE bytes per wave and
// decodes those units again from their start (or from their streaming checkpoint).
#include <mutex>

#include "chip_internal.h"
#include "launch_slots.h"
#define BROTLI_TAB_SPACE __device__
#include "brotli_tables.h"

namespace chip {
namespace {

namespace bt = brotli_tab;

__device__ const uint8_t BROTLI_DICT[bt::DICT_SIZE] = {
#include "build/brotli_dict.inc"
};

// BrotliDecoderErrorCode values (negative), passed through as DecodeError (src/decoder/brotli_c.rs:50-59)
enum : int32_t {
    BE_EXUBERANT_NIBBLE = -1,
    BE_RESERVED = -2,
    BE_EXUBERANT_META_NIBBLE = -3,
    BE_SIMPLE_HUFFMAN_ALPHABET = -4,
    BE_SIMPLE_HUFFMAN_SAME = -5,
    BE_CL_SPACE = -6,
    BE_HUFFMAN_SPACE = -7,
    BE_CONTEXT_MAP_REPEAT = -8,
    BE_BLOCK_LENGTH_1 = -9,
    BE_BLOCK_LENGTH_2 = -10,
    BE_TRANSFORM = -11,
    BE_DICTIONARY = -12,
    BE_WINDOW_BITS = -13,
    BE_PADDING_1 = -14,
    BE_PADDING_2 = -15,
    BE_DISTANCE = -16,
    BE_UNREACHABLE = -31,
};
constexpr int32_t ST_OVERFLOW = 0x7ffffffe;  // the metablock's tables did not fit the wave's slot

// Slot layout (bytes): context modes, literal context map, distance context map, heap offsets of the trees, the code length
// code's table, then the heap of Huffman tables (16-bit entries).
constexpr uint32_t OFF_MODES = 0, OFF_LMAP = 256, OFF_DMAP = OFF_LMAP + 64 * 256, OFF_TREES = OFF_DMAP + 4 * 256;
constexpr uint32_t OFF_CLTAB = OFF_TREES + 3 * 256 * 4, OFF_HEAP = OFF_CLTAB + 256 * 2;
// The worst case: 256 trees per category at the table bounds of an 8-bit root (630 entries for 256 symbols, 1080 for 704, 920
// for the largest distance alphabet, 520 symbols), the block type and count trees, context map codes.
constexpr uint32_t SLOT_LARGE = OFF_HEAP + 2u * (256u * (630u + 1080u + 920u) + 3u * (662u + 402u) + 662u) + 4096u;
constexpr uint32_t SLOT_SMALL = 128u << 10;
constexpr uint32_t LARGE_BLOCKS = 64;  // grid of the overflow launch
constexpr uint32_t IN_LEN_MAX = (1u << 29) - 64u;

struct BLds {
    uint8_t lens[720];      // code lengths of the prefix code being read
    uint16_t sorted[720];   // its symbols in canonical order
    uint32_t lit_tree[64];  // heap offsets of the literal trees of the current block type, by literal context
    uint8_t mtf[256];       // inverse move-to-front of a context map
    uint8_t wbuf[64];       // a transformed dictionary word
};

// the unit's input as dwords (aligned down), read through a 64-bit window; bit positions are absolute (from the aligned base)
struct Br {
    const uint32_t *g32;
    uint32_t total_dw;
    uint32_t pos, end;
    uint32_t wpos;
    uint64_t w;
};
__device__ __forceinline__ uint32_t ldw(const Br &b, uint32_t i) { return i < b.total_dw ? b.g32[i] : 0u; }
__device__ __forceinline__ void br_load(Br &b)
{
    b.wpos = b.pos >> 5;
    b.w = (uint64_t)ldw(b, b.wpos) | ((uint64_t)ldw(b, b.wpos + 1) << 32);
}
// 32 bits from the read position (zeros past the input: a caller checks the bits it uses against `end`)
__device__ __forceinline__ uint32_t br_peek(Br &b)
{
    const uint32_t d = (b.pos >> 5) - b.wpos;
    if (d == 1) {
        b.w = (b.w >> 32) | ((uint64_t)ldw(b, b.wpos + 2) << 32);
        b.wpos++;
    } else if (d != 0) {
        br_load(b);
    }
    return (uint32_t)(b.w >> (b.pos & 31u));
}
__device__ __forceinline__ uint32_t bmask(uint32_t n) { return (uint32_t)((1ull << n) - 1ull); }

__device__ __forceinline__ uint32_t hdecode(const uint16_t *t, uint32_t x, uint32_t &len)
{
    uint32_t e = t[x & 255u];
    const uint32_t nb = e >> 12;
    if (nb > 8) {
        const uint32_t sub = nb - 8;
        e = t[(e & 0xfffu) + ((x >> 8) & bmask(sub))];
        len = 8 + (e >> 12);
    } else {
        len = nb;
    }
    return e & 0xfffu;
}

// Builds the table of the complete prefix code whose lengths are L.lens[0 .. n) (at least two used symbols, lengths <= 15) at
// tab; returns its size in entries, 0 if it would pass `cap`.
__device__ uint32_t build_table(uint16_t *tab, uint32_t cap, BLds &L, uint32_t n)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = lanemask_lt();
    if (cap < 256) return 0;
    // lane j keeps the number of codes of length j, then the next free slot of length j in the canonical order
    uint32_t cnt = 0;
    for (uint32_t s0 = 0; s0 < n; s0 += 64) {
        const uint32_t l = s0 + lane < n ? L.lens[s0 + lane] : 0u;
        for (uint32_t len = 1; len <= 15; len++) {
            const uint64_t m = __ballot(l == len);
            if (lane == len) cnt += (uint32_t)__popcll(m);
        }
    }
    uint32_t next = wave_incl_scan(lane >= 1 && lane <= 15 ? cnt : 0u) - (lane >= 1 && lane <= 15 ? cnt : 0u);
    for (uint32_t s0 = 0; s0 < n; s0 += 64) {
        const uint32_t l = s0 + lane < n ? L.lens[s0 + lane] : 0u;
        for (uint32_t len = 1; len <= 15; len++) {
            const uint64_t m = __ballot(l == len);
            if (!m) continue;
            const uint32_t base = rdlane(next, len);
            if (l == len) L.sorted[base + (uint32_t)__popcll(m & lt)] = (uint16_t)(s0 + lane);
            if (lane == len) next += (uint32_t)__popcll(m);
        }
    }
    LSYNC();
    uint32_t rem = cnt;  // lane j: codes of length j not placed yet
    uint32_t size = 256, code = 0, k = 0, sub_prefix = ~0u, sub_base = 0, sub_bits = 0;
    for (uint32_t len = 1; len <= 15; len++) {
        const uint32_t c = rdlane(cnt, len);
        for (uint32_t i = 0; i < c; i++, code++) {
            const uint32_t sym = L.sorted[k++];
            if (len <= 8) {
                const uint32_t r = __builtin_bitreverse32(code) >> (32 - len);
                const uint16_t e = (uint16_t)((len << 12) | sym);
                for (uint32_t j = r + (lane << len); j < 256; j += 64u << len) tab[j] = e;
            } else {
                const uint32_t prefix = code >> (len - 8);
                if (prefix != sub_prefix) {
                    // subtable size: enough bits for the codes that share this 8-bit prefix (the code is complete)
                    int32_t left = 1 << (len - 8);
                    uint32_t l2 = len;
                    while (l2 < 15) {
                        left -= (int32_t)rdlane(rem, l2);
                        if (left <= 0) break;
                        l2++;
                        left <<= 1;
                    }
                    sub_bits = l2 - 8;
                    sub_base = size;
                    size += 1u << sub_bits;
                    if (size > cap || size > 4096) return 0;
                    if (lane == 0) tab[__builtin_bitreverse32(prefix) >> 24] = (uint16_t)(((8 + sub_bits) << 12) | sub_base);
                    sub_prefix = prefix;
                }
                const uint32_t sl = len - 8;
                const uint32_t r = __builtin_bitreverse32(code & bmask(sl)) >> (32 - sl);
                const uint16_t e = (uint16_t)((sl << 12) | sym);
                for (uint32_t j = r + (lane << sl); j < (1u << sub_bits); j += 64u << sl) tab[sub_base + j] = e;
            }
            if (lane == len) rem--;
        }
        code <<= 1;
    }
    return size;
}

// a code with one symbol: every root entry gives it, reading no bits
__device__ void fill_single(uint16_t *tab, uint32_t sym)
{
    for (uint32_t j = lane_id(); j < 256; j += 64) tab[j] = (uint16_t)sym;
}

__device__ __forceinline__ uint32_t bitlen(uint32_t x) { return x ? 32u - (uint32_t)__clz((int)x) : 0u; }

// forward copy of n bytes from `dist` bytes back (dist >= 1)
__device__ void wave_back_copy(uint8_t *dst, uint32_t dist, uint32_t n)
{
    const uint32_t lane = lane_id();
    const uint8_t *src = dst - dist;
    if (dist >= n) {
        for (uint32_t j = lane; j < n; j += 64) dst[j] = src[j];
    } else if (dist >= 64) {
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t j = base + lane;
            const uint8_t v = j < n ? src[j] : (uint8_t)0;
            if (j < n) dst[j] = v;
        }
    } else {
        for (uint32_t j = lane; j < n; j += 64) dst[j] = src[j % dist];
    }
}

// UTF-8 uppercasing of RFC 7932 Appendix B: returns the bytes stepped over
__device__ uint32_t to_upper(uint8_t *p)
{
    if (p[0] < 0xc0) {
        if (p[0] >= 'a' && p[0] <= 'z') p[0] ^= 32;
        return 1;
    }
    if (p[0] < 0xe0) {
        p[1] ^= 32;
        return 2;
    }
    p[2] ^= 5;
    return 3;
}

struct Unit {
    uint32_t u;
    uint8_t *arena;
    uint32_t slot_bytes;
};

// Decodes one unit; returns its status (ST_OVERFLOW: the tables did not fit, nothing final was written).
__device__ __forceinline__ int32_t decode_unit(const BatchArgs &a, const Unit &U, BLds &L)
{
    const uint32_t lane = lane_id();
    const uint32_t u = U.u;
    const uint8_t *gin = a.in_base + a.in_off[u];
    // bit positions are 32-bit: a longer unit reads as truncated
    const uint32_t in_len = a.in_len[u] < IN_LEN_MAX ? a.in_len[u] : IN_LEN_MAX;
    uint8_t *gout = a.out_base + a.out_off[u];
    const uint32_t cap = a.out_cap[u];
    uint8_t *const arena = U.arena;
    uint8_t *const modes = arena + OFF_MODES;
    uint8_t *const lmap = arena + OFF_LMAP;
    uint8_t *const dmap = arena + OFF_DMAP;
    uint32_t *const trees = (uint32_t *)(arena + OFF_TREES);  // [0..256) literal, [256..512) insert-and-copy, [512..768) distance
    uint16_t *const cltab = (uint16_t *)(arena + OFF_CLTAB);
    uint16_t *const heap = (uint16_t *)(arena + OFF_HEAP);
    const uint32_t heap_cap = (U.slot_bytes - OFF_HEAP) / 2;

    Br br;
    const uint32_t mis = (uint32_t)((uintptr_t)gin & 3u);
    br.g32 = (const uint32_t *)(gin - mis);
    br.total_dw = (mis + in_len + 3u) >> 2;
    const uint32_t B0 = mis * 8u;
    br.end = B0 + in_len * 8u;
    br.pos = B0;

    int32_t st = ST_RUNNING;
    uint32_t opos = 0;
    uint32_t ring[4] = {16, 15, 11, 4};  // ring[ridx & 3] is the oldest; the last distance is ring[(ridx - 1) & 3]
    uint32_t ridx = 0;
    uint32_t wbits = 0;
    // libbrotlidec's ring buffer size (BrotliCalculateRingBufferSize: the smallest power of two, up to the window, that holds the
    // output so far and the metablock; 0 = none yet).  Its verdicts depend on it: a metablock whose commands run past MLEN is
    // BLOCK_LENGTH_1 where the ring buffer is flushed (at its end, or when the input runs out) and BLOCK_LENGTH_2 where the
    // metablock ends.
    uint32_t rsz = 0;
    int32_t remaining = 1;  // bytes left in the current compressed metablock (negative: commands ran past MLEN)
    uint32_t *const rs = a.resume;  // streaming decoder: checkpoint of this (single) unit, else nullptr
    const uint64_t dropped = rs ? (uint64_t)rs[12] | ((uint64_t)rs[13] << 32) : 0ull;
    bool resumed = false;
    if (rs && rs[0] != 0 && rs[0] - 1u <= in_len * 8u && rs[1] <= cap) {
        resumed = true;
        br.pos = B0 + rs[0] - 1u;
        opos = rs[1];
        for (int k = 0; k < 4; k++) ring[k] = rs[2 + k];
        ridx = 0;
        wbits = rs[6] & 0xffu;
        rsz = rs[7];
    }
    br_load(br);

#define NEED(n) do { if ((n) > br.end - br.pos) { st = CHIP_NEED_INPUT; goto done; } } while (0)
#define GETBITS(var, n) do { const uint32_t n_ = (n); NEED(n_); var = br_peek(br) & bmask(n_); br.pos += n_; } while (0)
#define READSYM(var, tab) do { const uint32_t x_ = br_peek(br); uint32_t l_; var = hdecode((tab), x_, l_); NEED(l_); br.pos += l_; } while (0)
#define FAIL(code) do { st = (code); goto done; } while (0)
#define FENCE() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup")

    // Reads one prefix code over `alpha` symbols into heap[hp ..): tab = its table, hp advanced past it.  (A macro so that
    // NEED / FAIL leave the whole decode.)
#define READ_CODE(alpha, tab_out, advance)                                                                                         \
    do {                                                                                                                           \
        const uint32_t alpha_ = (alpha);                                                                                           \
        uint16_t *t_ = heap + hp;                                                                                                  \
        uint32_t hskip_;                                                                                                           \
        GETBITS(hskip_, 2);                                                                                                        \
        uint32_t size_ = 0;                                                                                                        \
        if (hskip_ == 1) {                                                                                                         \
            uint32_t nsm1_, s_[4] = {0, 0, 0, 0};                                                                                  \
            GETBITS(nsm1_, 2);                                                                                                     \
            const uint32_t nb_ = bitlen(alpha_ - 1);                                                                               \
            for (uint32_t i_ = 0; i_ <= nsm1_; i_++) {                                                                             \
                uint32_t v_;                                                                                                       \
                GETBITS(v_, nb_);                                                                                                  \
                if (v_ >= alpha_) FAIL(BE_SIMPLE_HUFFMAN_ALPHABET);                                                                \
                s_[i_] = v_;                                                                                                       \
            }                                                                                                                      \
            for (uint32_t i_ = 0; i_ < nsm1_; i_++)                                                                                \
                for (uint32_t j_ = i_ + 1; j_ <= nsm1_; j_++)                                                                      \
                    if (s_[i_] == s_[j_]) FAIL(BE_SIMPLE_HUFFMAN_SAME);                                                            \
            if (heap_cap - hp < 256) FAIL(ST_OVERFLOW);                                                                            \
            if (nsm1_ == 0) {                                                                                                      \
                fill_single(t_, s_[0]);                                                                                            \
                size_ = 256;                                                                                                       \
            } else {                                                                                                               \
                uint32_t tsel_ = 0;                                                                                                \
                if (nsm1_ == 3) GETBITS(tsel_, 1);                                                                                 \
                for (uint32_t j_ = lane; j_ < alpha_; j_ += 64) L.lens[j_] = 0;                                                    \
                LSYNC();                                                                                                           \
                if (lane == 0) {                                                                                                   \
                    if (nsm1_ == 1) {                                                                                              \
                        L.lens[s_[0]] = 1;                                                                                         \
                        L.lens[s_[1]] = 1;                                                                                         \
                    } else if (nsm1_ == 2) {                                                                                       \
                        L.lens[s_[0]] = 1;                                                                                         \
                        L.lens[s_[1]] = 2;                                                                                         \
                        L.lens[s_[2]] = 2;                                                                                         \
                    } else if (tsel_ == 0) {                                                                                       \
                        L.lens[s_[0]] = L.lens[s_[1]] = L.lens[s_[2]] = L.lens[s_[3]] = 2;                                         \
                    } else {                                                                                                       \
                        L.lens[s_[0]] = 1;                                                                                         \
                        L.lens[s_[1]] = 2;                                                                                         \
                        L.lens[s_[2]] = 3;                                                                                         \
                        L.lens[s_[3]] = 3;                                                                                         \
                    }                                                                                                              \
                }                                                                                                                  \
                LSYNC();                                                                                                           \
                size_ = build_table(t_, heap_cap - hp, L, alpha_);                                                                 \
                if (!size_) FAIL(ST_OVERFLOW);                                                                                     \
            }                                                                                                                      \
        } else {                                                                                                                   \
            /* code length code lengths, read with the fixed code of Section 3.5 */                                              \
            if (lane < 18) L.lens[lane] = 0;                                                                                       \
            LSYNC();                                                                                                               \
            uint32_t space_ = 32, num_ = 0, one_ = 0;                                                                              \
            for (uint32_t i_ = hskip_; i_ < 18; i_++) {                                                                            \
                const uint32_t ix_ = br_peek(br) & 15u;                                                                            \
                const uint32_t cl_len_ = (0x4222322242223222ull >> (4 * ix_)) & 15u;                                               \
                const uint32_t v_ = (0x5340234013402340ull >> (4 * ix_)) & 15u;                                                    \
                NEED(cl_len_);                                                                                                     \
                br.pos += cl_len_;                                                                                                 \
                if (lane == 0) L.lens[bt::CL_ORDER[i_]] = (uint8_t)v_;                                                             \
                if (v_ != 0) {                                                                                                     \
                    space_ -= 32u >> v_;                                                                                           \
                    num_++;                                                                                                        \
                    one_ = bt::CL_ORDER[i_];                                                                                       \
                    if (space_ - 1u >= 32u) break;                                                                                 \
                }                                                                                                                  \
            }                                                                                                                      \
            if (!(num_ == 1 || space_ == 0)) FAIL(BE_CL_SPACE);                                                                    \
            LSYNC();                                                                                                               \
            if (num_ == 1) {                                                                                                       \
                fill_single(cltab, one_);                                                                                          \
            } else {                                                                                                               \
                build_table(cltab, 256, L, 18);                                                                                    \
            }                                                                                                                      \
            FENCE();                                                                                                               \
            for (uint32_t j_ = lane; j_ < alpha_; j_ += 64) L.lens[j_] = 0;                                                        \
            LSYNC();                                                                                                               \
            uint32_t sym_ = 0, prev_ = 8, rep_ = 0, rlen_ = 0, sp_ = 32768;                                                       \
            while (sym_ < alpha_ && sp_ != 0) {                                                                                    \
                uint32_t cl_;                                                                                                      \
                READSYM(cl_, cltab);                                                                                               \
                if (cl_ < 16) {                                                                                                    \
                    rep_ = 0;                                                                                                      \
                    if (lane == 0) L.lens[sym_] = (uint8_t)cl_;                                                                    \
                    if (cl_ != 0) {                                                                                                \
                        prev_ = cl_;                                                                                               \
                        sp_ -= 32768u >> cl_;                                                                                      \
                    }                                                                                                              \
                    sym_++;                                                                                                        \
                } else {                                                                                                           \
                    const uint32_t xb_ = cl_ == 16 ? 2u : 3u;                                                                      \
                    const uint32_t nl_ = cl_ == 16 ? prev_ : 0u;                                                                   \
                    if (rlen_ != nl_) {                                                                                            \
                        rep_ = 0;                                                                                                  \
                        rlen_ = nl_;                                                                                               \
                    }                                                                                                              \
                    const uint32_t old_ = rep_;                                                                                    \
                    if (rep_ > 0) rep_ = (rep_ - 2) << xb_;                                                                        \
                    uint32_t e_;                                                                                                   \
                    GETBITS(e_, xb_);                                                                                              \
                    rep_ += e_ + 3;                                                                                                \
                    const uint32_t d_ = rep_ - old_;                                                                               \
                    if (sym_ + d_ > alpha_) FAIL(BE_HUFFMAN_SPACE);                                                                \
                    for (uint32_t j_ = lane; j_ < d_; j_ += 64) L.lens[sym_ + j_] = (uint8_t)rlen_;                                \
                    if (rlen_ != 0) sp_ -= d_ << (15 - rlen_);                                                                     \
                    sym_ += d_;                                                                                                    \
                }                                                                                                                  \
            }                                                                                                                      \
            if (sp_ != 0) FAIL(BE_HUFFMAN_SPACE);                                                                                  \
            LSYNC();                                                                                                               \
            size_ = build_table(t_, heap_cap - hp, L, alpha_);                                                                     \
            if (!size_) FAIL(ST_OVERFLOW);                                                                                         \
        }                                                                                                                          \
        tab_out = hp;                                                                                                              \
        if (advance) hp += size_;                                                                                                  \
    } while (0)

#define READ_VARLEN8(var)                 \
    do {                                  \
        uint32_t b_;                      \
        GETBITS(b_, 1);                   \
        if (!b_) {                        \
            var = 0;                          \
        } else {                          \
            uint32_t vn_;                 \
            GETBITS(vn_, 3);              \
            if (vn_ == 0) {               \
                var = 1;                  \
            } else {                      \
                uint32_t e_;              \
                GETBITS(e_, vn_);         \
                var = (1u << vn_) + e_;   \
            }                             \
        }                                 \
    } while (0)

    if (!resumed) {
        // WBITS (Section 9.1); the large-window marker is an error, as for a decoder without BROTLI_DECODER_PARAM_LARGE_WINDOW
        uint32_t b;
        GETBITS(b, 1);
        if (!b) {
            wbits = 16;
        } else {
            GETBITS(b, 3);
            if (b != 0) {
                wbits = 17 + b;
            } else {
                GETBITS(b, 3);
                if (b == 1) FAIL(BE_WINDOW_BITS);
                wbits = b != 0 ? 8 + b : 17;
            }
        }
    }
    {
        const uint32_t max_back = (1u << wbits) - 16u;
        for (;;) {
            // metablock boundary: the streaming checkpoint
            if (rs) {
                FENCE();
                if (lane == 0) {
                    rs[0] = 1u + (br.pos - B0);
                    rs[1] = opos;
                    for (int k = 0; k < 4; k++) rs[2 + k] = ring[(ridx + k) & 3];
                    rs[6] = wbits;
                    rs[7] = rsz;
                    rs[8] = 1u << wbits;
                    rs[9] = 0;
                }
            }
            uint32_t islast, mlen = 0, b;
            bool metadata = false, uncompressed = false;
            GETBITS(islast, 1);
            bool empty = false;
            if (islast) {
                GETBITS(b, 1);
                empty = b != 0;
            }
            if (!empty) {
                uint32_t nib;
                GETBITS(nib, 2);
                if (nib == 3) {
                    metadata = true;
                    GETBITS(b, 1);
                    if (b) FAIL(BE_RESERVED);
                    uint32_t nbytes;
                    GETBITS(nbytes, 2);
                    for (uint32_t i = 0; i < nbytes; i++) {
                        GETBITS(b, 8);
                        if (i + 1 == nbytes && nbytes > 1 && b == 0) FAIL(BE_EXUBERANT_META_NIBBLE);
                        mlen |= b << (8 * i);
                    }
                    if (nbytes) mlen++;
                } else {
                    const uint32_t nn = nib + 4;
                    for (uint32_t i = 0; i < nn; i++) {
                        GETBITS(b, 4);
                        if (i + 1 == nn && nn > 4 && b == 0) FAIL(BE_EXUBERANT_NIBBLE);
                        mlen |= b << (4 * i);
                    }
                    mlen++;
                    if (!islast) {
                        GETBITS(b, 1);
                        uncompressed = b != 0;
                    }
                }
            }
            if (metadata || uncompressed) {
                const uint32_t pad = (8u - (br.pos & 7u)) & 7u;
                if (pad) {
                    GETBITS(b, pad);
                    if (b) FAIL(BE_PADDING_1);
                }
            }
            if (metadata) {
                NEED(mlen * 8u);
                br.pos += mlen * 8u;
            }
            if (!metadata && mlen && rsz != (1u << wbits)) {
                const uint64_t need = dropped + opos + mlen;
                const uint64_t mn = need > (rsz ? rsz : 1024u) ? need : (rsz ? rsz : 1024u);
                uint32_t r = 1u << wbits;
                while ((r >> 1) >= mn) r >>= 1;
                rsz = r;
            }
            if (uncompressed) {
                const uint32_t avail = (br.end - br.pos) >> 3;
                const uint32_t room = cap - opos;
                const uint32_t n = mlen < avail ? mlen : avail;
                const uint32_t m = n < room ? n : room;
                const uint8_t *src = gin + ((br.pos - B0) >> 3);
                for (uint32_t j = lane; j < m; j += 64) gout[opos + j] = src[j];
                opos += m;
                br.pos += m * 8u;
                if (m < n || (m == room && m < mlen)) FAIL(CHIP_NEED_OUTPUT);
                if (n < mlen) FAIL(CHIP_NEED_INPUT);
            } else if (!metadata && mlen) {
                // ---- compressed metablock header (Section 9.2) ----
                uint32_t hp = 0;
                uint32_t nbl[3], btab[3] = {0, 0, 0}, ltab[3] = {0, 0, 0}, blen[3], rb_last[3] = {0, 0, 0}, rb_prev[3] = {1, 1, 1};
                for (int c = 0; c < 3; c++) {
                    uint32_t v;
                    READ_VARLEN8(v);
                    nbl[c] = v + 1;
                    blen[c] = 1u << 24;
                    if (nbl[c] >= 2) {
                        READ_CODE(nbl[c] + 2, btab[c], true);
                        READ_CODE(26u, ltab[c], true);
                        FENCE();
                        uint32_t sym, e;
                        READSYM(sym, heap + ltab[c]);
                        GETBITS(e, bt::BLOCK_LEN_EXTRA[sym]);
                        blen[c] = bt::BLOCK_LEN_BASE[sym] + e;
                    }
                }
                uint32_t v6;
                GETBITS(v6, 6);
                const uint32_t npostfix = v6 & 3u, ndirect = (v6 >> 2) << npostfix;
                for (uint32_t i = 0; i < nbl[0]; i++) {
                    uint32_t m;
                    GETBITS(m, 2);
                    if (lane == 0) modes[i] = (uint8_t)m;
                }
                uint32_t ntrees[3];
                ntrees[1] = nbl[1];
                // context maps (Section 7.3): literal then distance
                for (int which = 0; which < 2; which++) {
                    uint8_t *map = which == 0 ? lmap : dmap;
                    const uint32_t msize = (which == 0 ? 64u : 4u) * nbl[which == 0 ? 0 : 2];
                    uint32_t nt;
                    READ_VARLEN8(nt);
                    nt += 1;
                    ntrees[which == 0 ? 0 : 2] = nt;
                    if (nt <= 1) {
                        for (uint32_t j = lane; j < msize; j += 64) map[j] = 0;
                        continue;
                    }
                    uint32_t rlemax = 0;
                    GETBITS(b, 1);
                    if (b) {
                        GETBITS(rlemax, 4);
                        rlemax += 1;
                    }
                    uint32_t mtab;
                    READ_CODE(nt + rlemax, mtab, false);
                    FENCE();
                    uint32_t idx = 0;
                    while (idx < msize) {
                        uint32_t code;
                        READSYM(code, heap + mtab);
                        if (code == 0) {
                            if (lane == 0) map[idx] = 0;
                            idx++;
                        } else if (code > rlemax) {
                            if (lane == 0) map[idx] = (uint8_t)(code - rlemax);
                            idx++;
                        } else {
                            uint32_t e;
                            GETBITS(e, code);
                            const uint32_t reps = (1u << code) + e;
                            if (idx + reps > msize) FAIL(BE_CONTEXT_MAP_REPEAT);
                            for (uint32_t j = lane; j < reps; j += 64) map[idx + j] = 0;
                            idx += reps;
                        }
                    }
                    GETBITS(b, 1);
                    if (b) {  // inverse move-to-front, serial in lane 0
                        FENCE();
                        for (uint32_t j = lane; j < 256; j += 64) L.mtf[j] = (uint8_t)j;
                        LSYNC();
                        if (lane == 0) {
                            for (uint32_t j = 0; j < msize; j++) {
                                const uint32_t x = map[j];
                                const uint8_t val = L.mtf[x];
                                map[j] = val;
                                for (uint32_t k = x; k > 0; k--) L.mtf[k] = L.mtf[k - 1];
                                L.mtf[0] = val;
                            }
                        }
                        LSYNC();
                    }
                }
                // prefix codes of the three tree groups
                const uint32_t dalpha = 16u + ndirect + (48u << npostfix);
                const uint32_t alphas[3] = {256u, 704u, dalpha};
                for (int c = 0; c < 3; c++) {
                    for (uint32_t t = 0; t < ntrees[c]; t++) {
                        uint32_t off;
                        READ_CODE(alphas[c], off, true);
                        if (lane == 0) trees[256 * c + t] = off;
                    }
                }
                FENCE();

                // ---- commands (Section 10) ----
                remaining = (int32_t)mlen;
                uint32_t ltype = 0, itype = 0, dtype = 0;
                uint32_t mode = modes[0];
                const uint8_t *lut = bt::CONTEXT_LUT.v + 512u * mode;
                // literal trees of block type 0 by context
                if (lane < 64) L.lit_tree[lane] = trees[lmap[lane]];
                uint32_t itree = trees[256];
                LSYNC();
                uint32_t p1 = opos >= 1 ? gout[opos - 1] : 0u, p2 = opos >= 2 ? gout[opos - 2] : 0u;
                // block switch of category c (Section 6)
#define BLOCK_SWITCH(c, type)                                                     \
    do {                                                                          \
        if (nbl[c] < 2) FAIL(BE_UNREACHABLE); /* 2^24 symbols of one block type */ \
        uint32_t s_, e_;                                                          \
        READSYM(s_, heap + btab[c]);                                              \
        uint32_t ls_;                                                             \
        READSYM(ls_, heap + ltab[c]);                                             \
        GETBITS(e_, bt::BLOCK_LEN_EXTRA[ls_]);                                    \
        blen[c] = bt::BLOCK_LEN_BASE[ls_] + e_;                                   \
        uint32_t t_ = s_ == 1 ? rb_last[c] + 1 : s_ == 0 ? rb_prev[c] : s_ - 2;   \
        if (t_ >= nbl[c]) t_ -= nbl[c];                                           \
        rb_prev[c] = rb_last[c];                                                  \
        rb_last[c] = t_;                                                          \
        type = t_;                                                                \
    } while (0)
                for (;;) {
                    if (blen[1] == 0) {
                        BLOCK_SWITCH(1, itype);
                        itree = trees[256 + itype];
                    }
                    uint32_t cmd;
                    READSYM(cmd, heap + itree);
                    blen[1]--;
                    const uint32_t cell = cmd >> 6;
                    const uint32_t icode = bt::CMD_INSERT_CELL[cell] + ((cmd >> 3) & 7u);
                    const uint32_t ccode = bt::CMD_COPY_CELL[cell] + (cmd & 7u);
                    uint32_t e;
                    GETBITS(e, bt::INSERT_EXTRA[icode]);
                    const uint32_t ins = bt::INSERT_BASE[icode] + e;
                    GETBITS(e, bt::COPY_EXTRA[ccode]);
                    const uint32_t clen = bt::COPY_BASE[ccode] + e;
                    if (ins) {
                        remaining -= (int32_t)ins;
                        for (uint32_t i = 0; i < ins; i++) {
                            if (blen[0] == 0) {
                                BLOCK_SWITCH(0, ltype);
                                mode = modes[ltype];
                                lut = bt::CONTEXT_LUT.v + 512u * mode;
                                L.lit_tree[lane] = trees[lmap[64u * ltype + lane]];
                                LSYNC();
                            }
                            const uint32_t ctx = lut[p1] | lut[256 + p2];
                            uint32_t lit;
                            READSYM(lit, heap + L.lit_tree[ctx]);
                            blen[0]--;
                            // the literal that fills libbrotlidec's ring buffer makes it flush: past MLEN that fails
                            if (remaining < 0 && ((dropped + opos + 1) & (rsz - 1)) == 0) FAIL(BE_BLOCK_LENGTH_1);
                            if (opos >= cap) FAIL(CHIP_NEED_OUTPUT);
                            if (lane == 0) gout[opos] = (uint8_t)lit;
                            opos++;
                            p2 = p1;
                            p1 = lit;
                        }
                        if (remaining <= 0) break;
                    }
                    // distance
                    uint32_t dist;
                    bool push;
                    bool code0;
                    if (cmd < 128) {
                        dist = ring[(ridx - 1) & 3];
                        push = false;
                        code0 = true;
                    } else {
                        if (blen[2] == 0) BLOCK_SWITCH(2, dtype);
                        const uint32_t dctx = clen > 4 ? 3u : clen - 2;
                        const uint32_t dtree = trees[512 + dmap[4 * dtype + dctx]];
                        uint32_t dc;
                        READSYM(dc, heap + dtree);
                        blen[2]--;
                        code0 = dc == 0;
                        push = !code0;
                        if (dc < 16) {
                            // Section 4: last, 2nd, 3rd, 4th last, then last +-1..3 and 2nd last +-1..3
                            const uint32_t which = dc < 4 ? dc : dc < 10 ? 0u : 1u;
                            dist = ring[(ridx - 1 - which) & 3];
                            if (dc >= 4) {
                                const uint32_t k = dc < 10 ? dc - 4 : dc - 10;
                                const int32_t delta = (int32_t)(k >> 1) + 1;
                                const int32_t d = (k & 1) ? (int32_t)dist + delta : (int32_t)dist - delta;
                                dist = d <= 0 ? 0x7fffffffu : (uint32_t)d;
                            }
                        } else if (dc < 16 + ndirect) {
                            dist = dc - 15;
                        } else {
                            const uint32_t x = dc - ndirect - 16;
                            const uint32_t hcode = x >> npostfix, lcode = x & bmask(npostfix);
                            const uint32_t nb = 1 + (hcode >> 1);
                            const uint32_t offset = ((2u + (hcode & 1u)) << nb) - 4u;
                            GETBITS(e, nb);
                            dist = ((offset + e) << npostfix) + lcode + ndirect + 1;
                        }
                    }
                    const uint64_t total = dropped + opos;
                    const uint32_t max_dist = total < max_back ? (uint32_t)total : max_back;
                    FENCE();
                    if (dist > max_dist) {
                        // static dictionary reference (Section 8); the distance ring is left as it was
                        if (dist > 0x7ffffffcu) FAIL(BE_DISTANCE);
                        if (clen < 4 || clen > 24) FAIL(BE_DICTIONARY);
                        const uint32_t addr = dist - max_dist - 1;
                        const uint32_t shift = bt::DICT_NDBITS[clen];
                        const uint32_t widx = addr & bmask(shift), tidx = addr >> shift;
                        if (tidx >= (uint32_t)bt::NUM_TRANSFORMS) FAIL(BE_TRANSFORM);
                        const uint8_t *word = BROTLI_DICT + bt::DICT_OFFSET[clen] + widx * clen;
                        const bt::Transform &T = bt::TRANSFORMS[tidx];
                        const uint32_t type = T.type, plen = T.prefix_len, slen = T.suffix_len;
                        uint32_t skip = 0, wl = clen;
                        if (type >= 1 && type <= 9) wl = clen > type ? clen - type : 0;
                        if (type >= 12 && type <= 20) {
                            skip = type - 11;
                            wl = clen > skip ? clen - skip : 0;
                        }
                        if (lane < plen) L.wbuf[lane] = (uint8_t)T.prefix[lane];
                        if (lane < wl) L.wbuf[plen + lane] = word[skip + lane];
                        if (lane < 3) L.wbuf[plen + wl + lane] = 0;
                        LSYNC();
                        if (lane == 0 && wl) {
                            uint8_t *p = L.wbuf + plen;
                            if (type == 10) {
                                to_upper(p);
                            } else if (type == 11) {
                                int32_t left = (int32_t)wl;
                                while (left > 0) {
                                    const uint32_t step = to_upper(p);
                                    p += step;
                                    left -= (int32_t)step;
                                }
                            }
                        }
                        LSYNC();
                        if (lane < slen) L.wbuf[plen + wl + lane] = (uint8_t)T.suffix[lane];
                        LSYNC();
                        const uint32_t tl = plen + wl + slen;
                        remaining -= (int32_t)tl;
                        if (remaining < 0 && (((dropped + opos) & (rsz - 1)) + tl) >= rsz) FAIL(BE_BLOCK_LENGTH_1);
                        const uint32_t room = cap - opos;
                        const uint32_t m = tl < room ? tl : room;
                        if (lane < m) gout[opos + lane] = L.wbuf[lane];
                        const uint32_t op1 = p1;
                        if (m >= 1) p1 = L.wbuf[m - 1];
                        if (m >= 2) p2 = L.wbuf[m - 2]; else if (m == 1) p2 = op1;
                        opos += m;
                        if (m < tl) FAIL(CHIP_NEED_OUTPUT);
                    } else {
                        if (push) {
                            ring[ridx & 3] = dist;
                            ridx++;
                        }
                        (void)code0;
                        remaining -= (int32_t)clen;
                        if (remaining < 0 && (((dropped + opos) & (rsz - 1)) + clen) >= rsz) FAIL(BE_BLOCK_LENGTH_1);
                        if (dist > opos) FAIL(BE_UNREACHABLE);  // history a streaming caller dropped (never with the host's window)
                        const uint32_t room = cap - opos;
                        const uint32_t m = clen < room ? clen : room;
                        wave_back_copy(gout + opos, dist, m);
                        opos += m;
                        FENCE();
                        p1 = opos >= 1 ? gout[opos - 1] : 0u;
                        p2 = opos >= 2 ? gout[opos - 2] : 0u;
                        if (m < clen) FAIL(CHIP_NEED_OUTPUT);
                    }
                    if (remaining <= 0) break;
                }
#undef BLOCK_SWITCH
                if (remaining < 0) FAIL(BE_BLOCK_LENGTH_2);
                remaining = 1;
            }
            if (islast) {
                const uint32_t pad = (8u - (br.pos & 7u)) & 7u;
                if (pad) {
                    GETBITS(b, pad);
                    if (b) FAIL(BE_PADDING_2);
                }
                st = CHIP_FINISHED;
                break;
            }
        }
    }
done:
#undef NEED
#undef GETBITS
#undef READSYM
#undef FAIL
#undef READ_CODE
#undef READ_VARLEN8
    if (st == ST_OVERFLOW) return st;
    if (st == CHIP_NEED_INPUT && remaining < 0) st = BE_BLOCK_LENGTH_1;  // libbrotlidec flushes when the input runs out
    FENCE();
    if (rs && lane == 0 && st != CHIP_NEED_INPUT && st != CHIP_NEED_OUTPUT) rs[0] = 0;  // nothing to continue
    if (rs && lane == 0) rs[10] = rsz;  // the ring buffer size where the run stopped (what libbrotlidec could have flushed)
    if (lane == 0) {
        a.out_len[u] = opos;
        a.in_used[u] = st == CHIP_NEED_INPUT ? in_len : (((br.pos + 7u) >> 3) - (B0 >> 3));
        a.status[u] = st;
    }
    return st;
#undef FENCE
}

// pass 0: the batch (or a.sel) with SLOT_SMALL per wave, overflowing units appended to ovf; pass 1: the overflow list with
// SLOT_LARGE per wave.  ctr: [0] next unit of pass 0, [1] overflow count, [2] next unit of pass 1.
// Register budget of three waves per SIMD (168 VGPRs; four would spill 57 lane registers to scratch, unbounded 185 gives two)
__global__ __launch_bounds__(64, 3) void brotli_kernel(BatchArgs a, uint8_t *scratch, uint32_t slot_bytes, uint32_t *ctr, uint32_t *ovf,
                                                    uint32_t pass)
{
    __shared__ BLds L;
    Unit U;
    U.arena = scratch + (size_t)blockIdx.x * slot_bytes;
    U.slot_bytes = slot_bytes;
    const uint32_t count = pass == 0 ? (a.sel_n ? *a.sel_n : a.n) : ctr[1];
    for (;;) {
        uint32_t i = 0;
        if (lane_id() == 0) i = atomicAdd(&ctr[pass == 0 ? 0 : 2], 1u);
        i = rdfirst(i);
        if (i >= count) break;
        U.u = pass == 0 ? (a.sel ? a.sel[i] : i) : ovf[i];
        const int32_t st = decode_unit(a, U, L);
        if (st == ST_OVERFLOW && lane_id() == 0) {
            if (pass == 0) {
                ovf[atomicAdd(&ctr[1], 1u)] = U.u;
            } else {  // cannot happen with SLOT_LARGE; answered rather than left
                a.out_len[U.u] = 0;
                a.in_used[U.u] = 0;
                a.status[U.u] = BE_UNREACHABLE;
            }
        }
        WSYNC();
    }
}

// per-wave slots, the overflow list and the counters: a launch slot ("Launch slots")
struct BSlot {
    uint8_t *small = nullptr;
    uint8_t *large = nullptr;
    uint32_t *ctr = nullptr;  // 4 counters, then the overflow list
    int blocks = 0;
    uint32_t large_blocks = 0;
    size_t list_n = 0;
    void free()
    {
        (void)hipFree(small);
        (void)hipFree(large);
        (void)hipFree(ctr);
    }
    size_t bytes() const { return (size_t)blocks * SLOT_SMALL + (size_t)large_blocks * SLOT_LARGE + (4 + list_n) * sizeof(uint32_t); }
};
SlotCache<BSlot> g_br_cache;
ResidentWaves g_br_resident;

// (caller holds g_br_cache.mu) room for a batch of n units
hipError_t bslot_reserve(BSlot &sl, hipStream_t stream, uint32_t n)
{
    int max_blocks = 0;
    hipError_t e = g_br_resident.get((const void *)brotli_kernel, max_blocks, 16);  // bounds the small slots at 16 * CUs * 128 KiB
    if (e != hipSuccess) return e;
    const int want = n < (uint32_t)max_blocks ? (int)n : max_blocks;
    const uint32_t want_large = n < LARGE_BLOCKS ? n : LARGE_BLOCKS;  // a streaming decoder (n = 1) keeps one large slot
    if (sl.blocks < want || sl.list_n < n || sl.large_blocks < want_large) {
        if ((sl.small || sl.large) && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;  // launches on the stream still use them
        sl.free();
        const uint32_t old_large = sl.large_blocks;
        sl = BSlot{};
        const int blocks = grown_blocks(want, max_blocks);
        const size_t list_n = n < 1024 ? 1024 : (size_t)n;
        if ((e = hipMalloc((void **)&sl.small, (size_t)blocks * SLOT_SMALL)) != hipSuccess) return e;
        const uint32_t large_blocks = want_large > old_large ? want_large : old_large;
        if ((e = hipMalloc((void **)&sl.large, (size_t)large_blocks * SLOT_LARGE)) != hipSuccess) return e;
        if ((e = hipMalloc((void **)&sl.ctr, (4 + list_n) * sizeof(uint32_t))) != hipSuccess) return e;
        sl.blocks = blocks;
        sl.large_blocks = large_blocks;
        sl.list_n = list_n;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_brotli_decode(const BatchArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    std::lock_guard<std::mutex> lk(g_br_cache.mu);  // from the slot's lookup to the last launch
    BSlot *sl = nullptr;
    hipError_t e = g_br_cache.at(stream, sl);
    if (e == hipSuccess) e = bslot_reserve(*sl, stream, a.n);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(sl->ctr, 0, 16, stream)) != hipSuccess) return e;
    const uint32_t blocks = a.n < (uint32_t)sl->blocks ? a.n : (uint32_t)sl->blocks;
    hipLaunchKernelGGL(brotli_kernel, dim3(blocks), dim3(64), 0, stream, a, sl->small, SLOT_SMALL, sl->ctr, sl->ctr + 4, 0u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t lb = a.n < sl->large_blocks ? a.n : sl->large_blocks;
    hipLaunchKernelGGL(brotli_kernel, dim3(lb), dim3(64), 0, stream, a, sl->large, SLOT_LARGE, sl->ctr, sl->ctr + 4, 1u);
    return hipGetLastError();
}

size_t brotli_scratch_bytes_of(hipStream_t stream) { return g_br_cache.bytes_of(stream); }

}  // namespace chip
