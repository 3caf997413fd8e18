#pragma once
// The device code of the batched DEFLATE inflate for gfx950 (MI355X): one wavefront decodes one independent unit (inflate_unit).
// Included by the translation units that hold the kernels: inflate.hip, inflate_sizes.hip, inflate_members.hip, inflate_index.hip.
//
// Replaces, per unit, what compu reaches through sys::inflate (src/decoder/mod.rs:470) for a
// decoder built by Interface::zlib_ng(mode) (src/decoder/zlib_ng.rs:61-90): block-header parse,
// dynamic-Huffman table build, bitstream decode, LZ77 copy (RFC 1951), and the zlib / gzip
// wrappers with Adler-32 / CRC-32 verification (RFC 1950 / 1952).
//
// Data flow per wave (inflate_kernel):  block header --> canonical-Huffman tables in LDS (two-level, see below)
//   --> per block a sequence of SUPER-ROUNDS.  A super-round stages the next 64 x 320 bits of input in LDS (coalesced dword loads)
//   from the true token boundary B on; lane i decodes the token chain that starts at B + 320 i (a guess, except for lane 0), marks
//   the token boundaries it passes inside its own 320-bit segment in a bit map of the staged input, and keeps going past the
//   segment's end until it steps on a boundary marked by the owner of the segment it is in (from there on the two chains are the
//   same), at most 1536 bits further (3072 in fixed-Huffman blocks).  Tokens (literal | length, distance) go to the lane's row of
//   the wave's scratch in HBM / L2, 16 bytes per four tokens.  The chain of joins from lane 0 is the true token stream; it is found
//   in registers (pointer doubling with ds_bpermute) and executed a chunk (<= 2.5 KB of output) at a time: 64 tokens per step
//   fetched through an LDS-DMA ring, output offsets by wave prefix sum, literals and queued matches assembled in LDS and stored
//   coalesced into the unit's output range in HBM (the LZ77 window is the output itself).
// The grid is persistent: waves take units from a counter, so the token scratch is one slot per resident wave.
#include "chip_internal.h"
#include "wave_checksums.h"

namespace chip {

// pointers into HBM keep their address space through the scalar round trip of rdfirst_ptr (else every access through them is a
// flat one: slower, and counted as an LDS access too)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));  // at any byte address (gfx950 takes any alignment for global and LDS accesses)
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));
template <typename T>
__device__ __forceinline__ GAS T *rdfirst_gptr(T *p)
{
    return (GAS T *)rdfirst_ptr(p);
}

// phases of a unit's work: always inlined into the kernel (LDS accesses through a WaveLds reference become flat accesses in an
// out-of-line function: measured 25 % slower in round 2)
#ifndef CHIP_PHASE_FN
#define CHIP_PHASE_FN __attribute__((always_inline))
#endif

// The two variants of the parallel decode of one stream (inflate_parallel.hip, inflate_parallel_markers.hip),
// compiled only there, as the member loop and the index recording are: without the macros this file's tokens are what they were.
// CHIP_INFLATE_SPEC: the speculative size pass.  Unit u >= 1 begins at a block start the finder named, without a wrapper; a match
// may reach in front of the unit's first byte (how far is recorded, not refused); at every block boundary the unit looks for the
// boundary in the sorted list of starts behind its own and ends there, LINKED to that start.
// CHIP_INFLATE_MARKERS: the marker decode.  The unit begins at a bit offset like a resumed one and its output is 16-bit elements:
// literals 0 .. 255, and 0x8000 | j for the byte j of the 32 768 in front of the unit's first, which nobody knows yet.
#ifndef CHIP_INFLATE_SPEC
#define CHIP_INFLATE_SPEC 0
#endif
#ifndef CHIP_INFLATE_MARKERS
#define CHIP_INFLATE_MARKERS 0
#endif
#if CHIP_INFLATE_SPEC
#define SPEC_PARAM , uint32_t &sp_reach
#define SPEC_ARG , sp_reach
#else
#define SPEC_PARAM
#define SPEC_ARG
#endif

// Diagnostic build (-DCHIP_STATS): per-unit cycle and event counters; compiled out of the product.
#ifdef CHIP_STATS
#define STAT_DECL unsigned long long st_[24] = {0}; unsigned long long st_t0_ = 0
#define STAT_T0() (st_t0_ = __builtin_readcyclecounter())
#define STAT_ACC(i) do { unsigned long long n_ = __builtin_readcyclecounter(); st_[i] += n_ - st_t0_; st_t0_ = n_; } while (0)
#define STAT_ADD(i, v) (st_[i] += (unsigned long long)(v))
#define STAT_PARAM , unsigned long long *st_, unsigned long long &st_t0_
#define STAT_ARG , st_, st_t0_
#else
#define STAT_DECL
#define STAT_T0()
#define STAT_ACC(i)
#define STAT_ADD(i, v)
#define STAT_PARAM
#define STAT_ARG
#endif
// stat slots (cycles): 0 other header work, 1 walk set-up (first window chunks), 2 walk, 3 path resolve, 4 code lengths (+ block
// header), 5 table build, 6 checksum/trailer, 16 token groups (fetch, placement,
// literals, match queue), 17 match rounds, 18 chunk store, 20 rest of the flush; (counts): 8 walk rounds (macro-rounds), 9 pieces
// on the path, 10 tokens, 11 walk trips (8 tokens each), 12 parallel copy passes, 13 chunks, 14 match rounds, 15 matches
// copied by the whole wave, 21 lane-tokens decoded by the walk; block headers: 7 rounds of the code-length loop, 19 passes of the
// counting sort, 22 / 23 trips of the literal/length / distance sub-table fill

// ---- code-length alphabet: table entry format of round 1 (one level, 7-bit root) --------------------
// [3:0] code length, [31:16] symbol
enum : uint32_t { K_LIT = 0, K_LEN = 1, K_EOB = 2, K_BAD = 3 };
__device__ __forceinline__ constexpr uint32_t mk_entry(uint32_t cl, uint32_t eb, uint32_t kind, uint32_t base)
{
    return cl | (eb << 4) | (kind << 8) | (base << 16);
}

constexpr int LIT_ROOT = 9;
constexpr int DIST_ROOT = 8;
constexpr int CL_ROOT = 7;

// ---- literal/length and distance tables ------------------------------------------------------------
// Literal/length codes are always looked up in two steps, without a branch (with a 9-bit root 11 % of this
// workload's tokens have longer codes, so among 64 lanes the long path ran at every step anyway):
//   lit_root[next 9 bits] (16 bits) = [4:0] number of further index bits nb, [15:5] index in pool[] of the code's
//   entry (nb = 0) or of its prefix's sub-table (2^nb entries, indexed by the nb bits behind the root's nine);
//   pool[] entry (32 bits, "final"): [4:0] code length cl, [9:5] number of extra bits eb, [14:10] cl + eb,
//   [15] halt (end of block, or with [26]: invalid code), [25:16] value as the token wants it (literal byte, or 512 + length
//   base 3..258: the token's match bit comes with the base), [31] length code.  The fields sit where v_bfe_u32 /
//   v_alignbit_b32 read their 5-bit offset and width operands.  A root entry's [15:3] is the byte offset of the pool entry or
//   sub-table as it stands (nb is below 8, the offset a multiple of 4).
// Distance codes: dist_root[next 8 bits] (16 bits) is the final entry for codes of up to 8 bits (99 % of matches):
//   [3:0] code length, [7:4] number of extra bits, [9:8] mantissa (distance - 1 = mantissa << extra bits, plus the extra
//   bits' value), [10] invalid code, [15] longer code: then [3:0] is the number of further index bits and [11:3] the byte
//   offset of a sub-table of such entries from DIST_SUB_BYTES on (the sub-tables lie in the top 256 16-bit units of pool[],
//   and each starts at an even unit).
constexpr uint32_t F_HALT = 1u << 15, F_INV = 1u << 26, F_LEN = 1u << 31;
constexpr uint32_t D_BAD = 1u << 10, D_LONG = 1u << 15;
static_assert(15 - LIT_ROOT < 8 && 15 - DIST_ROOT < 8, "a root entry's index bit count leaves its bits [4:3] clear");
static_assert((2u << (15 - DIST_ROOT)) - 2u < 256u, "the distance sub-tables fit the 256 units that a root entry's offset spans");

__device__ __forceinline__ uint32_t make_final(uint32_t sym, uint32_t len)
{
    if (sym < 256) return len | (len << 10) | (sym << 16);
    if (sym == 256) return len | (len << 10) | F_HALT;
    if (sym >= 286) return len | (len << 10) | F_HALT | F_INV;
    const uint32_t s = sym - 257;
    uint32_t eb = 0, base = 3 + s;
    if (s == 28) base = 258;
    else if (s >= 8) {
        eb = (s >> 2) - 1;
        base = 3 + ((4 + (s & 3)) << eb);
    }
    return len | (eb << 5) | ((len + eb) << 10) | ((512u | base) << 16) | F_LEN;
}
__device__ __forceinline__ uint32_t make_dist16(uint32_t sym, uint32_t len)
{
    if (sym >= 30) return len | D_BAD;
    if (sym < 4) return len | (sym << 8);
    return len | (((sym >> 1) - 1) << 4) | ((2 + (sym & 1)) << 8);
}

// ---- geometry of the speculative wave-parallel walk --------------------------------------------------
// Per super-round lane i walks the token chain that starts at B + i*S_BITS (a guess, except for lane 0), marks the token
// boundaries it passes inside its own segment in a bit map of the staged input (one mark bit per input bit), and keeps walking
// past its segment until it steps on a boundary marked by the owner of the segment it is in (from there on the two chains are
// the same), at most XT_BITS further.  Every lane records up to ROW_TOKENS tokens.  S_BITS is an odd number of dwords so that
// the 64 lanes' first window reads hit distinct LDS banks.
#ifndef CHIP_S_BITS  // geometry overridable for experiments (round 4: 320-bit segments and 2.5 KB chunks let 18 waves per CU in, 8960 B of LDS
                     // each; at the full 65 536-unit launch that is 14.6 ms against 15.1 for 384 bits / 3.5 KB at 16 waves, 15.6 for this geometry at 16,
                     // 15.5 at 17 waves with 352 bits, 15.3 at 19 with 288, 15.9 at 20 with 224 -- DESIGN.md sec. 8)
#define CHIP_S_BITS 320
#define CHIP_XT_BITS 1536
#define CHIP_XT_BITS_FIXED 3072  // fixed-Huffman codes (nearly all 8 or 9 bits) fall into step slowly
#define CHIP_ROW_TOKENS 256
#endif
constexpr uint32_t S_BITS = CHIP_S_BITS;
constexpr uint32_t XT_BITS = CHIP_XT_BITS;
#ifndef CHIP_XT_BITS_FIXED
#define CHIP_XT_BITS_FIXED CHIP_XT_BITS
#endif
constexpr uint32_t XT_BITS_FIXED = CHIP_XT_BITS_FIXED;
constexpr uint32_t ROW_TOKENS = CHIP_ROW_TOKENS;
static_assert(S_BITS % 32 == 0 && ROW_TOKENS % 4 == 0 && 64 * ROW_TOKENS < 65536, "geometry");
constexpr uint32_t SEG_WORDS = S_BITS / 32 + 1;  // mark words a segment can touch
// x / S_BITS for x < 2^15 (bit offsets inside a super-round) as a multiply and a shift
constexpr uint32_t SEG_SHIFT = 24;  // (exact for every geometry tried: 224 .. 384-bit segments; checked below)
constexpr uint32_t SEG_MAGIC = ((1u << SEG_SHIFT) + S_BITS - 1) / S_BITS;
constexpr bool seg_magic_ok()
{
    for (uint32_t x = 0; x < 64u * S_BITS + 4096u; x++)
        if (((x * SEG_MAGIC) >> SEG_SHIFT) != x / S_BITS) return false;
    return true;
}
static_assert(seg_magic_ok() && (64u * S_BITS + 4096u) * (uint64_t)SEG_MAGIC < (1ull << 32), "segment index by multiplication");
constexpr uint32_t WIN_DW = (31 + 64 * S_BITS + 48 + 96 + 31) / 32 + 3;  // staged input of a super-round, dwords
constexpr uint32_t HDR_IN_DW = 192;    // input window of the block-header parser, dwords (the code lengths take <= 4584 bits)

// Scratch of a wave in HBM: the lanes' token rows.  Layout: a 128-byte line holds four tokens (one 16-byte store) of each of eight neighbouring lanes, so that one
// store instruction of the walk fills whole lines (lane l, row token k = 4q + j -> word rowbase(l) + 32 q + j with
// rowbase(l) = (l / 8) * 8 * ROW_TOKENS + (l % 8) * 4).
constexpr size_t ROWS_WORDS = (size_t)64 * ROW_TOKENS;
static_assert(64ull * ROW_TOKENS * 258 < (1ull << 32), "count_tokens() sums a super-round's output lengths in 32 bits");
__device__ __forceinline__ uint32_t row_base(uint32_t l) { return (l >> 3) * (8u * ROW_TOKENS) + (l & 7u) * 4u; }
__device__ __forceinline__ uint32_t row_word(uint32_t k) { return k + (k >> 2) * 28u; }  // 32 * (k / 4) + k % 4

// token: [8:0] literal byte, or match length 3..258; [9] match; [25:10] match distance - 1 (a piece's entry token in a joined lane's
// row is found from the popcount of the owner's boundary marks, not from the tokens).  A literal token may carry the literal behind
// it as well (a pair): [31] set, [23:16] the second byte (where a byte store of the register's high half reads it); a match has
// bit 31 clear.  tok_olen() is a token's output length for the code that reads tokens from the rows one by one (count_tokens(),
// overflow_bit()); flush_tokens() forms the same value from the fields it has already taken apart.
__device__ __forceinline__ uint32_t tok_olen(uint32_t t) { return (t & 512u) ? t & 0x1ffu : 1u + (t >> 31); }

struct HuffMeta {
    uint32_t limit15[16];  // [l] = end (exclusive) of the 15-bit-aligned code space of lengths <= l; [0] = 0
    uint32_t offs[16];     // [l] = index in sorted[] of the first symbol of length l
    uint32_t maxlen;
};

// LZ77 execution state of a chunk (see below)
#ifndef CHIP_CHUNK_BYTES
#define CHIP_CHUNK_BYTES 2560
#endif
#ifndef CHIP_COPY_LANE_MAX
#define CHIP_COPY_LANE_MAX 32
#endif
constexpr uint32_t CHUNK_BYTES = CHIP_CHUNK_BYTES;
constexpr uint32_t COPY_LANE_MAX = CHIP_COPY_LANE_MAX;
constexpr uint32_t MQ_CAP = 128;  // queued matches: at most 63 left over + 64 new
constexpr uint32_t IMG_WORDS = CHUNK_BYTES / 4 + 8;  // + room for the 16-byte reads that run past a source's end
constexpr uint32_t TOK_RING = 4;   // token groups on their way from the scratch rows into LDS (LDS-DMA: no registers held)
static_assert(CHUNK_BYTES % 4 == 0 && CHUNK_BYTES >= 1024 && COPY_LANE_MAX % 16 == 0 && IMG_WORDS % 2 == 0, "geometry");

constexpr uint32_t FLUSH_BYTES = 4 * (IMG_WORDS + 2 * MQ_CAP + 64 * TOK_RING + 128 + 4);
constexpr uint32_t HDR_BYTES = 4 * HDR_IN_DW + 4 * (1 << CL_ROOT) + 80 + sizeof(HuffMeta) + 64 + 320 + 2 * 288 + 2 * 32 + 2 * sizeof(HuffMeta);
constexpr uint32_t PHASE_BYTES = 8 * WIN_DW > FLUSH_BYTES ? (8 * WIN_DW > HDR_BYTES ? 8 * WIN_DW : HDR_BYTES) : (FLUSH_BYTES > HDR_BYTES ? FLUSH_BYTES : HDR_BYTES);
#ifndef CHIP_LDS_BYTES
#define CHIP_LDS_BYTES 8960  // per wave: 18 waves per CU (the occupancy query: 16 at 10240 B, 17 at 9600, 19 at 8448, 20 at 8192; CHIP_DEBUG_GRID prints it in the CHIP_STATS build)
#endif
constexpr uint32_t POOL_WORDS = (CHIP_LDS_BYTES - 2 * 512 - 2 * 256 - PHASE_BYTES) / 4;
constexpr uint32_t POOL_U16 = 2 * POOL_WORDS;
constexpr uint32_t DIST_SUB_BYTES = 2 * (POOL_U16 - 256);  // byte offset in pool[] that a long distance code's root entry counts from

struct alignas(16) WaveLds {
    union {  // first: the walk's window reads (ds_read2_b32) take small offsets only
        struct {                             // walk
            uint32_t win[WIN_DW];            // input dwords from the super-round's first on
            uint32_t bm[WIN_DW];             // mark bits, one per input bit
        } w;
        struct {                             // block header and table build
            uint32_t inbuf[HDR_IN_DW];
            uint32_t cl_lut[1 << CL_ROOT];
            uint32_t cl_sorted[20];
            HuffMeta cl_h;
            uint32_t count[16];
            uint8_t lens[320];
            uint16_t lit_sorted[288];        // symbols in canonical order
            uint16_t dist_sorted[32];
            HuffMeta lit_h, dist_h;
        } hdr;
        struct {                             // LZ77 execution
            uint32_t out[IMG_WORDS];         // the chunk's output bytes by offset (offset 0 = the dword-aligned address below the chunk)
            uint2 mq[MQ_CAP];                // queued match: .x offset of its first output byte, .y length | distance << 16
            uint32_t tok[64 * TOK_RING];     // token groups, written by global_load_lds_dword
            uint32_t pk[128];                // k-th piece of a batch: [2k] its first stream index, [2k+1] [15:0] (row token - stream index) mod 2^16, [31:16] row base
            uint32_t trash[4];               // where the stores of lanes that have nothing to store go (never read)
        } fl;
        uint32_t phase_words_[PHASE_BYTES / 4];
    };
    uint16_t lit_root[1 << LIT_ROOT];
    uint16_t dist_root[1 << DIST_ROOT];
    uint32_t pool[POOL_WORDS];  // literal/length finals and sub-tables from the bottom, distance sub-tables (16-bit) from the top
};
static_assert(sizeof(WaveLds) <= CHIP_LDS_BYTES, "the waves per CU that CHIP_LDS_BYTES stands for");
// pool[] cannot overflow.  In a canonical code the codes of one length are neighbours, so every 9-bit prefix that lies inside the codes
// of length L > 9 has a sub-table of 2^(L-9) entries, one per code; only the (at most one per length) prefixes that straddle two lengths
// hold entries that repeat a code.  Literal/length: <= 286 codes + 1 invalid entry + (2 + 4 + ... + 64) = 413 words; distance (16-bit
// entries, 8-bit root): <= 30 + (2 + 4 + ... + 128) = 284 entries = 142 words.
static_assert(POOL_WORDS >= 413 + 142, "the tables of any valid block fit");
// the CRC-32 tables (2048 words) take the whole structure: nothing else is live while a checksum runs
#ifndef CHIP_EXP_ALLOW_SMALL_LDS  // (timing probes of raw-deflate batches only: gzip units would run over the structure)
static_assert(sizeof(WaveLds) >= 2048 * 4, "wave_crc32 needs 8 KB");
#endif

// Canonical lookup: x15 = next 15 stream bits, first bit in bit 14 (MSB-first code value).  Returns the symbol's index in
// sorted[] (0xffffffff: no such code) and its length.
__device__ __forceinline__ uint32_t canon_index(const HuffMeta &H, uint32_t x15, uint32_t &l)
{
    l = 1;
    if (x15 >= H.limit15[15]) return 0xffffffffu;
#pragma unroll
    for (int j = 1; j < 15; j++) l += (x15 >= H.limit15[j]) ? 1u : 0u;
    return H.offs[l] + ((x15 - H.limit15[l - 1]) >> (15 - l));
}

// The same with the limits in scalar registers (read once per table build) and the code's length known to lie in [LO, HI]: the root
// fill knows x15 < limit15[ROOT] (lengths up to ROOT), a sub-table knows x15 >= limit15[ROOT] (lengths above it), so eight or five
// comparisons against registers stand where fourteen LDS reads and comparisons stood.
struct CanonLim {
    uint32_t lim[16];
};
__device__ __forceinline__ CanonLim canon_limits(const HuffMeta &H)
{
    CanonLim c;
#pragma unroll
    for (int j = 0; j < 16; j++) c.lim[j] = rdfirst(H.limit15[j]);
    return c;
}
template <int LO, int HI>
__device__ __forceinline__ uint32_t canon_index_in(const HuffMeta &H, const CanonLim &c, uint32_t x15, uint32_t &l)
{
    l = LO;
#pragma unroll
    for (int j = LO; j < HI; j++) l += (x15 >= c.lim[j]) ? 1u : 0u;
    return H.offs[l] + ((x15 - H.limit15[l - 1]) >> (15 - l));
}

// Code lengths -> canonical description H and the symbols in canonical order (RFC 1951 sec. 3.2.2), with zlib's acceptance
// rules.  Wave-cooperative; lens[], count[] live in LDS.  Returns 0, -1 (invalid set) or 1 (empty set); uniform.
template <typename SortedT, typename MakeT>
__device__ __forceinline__ int canon_prep(uint32_t *count, const uint8_t *lens, int n_, bool code_lengths, SortedT *sorted, HuffMeta &H, MakeT make STAT_PARAM)
{
    const uint32_t lane = lane_id();
    const int n = (int)rdfirst((uint32_t)n_);
    if (lane < 16) count[lane] = 0;
    WSYNC();
    for (int s = lane; s < n; s += 64) {
        uint32_t l = lens[s];
        if (l) atomicAdd(&count[l], 1u);
    }
    WSYNC();
    // Lane l (1..15) holds the count of length l.  offs[l] = symbols of shorter lengths; limit15[l] = sum over j <= l of
    // count[j] << (15 - j): the end of the code space that lengths <= l take, aligned to 15 bits.  zlib's running `left` is
    // (2^15 - limit15[l]) >> (15 - l): the set is over-subscribed when some limit15[l] exceeds 2^15 and incomplete when
    // limit15[15] stays below it.  (Two wave prefix sums instead of a 15-step chain of LDS reads and scalar updates.)
    const uint32_t c = lane >= 1 && lane <= 15 ? count[lane] : 0u;
    const uint32_t cincl = wave_incl_scan(c);
    const uint32_t off = cincl - c;
    const uint32_t lim = wave_incl_scan(lane <= 15 ? c << (15u - (lane & 15u)) : 0u);
    const uint32_t present = (uint32_t)__ballot(c != 0);
    const uint32_t maxlen = present ? 31u - (uint32_t)__clz((int)present) : 0u;
    const bool over = __any(lane <= 15 && lim > 32768u);
    const int left = rdlane(lim, 15) < 32768u ? 1 : 0;
    if (lane <= 15) {
        H.limit15[lane] = lim;
        H.offs[lane] = off;
        count[lane] = off;  // from here on: the place in sorted[] of the next symbol of length `lane`
    }
    if (lane == 0) H.maxlen = maxlen;
    WSYNC();
    if (maxlen == 0) return 1;
    if (over) return -1;
    if (left > 0 && (code_lengths || maxlen != 1)) return -1;
    // stable counting sort by (length, symbol), 64 symbols per pass.  `same` = the lanes whose length equals this lane's: four
    // ballots, one per bit of the length, each taken as it stands or complemented.  The lane's rank among them is its place
    // behind count[l]; the last lane of each length moves count[l] on for the next pass.
    for (int base = 0; base < n; base += 64) {
        STAT_ADD(19, 1);
        const int s = base + (int)lane;
        const uint32_t l = s < n ? lens[s] : 0;
        uint64_t same = ~0ull;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            const bool bit = (l >> b) & 1u;
            const uint64_t m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
        const uint32_t cnt = (uint32_t)__popcll(same);
        const uint32_t at = count[l];
        if (l) sorted[at + rank] = make((uint32_t)s, l);
        if (l && rank + 1u == cnt) count[l] = at + cnt;
        LSYNC();
    }
    WSYNC();
    return 0;
}

// The code-length alphabet's one-level table (zlib: a set made only of zeros reads as symbol 0 of length 1).
__device__ CHIP_PHASE_FN int build_cl_table(WaveLds &L STAT_PARAM)
{
    const uint32_t lane = lane_id();
    HuffMeta &H = L.hdr.cl_h;
    const int r = canon_prep(L.hdr.count, L.hdr.lens, 19, true, L.hdr.cl_sorted, H, [](uint32_t s, uint32_t l) { return mk_entry(l, 0, K_LIT, s); } STAT_ARG);
    if (r < 0) return -1;
    const CanonLim CL = canon_limits(H);
    for (uint32_t idx = lane; idx < (1u << CL_ROOT); idx += 64) {
        uint32_t e = mk_entry(1, 0, K_LIT, 0);
        if (r == 0) {
            uint32_t l;
            const uint32_t x15 = __brev(idx) >> 17;  // codes are at most 7 bits: the root covers them all
            const uint32_t ci = canon_index_in<1, CL_ROOT>(H, CL, x15 < CL.lim[15] ? x15 : 0u, l);
            e = x15 < CL.lim[15] ? L.hdr.cl_sorted[ci] : mk_entry(rdfirst(H.maxlen), 0, K_BAD, 0);
        }
        L.hdr.cl_lut[idx] = e;
    }
    WSYNC();
    return 0;
}

// Sub-table fill: one entry per lane and trip over the concatenation of a batch's sub-tables (`total` entries, flat index f).  A
// lane that holds a root prefix (have) owns the 2^sb entries from flat index `start` on.  Per trip of 64 flat indices every
// prefix that begins in the trip, or runs into it from the trip before, drops a head word (lane + 1, start, sb) at its first
// index of the trip in heads[] (64 words of LDS); a running maximum hands every index the head in front of it, its owner's.
// put(f, p, t, sb): flat index f is entry t of lane p's sub-table of 2^sb entries.
static_assert(POOL_U16 <= 0x2000u, "a head word holds a flat index in 13 bits");
template <typename PutT>
__device__ __forceinline__ void fill_flat(uint32_t *heads, bool have, uint32_t sb, uint32_t start, uint32_t total, PutT put)
{
    const uint32_t lane = lane_id();
    const uint32_t end = have ? start + (1u << sb) : 0u;
    const uint32_t head = ((lane + 1u) << 16) | (start << 3) | sb;  // start < 2^13 (POOL_U16), sb < 8
    for (uint32_t f0 = 0; f0 < total; f0 += 64) {
        heads[lane] = 0;
        if (end > f0 && start < f0 + 64u) heads[start > f0 ? start - f0 : 0u] = head;
        LSYNC();
        const uint32_t h = wave_incl_max_scan(heads[lane]);
        LSYNC();  // (the next trip's stores stay behind this read)
        const uint32_t f = f0 + lane;
        if (f < total) put(f, (h >> 16) - 1u, f - ((h >> 3) & 0x1fffu), h & 7u);
    }
}

// Literal/length tables of a block from lens[0..n).  Returns 0, -1 (invalid set), or 1 (the codes' entries do not fit pool[]: cannot
// happen, see POOL_WORDS).  `used` = words of pool[] taken.
__device__ CHIP_PHASE_FN int build_litlen(WaveLds &L, const uint8_t *lens, int n, uint32_t &used STAT_PARAM)
{
    const uint32_t lane = lane_id();
    HuffMeta &H = L.hdr.lit_h;
    uint16_t *const sorted = L.hdr.lit_sorted;
    const int r = canon_prep(L.hdr.count, lens, n, false, sorted, H, [](uint32_t s, uint32_t) { return (uint16_t)s; } STAT_ARG);
    if (r != 0) return -1;  // no literal/length code at all cannot be: the end-of-block code exists
    const CanonLim CL = canon_limits(H);
    const uint32_t lim_r = CL.lim[LIT_ROOT], top = CL.lim[15];
    const uint32_t nshort = rdfirst(H.offs[LIT_ROOT + 1 <= 15 ? LIT_ROOT + 1 : 15]);  // symbols with codes of up to nine bits come first
    const uint32_t nsym = rdfirst(L.hdr.count[15]);  // where the sort's place for 15-bit codes ended: behind the last symbol
    const uint32_t nfirst = rdfirst(H.maxlen) <= (uint32_t)LIT_ROOT ? nsym : nshort;
    if (nfirst + 1 > POOL_WORDS) return 1;
    for (uint32_t i = lane; i < nfirst; i += 64) {
        const uint32_t s = sorted[i];
        L.pool[i] = make_final(s, lens[s]);
    }
    const uint32_t bad_idx = nfirst;
    const uint32_t bad_e = rdfirst(H.maxlen) | (rdfirst(H.maxlen) << 10) | F_HALT | F_INV;
    if (lane == 0) L.pool[bad_idx] = bad_e;
    for (uint32_t idx = lane; idx < (1u << LIT_ROOT); idx += 64) {
        const uint32_t x15 = __brev(idx) >> 17;
        if (x15 >= top) L.lit_root[idx] = (uint16_t)(bad_idx << 5);
        else if (x15 < lim_r) {
            uint32_t l;
            L.lit_root[idx] = (uint16_t)(canon_index_in<1, LIT_ROOT>(H, CL, x15, l) << 5);
        }
    }
    used = nfirst + 1;
    if (top > lim_r) {
        // sub-tables: one per root prefix that holds longer codes; the longest code of a prefix is its last one
        constexpr uint32_t P = 1u << (15 - LIT_ROOT);
        const uint32_t np = (top - lim_r + P - 1) / P;
        for (uint32_t j0 = 0; j0 < np; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool have = j < np;
            const uint32_t xj = lim_r + j * P;
            uint32_t sb = 0;
            if (have) {
                uint32_t l;
                (void)canon_index_in<LIT_ROOT + 1, 15>(H, CL, xj + P < top ? xj + P - 1 : top - 1, l);
                sb = l - LIT_ROOT;
            }
            const uint32_t size = have ? (1u << sb) : 0u;
            const uint32_t incl = wave_incl_scan(size);
            const uint32_t off = used + incl - size;
            const uint32_t total = rdlane(incl, 63);
            if (used + total > POOL_WORDS) return 1;
            STAT_ADD(22, (total + 63u) / 64u);
            if (have) L.lit_root[__brev(xj >> (15 - LIT_ROOT)) >> (32 - LIT_ROOT)] = (uint16_t)((off << 5) | sb);
            fill_flat(L.hdr.cl_lut, have, sb, incl - size, total, [&](uint32_t f, uint32_t p, uint32_t t, uint32_t b) {
                const uint32_t x15 = lim_r + (j0 + p) * P + ((__brev(t) >> (32 - b)) << (15 - LIT_ROOT - b));
                uint32_t l, e = bad_e;
                if (x15 < top) {
                    const uint32_t s = sorted[canon_index_in<LIT_ROOT + 1, 15>(H, CL, x15, l)];
                    e = make_final(s, l);
                }
                L.pool[used + f] = e;
            });
            used += total;
        }
    }
    WSYNC();
    return 0;
}

// Distance tables from lens[0..n); `used` = pool words the literal/length tables took.  Returns 0, -1 or 1 as build_litlen.
__device__ CHIP_PHASE_FN int build_dist(WaveLds &L, const uint8_t *lens, int n, uint32_t used STAT_PARAM)
{
    const uint32_t lane = lane_id();
    HuffMeta &H = L.hdr.dist_h;
    uint16_t *const sorted = L.hdr.dist_sorted;
    const int r = canon_prep(L.hdr.count, lens, n, false, sorted, H, [](uint32_t s, uint32_t) { return (uint16_t)s; } STAT_ARG);
    if (r < 0) return -1;
    if (r == 1) {  // no distance code: zlib accepts the block, every match is invalid
        for (uint32_t idx = lane; idx < (1u << DIST_ROOT); idx += 64) L.dist_root[idx] = (uint16_t)(1u | D_BAD);
        WSYNC();
        return 0;
    }
    const CanonLim CL = canon_limits(H);
    const uint32_t lim_r = CL.lim[DIST_ROOT], top = CL.lim[15], maxlen = rdfirst(H.maxlen);
    uint16_t *const pool16 = (uint16_t *)L.pool;
    for (uint32_t idx = lane; idx < (1u << DIST_ROOT); idx += 64) {
        const uint32_t x15 = __brev(idx) >> 17;
        if (x15 >= top) L.dist_root[idx] = (uint16_t)(maxlen | D_BAD);
        else if (x15 < lim_r) {
            uint32_t l;
            const uint32_t s = sorted[canon_index_in<1, DIST_ROOT>(H, CL, x15, l)];
            L.dist_root[idx] = (uint16_t)make_dist16(s, l);
        }
    }
    if (top > lim_r) {
        constexpr uint32_t P = 1u << (15 - DIST_ROOT);
        const uint32_t np = (top - lim_r + P - 1) / P;  // at most 15: thirty symbols, two per longer prefix
        uint32_t used16 = 0;
        for (uint32_t j0 = 0; j0 < np; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool have = j < np;
            const uint32_t xj = lim_r + j * P;
            uint32_t sb = 0;
            if (have) {
                uint32_t l;
                (void)canon_index_in<DIST_ROOT + 1, 15>(H, CL, xj + P < top ? xj + P - 1 : top - 1, l);
                sb = l - DIST_ROOT;
            }
            const uint32_t size = have ? (1u << sb) : 0u;
            const uint32_t incl = wave_incl_scan(size);
            const uint32_t total = rdlane(incl, 63);
            if (2 * used + used16 + total > POOL_U16) return 1;
            STAT_ADD(23, (total + 63u) / 64u);
            const uint32_t base16 = POOL_U16 - used16 - incl;  // sub-tables grow downwards from the top
            if (have) L.dist_root[__brev(xj >> (15 - DIST_ROOT)) >> (32 - DIST_ROOT)] = (uint16_t)(D_LONG | sb | ((2u * base16 - DIST_SUB_BYTES) << 3));
            fill_flat(L.hdr.cl_lut, have, sb, incl - size, total, [&](uint32_t f, uint32_t p, uint32_t t, uint32_t b) {
                const uint32_t x15 = lim_r + (j0 + p) * P + ((__brev(t) >> (32 - b)) << (15 - DIST_ROOT - b));
                uint32_t l, e = maxlen | D_BAD;
                if (x15 < top) {
                    const uint32_t s = sorted[canon_index_in<DIST_ROOT + 1, 15>(H, CL, x15, l)];
                    e = make_dist16(s, l);
                }
                pool16[POOL_U16 - used16 - (f - t) - (1u << b) + t] = (uint16_t)e;  // the owner's base16, entry t
            });
            used16 += total;
        }
    }
    WSYNC();
    return 0;
}
// The pool entry of the literal/length code whose first bits are x's low ones; r = lit_root[x's low LIT_ROOT bits].  The root entry
// is used as it stands: [15:3] is a byte offset, [4:0] the width of the sub-table index.
__device__ __forceinline__ uint32_t pool_at(const WaveLds &L, uint32_t r, uint32_t x)
{
    return *(const uint32_t *)((const uint8_t *)L.pool + ((r >> 3) + (__builtin_amdgcn_ubfe(x, LIT_ROOT, r) << 2)));
}
// The sub-table entry of a distance code of more than DIST_ROOT bits; m = its root entry (D_LONG set), x's low bits the code.
__device__ __forceinline__ uint32_t dist_sub_at(const WaveLds &L, uint32_t m, uint32_t x)
{
    return *(const uint16_t *)((const uint8_t *)L.pool + DIST_SUB_BYTES + (__builtin_amdgcn_ubfe(m, 3, 9) + (__builtin_amdgcn_ubfe(x, DIST_ROOT, m) << 1)));
}

struct InWin {
    const uint32_t *g32;  // dword-aligned base covering the unit's bytes
    uint32_t total_dw;    // dwords that contain at least one byte of the unit
    uint32_t win0;        // header parser: dword index held in hdr.inbuf[0]
};


__device__ __forceinline__ void win_load(WaveLds &L, InWin &w, uint32_t dw_start)
{
    WSYNC();
    w.win0 = dw_start;
    // all loads of the window go out before the first LDS store waits for one
    constexpr uint32_t PER_LANE = (HDR_IN_DW + 63) / 64;
    uint32_t v[PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < PER_LANE; j++) {
        const uint32_t i = dw_start + 64u * j + lane_id();
        v[j] = i < w.total_dw ? w.g32[i] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < PER_LANE; j++) {
        const uint32_t k = 64u * j + lane_id();
        if (k < HDR_IN_DW) L.hdr.inbuf[k] = v[j];
    }
    WSYNC();
}

// make sure the dwords covering `span` bits from `pos` (plus one for the funnel shift) are staged
__device__ __forceinline__ void win_ensure(WaveLds &L, InWin &w, uint32_t pos, uint32_t span = 64)
{
    uint32_t d = pos >> 5;
    if (d < w.win0 || d + ((span + 62u) >> 5) + 1u > w.win0 + HDR_IN_DW) win_load(L, w, d);
}

// 64 stream bits starting at `pos` (lo = first 32)
__device__ __forceinline__ void win_bits(const WaveLds &L, const InWin &w, uint32_t pos, uint32_t &lo, uint32_t &hi)
{
    uint32_t D = (pos >> 5) - w.win0, sh = pos & 31;
    uint32_t d0 = L.hdr.inbuf[D], d1 = L.hdr.inbuf[D + 1], d2 = L.hdr.inbuf[D + 2];
    lo = __builtin_amdgcn_alignbit(d1, d0, sh);
    hi = __builtin_amdgcn_alignbit(d2, d1, sh);
}

// the same at a wave-uniform position: the result is the same in every lane, and is handed back as such (scalar
// registers; branches on header fields become scalar branches instead of exec-mask regions)
__device__ __forceinline__ void win_bits_uniform(const WaveLds &L, const InWin &w, uint32_t pos, uint32_t &lo, uint32_t &hi)
{
    uint32_t l, h;
    win_bits(L, w, pos, l, h);
    lo = rdfirst(l);
    hi = rdfirst(h);
}

__device__ __forceinline__ uint32_t bfe(uint32_t v, uint32_t off, uint32_t width) { return __builtin_amdgcn_ubfe(v, off, width); }

// zlib / gzip header (RFC 1950 sec. 2.2, RFC 1952 sec. 2.3), checks in zlib's order.  Returns
// ST_RUNNING and the header length in bytes, or the final status (need-input / error / need-dict).
__device__ int32_t parse_wrapper(LDS_AS uint32_t *tab, const uint8_t *gin, uint32_t avail, int32_t format, uint32_t &wrap, uint32_t &hdr)
{
    wrap = 0;
    hdr = 0;
    if (avail < 2) return CHIP_NEED_INPUT;
    const uint32_t b0 = gin[0], b1 = gin[1];
    const bool allow_gzip = format == CHIP_FMT_GZIP || format == CHIP_FMT_AUTO;
    const bool allow_zlib = format == CHIP_FMT_ZLIB || format == CHIP_FMT_AUTO;
    if (allow_gzip && b0 == 0x1f && b1 == 0x8b) {
        wrap = 2;
        if (avail < 4) return CHIP_NEED_INPUT;
        const uint32_t flg = gin[3];
        if (gin[2] != 8) return Z_DATA_ERROR;  // unknown compression method
        if (flg & 0xe0) return Z_DATA_ERROR;   // unknown header flags set
        if (avail < 10) return CHIP_NEED_INPUT;
        uint32_t k = 10;
        if (flg & 4) {  // FEXTRA
            if (avail < k + 2) return CHIP_NEED_INPUT;
            uint32_t xlen = gin[k] | ((uint32_t)gin[k + 1] << 8);
            k += 2;
            if (avail - k < xlen) return CHIP_NEED_INPUT;
            k += xlen;
        }
        for (uint32_t bit = 8; bit <= 16; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
            if (!(flg & bit)) continue;
            for (;;) {
                uint32_t idx = k + lane_id();
                uint64_t z = __ballot(idx < avail && gin[idx] == 0);
                if (z) {
                    k += (uint32_t)__ffsll((long long)z);
                    break;
                }
                if (avail - k <= 64) return CHIP_NEED_INPUT;
                k += 64;
            }
        }
        if (flg & 2) {  // FHCRC: low 16 bits of the CRC-32 of the header so far
            if (avail < k + 2) return CHIP_NEED_INPUT;
            uint32_t crc = wave_crc32(tab, gin, k);
            if ((crc & 0xffffu) != (gin[k] | ((uint32_t)gin[k + 1] << 8))) return Z_DATA_ERROR;
            k += 2;
        }
        hdr = k;
        return ST_RUNNING;
    }
    if (!allow_zlib) return Z_DATA_ERROR;                  // incorrect header check
    if (((b0 << 8) | b1) % 31u) return Z_DATA_ERROR;       // incorrect header check
    if ((b0 & 15u) != 8) return Z_DATA_ERROR;              // unknown compression method
    if ((b0 >> 4) + 8 > 15) return Z_DATA_ERROR;           // invalid window size
    wrap = 1;
    hdr = 2;
    if (b1 & 0x20) {  // FDICT: compu never sets a dictionary, zlib answers Z_NEED_DICT after the id
        if (avail < 6) return CHIP_NEED_INPUT;
        hdr = 6;
        return CHIP_NEED_DICT;
    }
    return ST_RUNNING;
}

// unaligned accesses (gfx950 handles any byte alignment for LDS and global dword accesses); LDS pointers carry their
// address space so that a choice between an LDS and a global source never turns into a flat access
struct __attribute__((packed)) U32u { uint32_t v; };
struct __attribute__((packed)) U16u { uint16_t v; };
struct __attribute__((packed)) U128u { uint32_t x, y, z, w; };
typedef LDS_AS uint8_t lds_u8;

// Stored-block payload: copy n bytes from byte offset `so` of the unit's input to gdst.  Byte copies bring the
// destination to 16-byte alignment, then every lane moves 16 bytes per piece, two pieces in flight: one (unaligned) dwordx4
// load straight from the source -- gfx950 takes any byte alignment -- and one aligned dwordx4 store: a memcpy at HBM rate.
__device__ void wave_copy_stored(uint8_t *gdst, const uint32_t *g32, uint32_t total_dw, uint32_t so, uint32_t n)
{
    const uint32_t lane = lane_id();
    const uint8_t *gsrc = (const uint8_t *)g32 + so;
    uint32_t head = (uint32_t)((16u - ((uintptr_t)gdst & 15u)) & 15u);
    if (head > n) head = n;
    if (lane < head) gdst[lane] = gsrc[lane];
    uint32_t done = head;
    const uint32_t body = (n - done) & ~15u;  // every 16-byte read lies inside the n source bytes
    if (body) {
        uint4 *d16 = (uint4 *)(gdst + done);
        const U128u *s16 = (const U128u *)(gsrc + done);
        const uint32_t cnt = body >> 4;
        uint32_t i = lane;
#ifdef CHIP_STORED_NT_LD
#define CHIP_STORED_LD(p) __builtin_nontemporal_load(p)
#else
#define CHIP_STORED_LD(p) (*(p))
#endif
#ifndef CHIP_STORED_PLAIN_ST  // stored bytes are written once: the non-temporal hint keeps them from pushing other units' windows out of L2 (0.507 -> 0.476 ms per 16 384 units)
#define CHIP_STORED_ST(v, p) __builtin_nontemporal_store(v, p)
#else
#define CHIP_STORED_ST(v, p) (*(p) = (v))
#endif
#ifndef CHIP_STORED_DEPTH
#define CHIP_STORED_DEPTH 2  // 16-byte pieces per lane in flight (4 and 8 measured slower: 1.62 / 1.65 / 1.70 ms per 65 536 units)
#endif
        for (; i + 64u * (CHIP_STORED_DEPTH - 1) < cnt; i += 64u * CHIP_STORED_DEPTH) {
            u32x4 v[CHIP_STORED_DEPTH];
#pragma unroll
            for (int k = 0; k < CHIP_STORED_DEPTH; k++) v[k] = CHIP_STORED_LD((const u32x4_u *)(s16 + i + 64u * k));
#pragma unroll
            for (int k = 0; k < CHIP_STORED_DEPTH; k++) CHIP_STORED_ST(v[k], (u32x4 *)(d16 + i + 64u * k));
        }
        for (; i < cnt; i += 64u) {
            const U128u a = s16[i];
            d16[i] = make_uint4(a.x, a.y, a.z, a.w);
        }
        done += body;
    }
    const uint32_t tail = n - done;
    if (lane < tail) gdst[done + lane] = gsrc[done + lane];
    (void)total_dw;
}

// (off % d) for off, d < 512 without an integer divide
__device__ __forceinline__ uint32_t small_mod(uint32_t off, uint32_t d)
{
    uint32_t q = (uint32_t)(((float)off + 0.5f) * __builtin_amdgcn_rcpf((float)d));
    return off - q * d;
}
// ---- LZ77 execution -----------------------------------------------------------------------------
// The true token stream of a walk round is executed a chunk at a time.  A chunk is as many tokens as
// produce at most CHUNK_BYTES of output; the chunk's output is assembled in LDS (the image) and leaves
// with coalesced dword stores.  Tokens are taken 64 at a time (lane = token): a wave prefix sum of the
// output lengths places every token, literal lanes drop their byte into the image at once, match lanes
// append {position, length, distance} to a queue in LDS.  Whenever 64 matches are queued they are
// executed one per lane: a lane whose source is complete (entirely below the chunk: the unit's earlier
// output in HBM; or inside the image below the first match of the round) copies up to COPY_LANE_MAX
// bytes with 16-byte unaligned loads and exact-length unaligned LDS stores; what is left (sources that
// depend on matches of the same round, self-overlapping, very long or chunk-straddling matches) is done
// in further passes or, when few, one match at a time by the whole wave.
struct ChunkLds {
    uint32_t *out;  // [IMG_WORDS] the chunk's output bytes by offset (offset 0 = the dword-aligned address below the chunk)
    uint2 *mq;      // [MQ_CAP] queued match: .x offset of its first output byte, .y length | distance << 16
    uint32_t *tok;  // [64 * TOK_RING] token groups, written by global_load_lds_dword
    lds_u8 *trash;  // 16 bytes nobody reads: a lane with nothing to store stores there (a select, not a branch around the store)
};

__device__ __forceinline__ ChunkLds chunk_lds(WaveLds &L)
{
    ChunkLds c;
    c.out = L.fl.out;
    c.mq = L.fl.mq;
    c.tok = L.fl.tok;
    c.trash = (lds_u8 *)L.fl.trash;
    return c;
}

// exactly n (0..16) bytes of v to the LDS address d.  No branches: a store that n does not reach goes to `trash` (16 bytes that
// nobody reads) through a select of its address -- a compare and a select per store where an exec-mask region costs five or six
// instructions, most of them scalar, whether or not a lane is left in it.
__device__ __forceinline__ void lds_put(lds_u8 *d, lds_u8 *trash, const U128u &v, uint32_t n)
{
    ((LDS_AS U32u *)(n >= 4 ? d : trash))->v = v.x;
    ((LDS_AS U32u *)((n >= 8 ? d : trash) + 4))->v = v.y;
    ((LDS_AS U32u *)((n >= 12 ? d : trash) + 8))->v = v.z;
    ((LDS_AS U32u *)((n >= 16 ? d : trash) + 12))->v = v.w;
    const uint32_t w = n < 4 ? v.x : n < 8 ? v.y : n < 12 ? v.z : v.w;  // (n = 16: nothing below reads it)
    lds_u8 *const t = d + (n & 12u);
    const bool two = (n & 2u) != 0, one = (n & 1u) != 0;
    ((LDS_AS U16u *)(two ? t : trash))->v = (uint16_t)w;
    *(one ? (two ? t + 2 : t) : trash) = (uint8_t)(two ? w >> 16 : w);
}

// One queued match, copied by the whole wave (any distance, any length, source anywhere below it).
__device__ __forceinline__ void copy_one_match(lds_u8 *img, const uint8_t *base, uint32_t mis, uint32_t x, uint32_t len, uint32_t dist)
{
    const uint32_t lane = lane_id();
    const int32_t sx = (int32_t)x - (int32_t)dist;
    for (uint32_t i = lane; i < len; i += 64) {
        // a self-overlapping match repeats its first `dist` bytes; all of them lie below x and are complete
        const int32_t s = sx + (int32_t)(dist >= len ? i : small_mod(i, dist));
        uint8_t b = 0;
        if (s < (int32_t)mis) b = ((GAS const uint8_t *)base)[s];
        if (s >= (int32_t)mis) b = img[s];
        img[x + i] = b;
    }
    LSYNC();
}

// A round = up to 64 queued matches, one per lane.  round_issue() takes them off the queue and starts the loads of the
// sources that lie entirely below the chunk (final bytes in HBM: nothing in the chunk can change them); round_finish()
// copies.  The caller puts the next token group's work between the two, so the loads' latency is covered.
struct Round {
    uint32_t x, len, dist;  // first output offset, length (0 = no match in this lane), distance
    bool glob;              // source entirely below the chunk: v0 / v1 hold its first 32 bytes
    U128u v0, v1;
};

// glob_ok: 16-byte reads that start below the chunk may run up to 15 bytes into the chunk's (not yet written) output
// range without leaving the unit's capacity.
__device__ __forceinline__ void round_issue(Round &r, const ChunkLds &C, const uint8_t *base, uint32_t mis, uint32_t qh, uint32_t nr,
                                            bool glob_ok)
{
    const uint32_t lane = lane_id();
    const bool act = lane < nr;
    const uint32_t qi = (qh + lane) & (MQ_CAP - 1u);
    const uint2 e = C.mq[qi];
    r.x = e.x;
    const uint32_t ld = act ? e.y : 0u;
    r.len = ld & 0xffffu;
    r.dist = ld >> 16;
    const int32_t sx = (int32_t)r.x - (int32_t)r.dist;
    r.glob = glob_ok && r.len != 0 && r.len <= COPY_LANE_MAX && sx + (int32_t)r.len <= (int32_t)mis;
    r.v0 = U128u{0, 0, 0, 0};
    r.v1 = U128u{0, 0, 0, 0};
#ifndef CHIP_EXP_NO_GLOB  // ablation (wrong output): the LZ77 source fetches from HBM are left out
    if (r.glob) {
        const u32x4_u t = *(GAS const u32x4_u *)(base + sx);
        r.v0 = U128u{t.x, t.y, t.z, t.w};
    }
#endif
#ifndef CHIP_EXP_NO_GLOB
    if (r.glob && r.len > 16u) {
        const u32x4_u t = *(GAS const u32x4_u *)(base + sx + 16);
        r.v1 = U128u{t.x, t.y, t.z, t.w};
    }
#endif
}

__device__ __forceinline__ void round_finish(const Round &r, const ChunkLds &C, const uint8_t *base, uint32_t mis STAT_PARAM)
{
    const uint32_t lane = lane_id();
    lds_u8 *const img = (lds_u8 *)C.out;
    const int32_t sx = (int32_t)r.x - (int32_t)r.dist;
    uint64_t pend = __ballot(r.len != 0);
    STAT_ADD(14, 1);
    while (pend) {
        const uint32_t f = (uint32_t)__ffsll((long long)pend) - 1u;
        const uint32_t wp = rdlane(r.x, f);  // every byte below the first pending match is final
        const bool mine = (pend >> lane) & 1ull;
        const bool loc = sx >= (int32_t)mis && (uint32_t)sx + r.len <= wp;
        const bool ready = mine && r.len <= COPY_LANE_MAX && (r.glob || loc);
        const uint64_t rm = __ballot(ready);
        if (!((rm >> f) & 1ull)) {  // long, self-overlapping or chunk-straddling: by the whole wave
            STAT_ADD(15, 1);
            copy_one_match(img, base, mis, wp, rdlane(r.len, f), rdlane(r.dist, f));
            pend &= pend - 1ull;
            continue;
        }
        STAT_ADD(12, 1);
        uint32_t rem = ready ? r.len : 0u;
#pragma unroll
        for (uint32_t it = 0; it < COPY_LANE_MAX / 16; it++) {
            if (it && !__any(rem != 0)) break;
            U128u v = it ? r.v1 : r.v0;
            if (rem && !r.glob) {
                const lds_u8 *sp = img + sx + (int32_t)(16u * it);
                v.x = ((const LDS_AS U32u *)sp)->v;
                v.y = ((const LDS_AS U32u *)(sp + 4))->v;
                v.z = ((const LDS_AS U32u *)(sp + 8))->v;
                v.w = ((const LDS_AS U32u *)(sp + 12))->v;
            }
            const uint32_t n = rem < 16u ? rem : 16u;  // (0 in a lane that is not copying: its stores go to the trash)
            lds_put(img + r.x + 16u * it, C.trash, v, n);
            rem -= n;
        }
        LSYNC();
        pend &= ~rm;
    }
}

// lane i's value of x from lane `src` (any lane; ds_bpermute: no LDS memory is touched)
__device__ __forceinline__ uint32_t lane_gather(uint32_t x, uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)x);
}

// ---- CHIP_F_COMPU_STATUS only (rare path): where zlib's inflate() stands when the output has filled ---------------
// zlib leaves with every bit of the token consumed during which (or, when the output was exactly full, in front of which) it ran
// out of room, and holds fewer than eight unused bits: its avail_in follows from the bit position behind that token.
// End of the token that starts at bit p (never an end-of-block code), read from memory with the block's tables.
// (second: the token is a literal pair and the code of its second literal counts too)
__device__ uint32_t token_end(const WaveLds &L, const InWin &w, uint32_t p, bool second)
{
    const uint32_t i = p >> 5;
    const uint32_t d0 = i < w.total_dw ? w.g32[i] : 0u, d1 = i + 1u < w.total_dw ? w.g32[i + 1u] : 0u, d2 = i + 2u < w.total_dw ? w.g32[i + 2u] : 0u;
    const uint32_t lo = __builtin_amdgcn_alignbit(d1, d0, p), hi = __builtin_amdgcn_alignbit(d2, d1, p);
    const uint32_t r = L.lit_root[lo & ((1u << LIT_ROOT) - 1u)];
    const uint32_t e = pool_at(L, r, lo);
    const uint32_t n1 = __builtin_amdgcn_ubfe(e, 10, 5);
    const uint32_t w2 = __builtin_amdgcn_alignbit(hi, lo, n1);
    if (!(e & F_LEN)) {
        if (!second) return p + n1;
        const uint32_t r2 = L.lit_root[w2 & ((1u << LIT_ROOT) - 1u)];
        return p + n1 + __builtin_amdgcn_ubfe(pool_at(L, r2, w2), 10, 5);
    }
    uint32_t m = L.dist_root[w2 & ((1u << DIST_ROOT) - 1u)];
    if (m & D_LONG) m = dist_sub_at(L, m, w2);
    return p + n1 + (m & 15u) + __builtin_amdgcn_ubfe(m, 4, 4);
}

// The chunk that began with stream token `cstart` at image offset `run0` overflowed the room `xcap` (image offsets): bit position
// behind the first token that does not fit entirely.  B = the super-round's first bit (lane l's chain starts at B + l * S_BITS).
__device__ __attribute__((always_inline)) uint32_t overflow_bit(const WaveLds &L, const InWin &w, const uint32_t *grow, uint32_t ntok, uint32_t npieces,
                                                           uint32_t cstart, uint32_t run0, uint32_t xcap, uint32_t B)
{
    const uint32_t lane = lane_id();
    const uint32_t pfirst = lane < npieces ? L.fl.pk[2u * lane] : 0xffffffffu;
    const uint32_t pdelta = lane < npieces ? L.fl.pk[2u * lane + 1u] : 0u;
    uint32_t run = run0;
    for (uint32_t g = cstart; g < ntok; g += 64u) {
        const uint32_t t = g + lane < ntok ? g + lane : ntok - 1u;
        uint32_t k = 0;  // pieces that start at or before token t
        for (uint32_t q = 0; q < npieces; q++) k += rdlane(pfirst, q) <= t ? 1u : 0u;
        const uint32_t d = lane_gather(pdelta, k - 1u);
        const uint32_t krow = (t + d) & 0xffffu, rb = d >> 16;
        const uint32_t tok = grow[rb + row_word(krow)];
        uint32_t olen = tok_olen(tok);
        if (g + lane >= ntok) olen = 0;
        const uint32_t incl = wave_incl_scan(olen);
        const uint64_t over = __ballot(olen != 0 && run + incl > xcap);
        if (over) {
            const uint32_t f = (uint32_t)__ffsll((long long)over) - 1u;
            const uint32_t rbf = rdlane(rb, f), kf = rdlane(krow, f);
            const uint32_t owner = ((rbf / (8u * ROW_TOKENS)) << 3) | ((rbf % (8u * ROW_TOKENS)) >> 2);  // row_base() inverted
            // zlib reads a literal's code before it looks for room: of a pair that overflows, the second code is consumed only
            // if the first byte was written
            const bool both = rdlane(run + incl - 1u, f) <= xcap;
            uint32_t p = B + owner * S_BITS;
            for (uint32_t j = 0; j <= kf; j++) {
                const uint32_t tj = rdfirst(grow[rbf + row_word(j)]);
                p = rdfirst(token_end(L, w, p, (tj >> 31) != 0 && (j < kf || both)));
            }
            return p;
        }
        run += rdlane(incl, 63u);
    }
    return 0;  // (not reached: the caller saw the overflow)
}

// Executes the ntok tokens of a batch of the true stream (npieces pieces described by L.fl.pk) into gout at opos.
// Returns false when decoding must stop (error / output full).
// (ovf: on CHIP_NEED_OUTPUT the overflowing chunk's first stream token, first image offset and room, for overflow_bit())
__device__ CHIP_PHASE_FN bool flush_tokens(WaveLds &L, const uint32_t *grow_, uint32_t ntok_, uint32_t npieces_, uint8_t *gout_, uint32_t &opos_,
                             uint32_t cap_, int32_t &status, uint32_t (&ovf)[3] STAT_PARAM)
{
    const uint32_t lane = lane_id();
    // every argument is wave-uniform; say so (scalar registers, scalar loop branches)
    const uint32_t *const grow = rdfirst_ptr(grow_);
    uint8_t *const gout = rdfirst_ptr(gout_);
    const uint32_t ntok = rdfirst(ntok_), npieces = rdfirst(npieces_), cap = rdfirst(cap_);
    uint32_t opos = rdfirst(opos_);
    const ChunkLds C = chunk_lds(L);
    lds_u8 *const img = (lds_u8 *)C.out;
    if (ntok == 0) return true;
    // piece `lane`: first stream index, and what to add to a stream index to get the token's word in the scratch rows
    const uint32_t pfirst = lane < npieces ? L.fl.pk[2u * lane] : 0xffffffffu;
    const uint32_t pdelta = lane < npieces ? L.fl.pk[2u * lane + 1u] : 0u;
    // Token g + lane of the stream (lanes behind the end re-read the last token: no branch around the load).  The pieces are in
    // stream order, so a scalar cursor walks them: `before` pieces start in front of the group, `nfirst` is where the next one
    // starts and `dcur` is the delta of the piece the group begins in.  A group that lies inside one piece (most do: a piece
    // is a lane's whole run of tokens) takes `dcur` as it stands; every piece that starts inside the group costs two lane
    // reads and one select.  No mask of piece starts, no bit count, no cross-lane gather.
    uint32_t before = 0;       // pieces that start before stream index gnext
    uint32_t nfirst = 0;       // first stream index of piece `before` (0xffffffff: there is none; piece 0 starts at 0)
    uint32_t dcur = 0;         // pdelta of piece before - 1
    uint32_t gnext = 0;        // stream index the next fetch() asks for
    const uint32_t tok_lds = rdfirst((uint32_t)(uintptr_t)(LDS_AS uint32_t *)C.tok);  // LDS byte address of the ring
    // The load goes straight into LDS (global_load_lds_dword: LDS address = M0 + 4 * lane): no register is held while it
    // is in flight, and the compiler does not wait for it -- issue() and the explicit vmcnt wait in front of a slot's
    // first read keep the count: a slot's load is complete once at most TOK_RING - 1 younger loads are outstanding.
    auto fetch = [&](const uint32_t slot_w) {
        const uint32_t g = gnext;
        uint32_t d = dcur;
        while (nfirst - g < 64u) {  // (nfirst >= g; "none" is far above any g)
            dcur = rdlane(pdelta, before);
            d = lane >= nfirst - g ? dcur : d;
            before++;
            const uint32_t nx = rdlane(pfirst, before & 63u);
            nfirst = before < npieces ? nx : 0xffffffffu;
        }
        const uint32_t t = min(g + lane, ntok - 1u);  // (lanes behind the batch's end read its last token again)
        gnext = g + 64u;
        const uint32_t krow = (t + d) & 0xffffu;  // the token's index in its lane's row
        const uint32_t *src = grow + ((d >> 16) + row_word(krow));
        const uint32_t dst = tok_lds + 256u * slot_w;
        uint32_t keep;  // (M0 is a reserved register: it cannot be named as clobbered, so it is put back)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(src), "s"(dst)
                     : "memory");
    };
    WSYNC();  // the piece descriptions are in LDS; whatever used the chunk state's place before is done
    uint32_t c0 = 0;  // tokens executed so far
    // Ring slot of the group at c0.  Whenever a group is taken whole, fetch() refills the slot just read with the group TOK_RING
    // ahead, and a partly taken group starts the ring over: the slot that is read next is always the slot that is filled next,
    // and one counter serves both.
    uint32_t slot_r = 0;
#pragma unroll
    for (uint32_t k = 0; k < TOK_RING; k++) fetch(k);
    for (;;) {  // one trip per chunk
        STAT_ADD(13, 1);
        const uint32_t mis = (uint32_t)((uintptr_t)(gout + opos) & 3u);
        uint8_t *const base = gout + opos - mis;  // byte x of the chunk lives at base[x]; base is dword aligned
        const bool glob_ok = cap - opos >= 16u;
        const uint32_t prod0 = opos - mis;  // output bytes in front of offset 0
        const uint32_t cstart = c0;
        uint32_t run = mis, nq = 0, qh = 0;
        Round R;
        bool inflight = false;  // R's loads are under way
        uint64_t globm = 0;     // R.glob by lane, as a scalar (a flag per lane carried around a loop costs three mask operations a trip)
        // ---- the group at c0: token, lengths, wave prefix sum
        // token: [8:0] literal byte or match length, [9] match, [25:10] distance - 1; a literal pair: [31], second byte in [23:16]
        // (a literal's byte is the token's low byte as it stands; length and distance are only formed where a match is queued)
        uint32_t t, len, val, left, incl, start, total;
        bool pair;
        uint64_t lenm;
        auto group = [&]() __attribute__((always_inline)) {
            static_assert(TOK_RING == 4, "the wait below counts three younger ring loads");
            asm volatile("s_waitcnt vmcnt(3)" ::: "memory");  // the load into slot_r has landed
            t = C.tok[64u * slot_r + lane];
            const bool ismatch = (t & 512u) != 0;
            len = ismatch ? t & 0x1ffu : 0u;
            val = ismatch ? __builtin_amdgcn_ubfe(t, 10, 16) + 1u : t;  // distance, or the literal (low byte)
            left = ntok - c0;
            pair = (int32_t)t < 0;
            uint32_t olen = ismatch ? len : 1u + (t >> 31);
            olen = lane < left ? olen : 0u;  // (only the last group of a batch has lanes behind the end)
            incl = wave_incl_scan(olen);
            start = run + incl - olen;
            total = rdlane(incl, 63u);
            lenm = __ballot(len != 0);
        };
        // ---- The steady loop: common groups and nothing else.  A common group is 64 tokens that all fit the chunk, no distance
        // reaching in front of the output's first byte.  It carries no flag of the chunk's end, no count of accepted tokens and no
        // stop mask: the first group that is not common leaves the loop as it stands in the registers, for the general code below.
        // (a distance cannot reach in front of the output once 32 KiB of it exist: dist_test is a constant of the chunk.  The
        // test is one compare in every lane, masked by the match lanes: a literal's `val` is below 256.  It goes by the chunk's
        // first output position, not by prod0: prod0 = opos - mis wraps below zero for a unit whose first byte is not dword
        // aligned, and the sum prod0 + start is right all the same)
        auto steady = [&](const bool dist_test) __attribute__((always_inline)) {
            // No round outlives its chunk, so R holds nothing here.  (The empty statements say so to the compiler, loop by loop:
            // left alone it carries R's eleven lane registers around the chunk loop in a second set, copies them at both ends of
            // each steady loop behind a wait for every load in flight, and runs out of lane registers elsewhere in the kernel.)
            {
                uint32_t u[11];
#pragma unroll
                for (int k = 0; k < 11; k++) asm volatile("" : "=v"(u[k]));
                R.x = u[0], R.len = u[1], R.dist = u[2], R.glob = false;
                R.v0 = U128u{u[3], u[4], u[5], u[6]};
                R.v1 = U128u{u[7], u[8], u[9], u[10]};
            }
            for (;;) {
                group();
                if (left < 64u || run + total > CHUNK_BYTES) break;
                if (dist_test && (__ballot(val > prod0 + start) & lenm) != 0) break;
                // (the markers keep the compiler from folding the loops into each other or into the general group)
                if (dist_test)
                    asm volatile("; a steady group, distances tested" ::: "memory");
                else
                    asm volatile("; a steady group" ::: "memory");
                // every lane makes all three stores, those it has nothing for to the trash: selects instead of exec-mask regions
                const uint32_t qi = __builtin_amdgcn_mbcnt_hi((uint32_t)(lenm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lenm, nq)) & (MQ_CAP - 1u);
                *(len == 0 ? img + start : C.trash) = (uint8_t)val;
                *(pair ? img + start + 1u : C.trash) = (uint8_t)(t >> 16);
                *(len != 0 ? &C.mq[qi] : (uint2 *)(uint8_t *)C.trash) = make_uint2(start, len | (val << 16));
                nq += (uint32_t)__popcll(lenm);
                c0 += 64u;
                run += total;
                LSYNC();  // literals and queue entries are in LDS; the slot's tokens are in registers
                STAT_ACC(16);
                // A round's source loads are started as soon as 64 matches are queued and it is finished when the next 64 are
                // (about three token groups later: the loads have landed by then), or at the chunk's end.
                if (nq - qh >= 64u) {
                    if (inflight) {
                        R.glob = __builtin_amdgcn_inverse_ballot_w64(globm);
                        round_finish(R, C, base, mis STAT_ARG);
                    }
                    round_issue(R, C, base, mis, qh, 64u, glob_ok);
                    globm = __ballot(R.glob);
                    qh += 64u;
                    inflight = true;
                }
                STAT_ACC(17);
                // (behind the round: its waits do not hold a ring load that was only just issued)
                fetch(slot_r);
                slot_r = (slot_r + 1u) & (TOK_RING - 1u);
            }
        };
        // Two loops: opos only grows, so half the chunks of a 64 KiB unit run the one without the test.  (One loop with the flag
        // tested per trip was built too: the compiler splits it in two by itself and then carries R through the trip in a second
        // set of registers, eighteen copies per group.)
        if (opos < 32768u)
            steady(true);
        else
            steady(false);
        // ---- The general group, which ends the chunk: the batch's last tokens (fewer than 64, or none when the batch ended with
        // a steady group), a group that does not fit, or one with a distance too far back.
        const uint32_t nvalid = left < 64u ? left : 64u;
        // stops: the first token that does not fit the chunk, or with an "invalid distance too far back" (the distance
        // reaches before the first output byte)
        const uint64_t validm = nvalid == 64u ? ~0ull : (1ull << nvalid) - 1ull;
        const uint64_t nofit = __ballot(incl > CHUNK_BYTES - run) & validm;
        const uint64_t badm = __ballot(val > prod0 + start) & lenm & validm;
        const uint64_t stopm = nofit | badm;
        uint32_t nacc = stopm ? (uint32_t)__ffsll((long long)stopm) - 1u : nvalid;
        // a group that does not fit is left whole to the next chunk (the prefetched group stays the right one) unless the
        // chunk is empty (long matches: 64 tokens can be 16 KB) or the stop is an error
        const bool too_far = stopm != 0 && ((badm & ~nofit) >> nacc) & 1ull;
        if (stopm && !too_far && run != mis) nacc = 0;
        // (a pair whose second byte does not fit the chunk is a token that does not fit: it goes whole to the next chunk)
        if (lane < nacc && len == 0) img[start] = (uint8_t)val;
        if (lane < nacc && pair) img[start + 1u] = (uint8_t)(t >> 16);
        const uint64_t mm = lenm & (nacc == 64u ? ~0ull : (1ull << nacc) - 1ull);
        if (lane < nacc && len != 0) {
            const uint32_t qi = __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, nq)) & (MQ_CAP - 1u);
            C.mq[qi] = make_uint2(start, len | (val << 16));
        }
        nq += (uint32_t)__popcll(mm);
        c0 += nacc;
        if (stopm) {
            if (nacc) run = rdlane(start, nacc);
        } else {
            run += total;
        }
        LSYNC();
        STAT_ACC(16);
        // ---- the chunk's last rounds: the one in flight, then what is left in the queue
        for (;;) {
            if (inflight) {
                R.glob = __builtin_amdgcn_inverse_ballot_w64(globm);
                round_finish(R, C, base, mis STAT_ARG);
                inflight = false;
            }
            const uint32_t pq = nq - qh;
            if (pq == 0) break;
            const uint32_t nr = pq < 64u ? pq : 64u;
            round_issue(R, C, base, mis, qh, nr, glob_ok);
            globm = __ballot(R.glob);
            qh += nr;
            inflight = true;
        }
        // (To the compiler a round may still be loading into R: round_finish() does not read v0 and v1 on every path.  R is read
        // here for nothing, so that the compiler's wait for those loads stands here, where the ring's loads are a group old or
        // older, and not in front of the first reuse of the registers below, where it would wait for the loads issued there.)
        asm volatile("" ::"v"(R.v0.x), "v"(R.v0.y), "v"(R.v0.z), "v"(R.v0.w), "v"(R.v1.x), "v"(R.v1.y), "v"(R.v1.z), "v"(R.v1.w));
        STAT_ACC(17);
        // ---- the token ring
        if (nacc == 64u) {
            fetch(slot_r);
            slot_r = (slot_r + 1u) & (TOK_RING - 1u);
        } else if (nacc != 0 && c0 < ntok) {  // a partly taken group: the stream moves by less than a group, the ring starts over
            gnext = c0;
            before = (uint32_t)__popcll(__ballot(pfirst < c0));  // (at least one: piece 0 starts at 0 and c0 is not 0 here)
            dcur = rdlane(pdelta, before - 1u);
            {
                const uint32_t nx = rdlane(pfirst, before & 63u);
                nfirst = before < npieces ? nx : 0xffffffffu;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no load of the old ring is left to land on the new one
            slot_r = 0;
#pragma unroll
            for (uint32_t k = 0; k < TOK_RING; k++) fetch(k);
        }
        // ---- the finished chunk: offsets [mis, min(run, capacity)) of the LDS image go to HBM
        const uint32_t xcap = cap - (opos - mis);
        {
            const uint32_t xe = run < xcap ? run : xcap;
            // The whole 16-byte blocks from image offset 16 on: one LDS read and one global store of four dwords per lane and trip
            // (the image offset is a multiple of 16, the address dword aligned), 1 KiB per trip.
            for (uint32_t xq = 16u + 16u * lane; xq + 16u <= xe; xq += 1024u) *(GAS u32x4_a4 *)(base + xq) = *(const LDS_AS u32x4 *)(img + xq);
            // The first block (what lies below `mis` belongs to the chunk before) and the partial last one, byte-exact: lanes 0..15
            // hold the first block's bytes, lanes 16..31 those behind the last whole block; one byte store for both.
            const uint32_t xt = xe < 16u ? 16u : xe & ~15u;
            const uint32_t xb = lane < 16u ? lane : xt + (lane - 16u);
            if (lane < 32u && xb >= mis && xb < xe) ((GAS uint8_t *)base)[xb] = img[xb];
        }
        WSYNC();  // the next chunk overwrites the image and may load these bytes from memory
        STAT_ACC(18);
        opos += run - mis;
        opos_ = opos;
        // zlib tests a match's distance only once there is room for its first byte: a match that reaches too far back while the
        // output is exactly full is "no room", not an error
        const bool no_room = opos > cap || (too_far && opos == cap);
        if (no_room || too_far) {
            if (no_room) {
                opos_ = cap;
                ovf[0] = cstart;
                ovf[1] = mis;
                ovf[2] = xcap;
            }
            status = no_room ? CHIP_NEED_OUTPUT : Z_DATA_ERROR;
            return false;
        }
        if (c0 >= ntok) return true;
    }
}
// ---- the walk of a super-round -----------------------------------------------------------------------------
constexpr size_t SCRATCH_WORDS = ROWS_WORDS;


// why a lane's chain ended
enum : uint32_t { R_JOIN = 1, R_LIMIT = 2, R_EOB = 3, R_NEED_INPUT = 4, R_BAD = 5 };

// One super-round: stages the input from the true token boundary B on, walks 64 chains, finds the true stream among them and
// leaves its description in L.fl.pk (ntok tokens in npieces pieces).  term_why / term_pos say how and where the stream ends.
__device__ CHIP_PHASE_FN uint32_t walk_round(WaveLds &L, const InWin &w, const uint32_t B_, const uint32_t end_bit_, uint32_t *rows_, const uint32_t xt_bits,
                                             uint32_t &ntok_out, uint32_t &term_why, uint32_t &term_pos STAT_PARAM)
{
    const uint32_t lane = lane_id();
    const uint32_t B = rdfirst(B_), end_bit = rdfirst(end_bit_);
    GAS const uint32_t *const g32 = rdfirst_gptr(w.g32);
    const uint32_t total_dw = rdfirst(w.total_dw);
    GAS uint32_t *const myrow = rdfirst_gptr(rows_) + row_base(lane);
    const uint32_t D0 = B >> 5;
    WSYNC();  // the phase before (header parse, previous flush) is done with the window's place
    {
        // Four dwords per lane and access: WIN_Q whole quads of input (loaded dword aligned, stored 16-byte aligned: win[] is the
        // structure's first member) and BM_Q 16-byte aligned quads of zeroed mark bits.  What that leaves goes one dword per lane
        // in a narrow step of EDGE_LANES lanes: the quad the input ends in (lanes 0..3: no load touches a dword at or beyond
        // total_dw; the wide store has zeroed the quad, these dwords overwrite it), the window's dwords behind its last whole
        // quad, and the mark words in front of and behind the aligned quads.  win[] and bm[] are neighbours: one index serves both.
        constexpr uint32_t WIN_Q = WIN_DW / 4, WIN_R = WIN_DW % 4;
        constexpr uint32_t BM_A = (WIN_DW + 3u) & ~3u;                // first 16-byte aligned word of bm[], as an index from win[0]
        constexpr uint32_t BM_Q = (2u * WIN_DW - BM_A) / 4, BM_TAIL = (2u * WIN_DW - BM_A) % 4;
        constexpr uint32_t EDGE_LO = WIN_R + (BM_A - WIN_DW);         // dwords between the window's last whole quad and BM_A
        constexpr uint32_t EDGE_LANES = 4u + EDGE_LO + BM_TAIL;
        constexpr uint32_t PER_LANE = (WIN_Q + 63) / 64;
        static_assert(offsetof(WaveLds, w.win) == 0 && offsetof(WaveLds, w.bm) == 4 * WIN_DW && BM_Q <= WIN_Q && EDGE_LANES <= 64, "window staging");
        uint32_t *const ww = L.w.win;
        const uint32_t rem = total_dw - D0;  // dwords of input from the window's first on (at least one: B lies inside the input)
        // all loads of the window go out before the first LDS store waits for one
        static_assert(PER_LANE <= 4, "the quads per lane below");  // (named values, not an array: as an array the compiler waits for each load in turn)
        auto quad = [&](uint32_t j) -> u32x4 {
            const uint32_t k = 64u * j + lane;
            if ((64u * j + 63u < WIN_Q || k < WIN_Q) && 4u * k + 4u <= rem) return *(GAS const u32x4_a4 *)(g32 + D0 + 4u * k);
            return u32x4{0, 0, 0, 0};
        };
        const u32x4 v0 = quad(0), v1 = quad(1), v2 = quad(2), v3 = quad(3);  // (a quad index no lane has costs nothing)
        uint32_t ni = 4u * (rem >> 2) + lane;
        bool nput = ni < rem && ni < 4u * WIN_Q;
        if (lane >= 4u) {
            const uint32_t j = lane - 4u;
            ni = j < EDGE_LO ? 4u * WIN_Q + j : 2u * WIN_DW - BM_TAIL + (j - EDGE_LO);
            nput = j < EDGE_LO + BM_TAIL;
        }
        uint32_t nv = 0;
        if (nput && ni < rem && ni < WIN_DW) nv = g32[D0 + ni];
#pragma unroll
        for (uint32_t j = 0; j < PER_LANE; j++) {
            const uint32_t k = 64u * j + lane;
            if (64u * j + 63u < WIN_Q || k < WIN_Q) *(u32x4 *)(ww + 4u * k) = j == 0 ? v0 : j == 1 ? v1 : j == 2 ? v2 : v3;
            if (64u * j + 63u < BM_Q || k < BM_Q) *(u32x4 *)(ww + BM_A + 4u * k) = u32x4{0, 0, 0, 0};
        }
        if (nput) ww[ni] = nv;
    }
    LSYNC();
    STAT_ACC(1);
    STAT_ADD(8, 1);
    // ---- walk: every lane decodes from its guessed start until it joins another lane's chain ----
    const uint32_t s0 = B + lane * S_BITS;
    const uint32_t own_end = s0 + S_BITS;
    uint32_t hard = own_end + xt_bits;  // a token is taken if it ends in front of this: the chain's limit, the input's end
    {
        const uint32_t sr_end = B + 64u * S_BITS;  // nobody to join behind the last segment
        hard = hard < sr_end ? hard : sr_end;
        hard = hard < end_bit ? hard : end_bit;
    }
    // Positions inside the walk count from the window's first bit (32 * D0): a position's byte address in the window and in the mark
    // bits is then a shift and a mask.  q = position of the next token; a step adds the token's length to it before it knows whether
    // the token can be taken -- a lane that drops out keeps the length (tl), and the token's start is q - tl.
    const uint32_t wbase = 32u * D0;
    const uint32_t own_end_r = own_end - wbase, hard_r = hard - wbase;
    uint32_t q = s0 - wbase, tl = 0, nst = 0;
    uint32_t jb = 0, z = 0;  // of the lane's last token: join bit, halt flags
    bool run = s0 < end_bit;
    // nx = the stream's bits from q on, of which a step uses the low 15: the 9 of the root index and the at most 6 of a sub-table's.
    // Every step leaves them for the next one out of the 64 bits it holds anyway, so that the next step's two table reads start
    // from a register and not from its window read, which lands while they are in flight.
    uint32_t nx;
    {
        const uint32_t *wp = (const uint32_t *)((const uint8_t *)L.w.win + ((q >> 3) & ~3u));
        nx = __builtin_amdgcn_alignbit(wp[1], wp[0], q);
    }
    // A token's work is straight-line code; a lane whose token cannot be taken (it joined another chain, met an end-of-block or
    // invalid code, or the token ends behind `hard`) drops out with jb / z / pn as that step left them: the reason is read off them
    // after the loop.
    auto token = [&](uint32_t &tok) -> bool {
        const uint32_t p = q;
        const uint32_t a = (p >> 3) & ~3u;
        const uint32_t bit = 1u << (p & 31u);
        const uint32_t mine = p < own_end_r ? bit : 0u;
        const uint32_t old = atomicOr((uint32_t *)((uint8_t *)L.w.bm + a), mine);
        jb = old & bit & ~mine;  // a boundary of the segment's owner: from here on the two chains are one (one three-input bit operation)
        const uint32_t *wp = (const uint32_t *)((const uint8_t *)L.w.win + a);
        const uint32_t d0 = wp[0], d1 = wp[1], d2 = wp[2];
        const uint32_t lo = __builtin_amdgcn_alignbit(d1, d0, p), hi = __builtin_amdgcn_alignbit(d2, d1, p);
        const uint32_t r = L.lit_root[nx & ((1u << LIT_ROOT) - 1u)];  // (nx and lo agree in their low 16 bits)
        const uint32_t e = pool_at(L, r, nx);
        const uint32_t n1 = __builtin_amdgcn_ubfe(e, 10, 5);
        const uint32_t msk = (uint32_t)((int32_t)e >> 31);  // all ones for a length code
        const uint32_t w2 = __builtin_amdgcn_alignbit(hi, lo, n1);
        uint32_t m = L.dist_root[w2 & ((1u << DIST_ROOT) - 1u)] & msk;
#ifndef CHIP_EXP_NO_PAIR
        // A literal takes the literal behind it along as one token (a pair) when there is one, it ends inside the chain's limit, and
        // its start is no boundary of the segment's owner: a chain that pairs across the owner's boundary walks one literal out of
        // phase with the owner and cannot join before the run of literals ends.  (Inside its own segment a lane sees no mark in
        // front of it.)  Whatever else the second code is, the literal goes alone, and that code is met as a token's first.
        // The second code's root entry and its mark word have their addresses as soon as n1 is known: both reads go out beside the
        // distance root's, in front of the branch below, and share its wait (one LDS round trip, not two).
        const uint32_t p2 = p + n1;
        const uint32_t r2 = L.lit_root[w2 & ((1u << LIT_ROOT) - 1u)];
        const uint32_t mw2 = *(const uint32_t *)((const uint8_t *)L.w.bm + ((p2 >> 3) & ~3u));
#endif
        // a distance code of more than 8 bits (1 % of the matches) goes through its sub-table: five steps in six have no such lane
        if (__any((m & D_LONG) != 0)) {
            asm volatile("; long distance codes");  // (keeps the skip: the compiler would issue the short region in every step)
            if (m & D_LONG) m = dist_sub_at(L, m, w2);
        }
#ifndef CHIP_EXP_NO_PAIR
        const uint32_t e2 = pool_at(L, r2, w2);
        const uint32_t mk2 = __builtin_amdgcn_ubfe(mw2, p2, 1);
#endif
        const uint32_t cl2 = m & 15u, eb2 = __builtin_amdgcn_ubfe(m, 4, 4);
        // (only a token that is taken uses dm1: its entry has neither D_BAD nor D_LONG, so what lies above bit 8 is the mantissa)
        const uint32_t dm1 = ((m >> 8) << eb2) + __builtin_amdgcn_ubfe(w2, cl2, eb2);
        z = (e & (F_HALT | F_INV)) | (m & D_BAD);
        tl = n1 + cl2 + eb2;
#ifndef CHIP_EXP_NO_PAIR
        const uint32_t n2 = __builtin_amdgcn_ubfe(e2, 10, 5);
        const bool pair = ((e | e2) & (F_LEN | F_HALT)) == 0 && p2 + n2 <= hard_r && mk2 == 0;
        tl += pair ? n2 : 0u;
        const uint32_t pr = pair ? (e2 & 0x00ff0000u) | 0x80000000u : 0u;
#else
        const uint32_t pr = 0;
#endif
        // hi:lo is 64 bits from p on.  A token has at most 48: a match's length code of 15 bits and 5 extra ones (n1 <= 20), then a
        // distance code of 15 bits and 13 extra ones; a pair has 15 + 15.  That leaves at least 16 bits of the next position.
        static_assert((15 + 5) + (15 + 13) == 48 && 64 - 48 >= LIT_ROOT + (15 - LIT_ROOT), "the next step's index bits are in hi:lo");
        nx = (uint32_t)((((uint64_t)hi << 32) | lo) >> (tl & 63u));
        q = p + tl;
        if ((jb | z) != 0 || q > hard_r) return false;
        const uint32_t v = __builtin_amdgcn_ubfe(lo, e, e >> 5) + __builtin_amdgcn_ubfe(e, 16, 10);  // (a length's entry brings the match bit)
        tok = (dm1 << 10) | v | pr;  // (a literal's m is zero, and so is its dm1)
        return true;
    };
    bool full = false;  // the lane's row is full
    while (__any(run)) {
        STAT_ADD(11, 1);
        uint32_t t4[4];  // (a slot whose token is not taken keeps whatever its registers hold: nothing reads a row behind its lane's count)
#pragma unroll
        for (int k = 0; k < 4; k++) asm volatile("" : "=v"(t4[k]));
        uint32_t took = 0;  // tokens the lane takes in this trip: a constant per step, added to the row's count once
        if (run) {
            if (nst + 4u > ROW_TOKENS) {
                run = false;
                full = true;
            } else {
                bool ok = token(t4[0]);
                if (ok) {
                    took = 1;
                    ok = token(t4[1]);
                    if (ok) {
                        took = 2;
                        ok = token(t4[2]);
                        if (ok) {
                            took = 3;
                            ok = token(t4[3]);
                            if (ok) took = 4;
                        }
                    }
                }
                run = ok;
            }
        }
        if (took) *(GAS u32x4 *)(myrow + 8u * nst) = u32x4{t4[0], t4[1], t4[2], t4[3]};  // nst is a multiple of 4 here: row_word(nst)
        nst += took;
    }
    // back to stream positions: a lane that dropped out stands behind the token it did not take
    const bool dropped = s0 < end_bit && !full;
    const uint32_t pn = q + wbase;                     // end of the lane's last token (taken or not)
    const uint32_t p = pn - (dropped ? tl : 0u);       // start of the token that was not taken / of the next one
    // why the lane's last token was not taken, in zlib's order of verdicts
    uint32_t why = R_LIMIT;  // the chain simply ends (limit reached, row full, or it never ran)
    if (s0 < end_bit && !full) {
        if (jb) why = R_JOIN;
        else if (pn > end_bit) why = R_NEED_INPUT;  // the token does not end inside the input
        else if (z) why = z == F_HALT ? (uint32_t)R_EOB : (uint32_t)R_BAD;
    }
    STAT_ADD(21, __popcll(__ballot(nst != 0)));
    STAT_ACC(2);
    // ---- the true stream: lane 0's chain, then the chain it joined from the join on, and so on ----
    // the lane a chain joined, and the index, in that lane's row, of the token that starts at the join: the boundaries the
    // segment's owner marked in front of it
    const uint32_t rel = p - B;
    const uint32_t jl = why == R_JOIN ? (__umul24(rel, SEG_MAGIC) >> SEG_SHIFT) & 63u : lane;
    uint32_t a_join = 0;
    if (__any(why == R_JOIN)) {
        const uint32_t sj = B + jl * S_BITS;            // the owner's first bit
        const uint32_t w0 = (sj >> 5) - D0;             // ... and its dword in the window
        const uint32_t lo_cut = sj & 31u;               // bits below this in the first word belong to the segment before
        const uint32_t nb = p - (sj & ~31u);            // marks in front of bit nb (counted from the first word's bit 0) count
#pragma unroll
        for (uint32_t t = 0; t < SEG_WORDS; t++) {
            uint32_t mw = L.w.bm[w0 + t];
            if (t == 0) mw &= ~0u << lo_cut;
            const int32_t k = (int32_t)nb - 32 * (int32_t)t;
            const uint32_t keep = k <= 0 ? 0u : k >= 32 ? 0xffffffffu : (1u << k) - 1u;
            a_join += __popc(mw & keep);
        }
        if (why != R_JOIN) a_join = 0;
    }
    // the n-th piece of the stream = the lane reached from lane 0 by n joins: powers of the join map by doubling, composed along
    // the bits of n (lanes: ds_bpermute, no memory); the map's fixed points are the chains that end the stream
    uint32_t node = 0;  // lane n: the lane holding the stream's n-th piece
    {
        uint32_t pw = jl;  // the join map to the power 2^r
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const uint32_t nx = lane_gather(pw, node);
            if ((lane >> r) & 1u) node = nx;
            pw = lane_gather(pw, pw);
        }
    }
    const uint32_t prev = wave_shr1(node);                    // the piece before (lane 0: none)
    const bool fresh = lane == 0 || node != prev;               // lanes behind the stream's end repeat its last piece
    const uint32_t e_nst = lane_gather(nst, node);
    const uint32_t g_a0 = lane_gather(a_join, prev);  // (every lane takes part: a lane that is switched off cannot be read)
    const uint32_t e_a0 = lane == 0 ? 0u : g_a0;      // where the stream enters the piece
    const uint32_t cnt = (fresh && e_nst > e_a0) ? e_nst - e_a0 : 0u;
    const uint32_t incl = wave_incl_scan(cnt);
    const uint64_t nonempty = __ballot(cnt != 0);
    WSYNC();  // the walk's LDS reads are done (the flush's state takes the window's place)
    if (cnt) {
        const uint32_t k = (uint32_t)__popcll(nonempty & lanemask_lt()), first = incl - cnt;
        L.fl.pk[2u * k] = first;
        L.fl.pk[2u * k + 1u] = ((e_a0 - first) & 0xffffu) | (row_base(node) << 16);  // row token = stream index + (a0 - first)
    }
    const uint32_t kz = rdlane(node, 63);  // the chain the stream ends in
    term_why = rdlane(why, kz);
    term_pos = rdlane(p, kz);
    ntok_out = rdlane(incl, 63u);
    WSYNC();
    STAT_ACC(3);
    STAT_ADD(9, __popcll(nonempty));
    STAT_ADD(10, ntok_out);
    return (uint32_t)__popcll(nonempty);
}

// ---- the size pass: what the true stream of a super-round adds to the unit's decoded length ----------------------
// Stands where flush_tokens() stands in the decoder and needs the tokens' lengths only: no LZ77 execution, no window, no output.
// The path resolve left the stream's pieces in stream order in L.fl.pk; lane k owns piece k, whose tokens are neighbours in one
// scratch row, so the lane reads them four at a time (the 16-byte groups the walk stored) and sums literal ? 1 : length.  One wave
// prefix sum gives every piece its start position.  Only while the unit's length is below 32 768 can a distance reach in front of
// the first byte (a distance is at most 32 768): until then a second sweep over the same tokens, now with a running position,
// makes the decoder's "invalid distance too far back" check; the first offending token in stream order decides, and the length
// counted in front of it is what the decoder would have written.  `osize` is wave-uniform.  Returns false on that error.
__device__ CHIP_PHASE_FN bool count_tokens(WaveLds &L, const uint32_t *grow_, uint32_t ntok_, uint32_t npieces_, uint64_t &osize, int32_t &status SPEC_PARAM)
{
    const uint32_t lane = lane_id();
    GAS const uint32_t *const grow = rdfirst_gptr(grow_);
    const uint32_t ntok = rdfirst(ntok_), npieces = rdfirst(npieces_);
    if (ntok == 0) return true;
    const bool have = lane < npieces;
    const uint32_t pfirst = have ? L.fl.pk[2u * lane] : ntok;
    const uint32_t pdelta = have ? L.fl.pk[2u * lane + 1u] : 0u;
    const uint32_t pnext = lane + 1u < npieces ? L.fl.pk[2u * lane + 2u] : ntok;  // the piece ends where the next one starts
    const uint32_t k0 = (pfirst + pdelta) & 0xffffu;                               // the piece's first token in its row
    const uint32_t kend = k0 + (have ? pnext - pfirst : 0u);
    GAS const uint32_t *const row = grow + (pdelta >> 16);
    uint32_t sum = 0;
    for (uint32_t kq = k0 & ~3u; __any(kq < kend); kq += 4u) {
        if (kq < kend) {
            const u32x4 t = *(GAS const u32x4 *)(row + 8u * kq);  // kq is a multiple of 4: row_word(kq)
            const uint32_t t4[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                if (kq + j >= k0 && kq + j < kend) sum += tok_olen(t4[j]);
        }
    }
    const uint32_t incl = wave_incl_scan(sum);  // (a round's tokens give less than 64 * 256 * 258 bytes)
    const uint32_t olo = rdfirst((uint32_t)osize), ohi = rdfirst((uint32_t)(osize >> 32));
#if CHIP_INFLATE_SPEC
    if (ohi == 0 && olo < 32768u) {  // a distance may reach in front of the unit's first byte: the farthest reach is kept, nothing is refused
        uint32_t at = olo + incl - sum, reach = 0;
        for (uint32_t kq = k0 & ~3u; __any(kq < kend); kq += 4u) {
            if (kq < kend) {
                const u32x4 t = *(GAS const u32x4 *)(row + 8u * kq);
                const uint32_t t4[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (kq + j >= k0 && kq + j < kend) {
                        const uint32_t dist = __builtin_amdgcn_ubfe(t4[j], 10, 16) + 1u;
                        if ((t4[j] & 512u) != 0 && dist > at && dist - at > reach) reach = dist - at;
                        at += tok_olen(t4[j]);
                    }
            }
        }
        const uint32_t far = rdlane(wave_incl_max_scan(reach), 63u);
        if (far > sp_reach) sp_reach = far;
    }
    (void)status;
#else
    if (ohi == 0 && olo < 32768u) {
        uint32_t at = olo + incl - sum, badat = 0xffffffffu;
        for (uint32_t kq = k0 & ~3u; __any(kq < kend); kq += 4u) {
            if (kq < kend) {
                const u32x4 t = *(GAS const u32x4 *)(row + 8u * kq);
                const uint32_t t4[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (kq + j >= k0 && kq + j < kend) {
                        const bool ismatch = (t4[j] & 512u) != 0;
                        if (ismatch && __builtin_amdgcn_ubfe(t4[j], 10, 16) + 1u > at && badat == 0xffffffffu) badat = at;
                        at += tok_olen(t4[j]);
                    }
            }
        }
        const uint64_t badm = __ballot(badat != 0xffffffffu);
        if (badm) {
            osize = rdlane(badat, (uint32_t)__ffsll((long long)badm) - 1u);
            status = Z_DATA_ERROR;
            return false;
        }
    }
#endif
    osize = (((uint64_t)ohi << 32) | olo) + rdlane(incl, 63u);
    return true;
}

#if CHIP_INFLATE_MARKERS
// ---- the marker decode's executor: 16-bit elements, a plain one ------------------------------------------------------------------
// Element x of the unit's output lives at gout[x]; the element at x - d of a match that reaches in front of x = 0 is the marker
// 0x8000 | (32768 + x - d): nothing stands there in memory, the unit in front owns those elements.  64 tokens per trip (lane =
// token, found in the rows as overflow_bit() finds them): a prefix sum places them, the literals are stored at once, then the
// matches are copied in passes: the short ones whose source is final each by their own lane, the others one by one by the whole
// wave.  Between a pass's stores and the loads of the next one stands a fence of the workgroup's scope (one wave: a wait for the
// stores; the L1 is this CU's alone).
#define MSYNC() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup")
constexpr uint32_t MARK = 0x8000u, MARK_WINDOW = 32768u;
constexpr uint32_t LANE_COPY16 = 32;  // elements a lane copies for its own match; longer matches are the whole wave's

__device__ __forceinline__ void copy_match16(GAS uint16_t *gout, uint32_t x, uint32_t len, uint32_t dist)
{
    const uint32_t lane = lane_id();
    const int32_t sx = (int32_t)x - (int32_t)dist;
    for (uint32_t i = lane; i < len; i += 64) {
        // a self-overlapping match repeats its first `dist` elements; all of them lie below x and are complete
        const int32_t s = sx + (int32_t)(dist >= len ? i : small_mod(i, dist));
        const uint16_t v = s < 0 ? (uint16_t)(MARK | (uint32_t)(s + (int32_t)MARK_WINDOW)) : gout[s];
        gout[x + i] = v;
    }
    MSYNC();
}

// As flush_tokens(): executes the batch's tokens into gout (elements) at opos.  A token that does not fit `cap` elements whole stops
// the unit with CHIP_NEED_OUTPUT (a chunk of the chain ends on a token's end); a distance beyond the marker window is an error.
__device__ CHIP_PHASE_FN bool flush_tokens16(WaveLds &L, const uint32_t *grow_, uint32_t ntok_, uint32_t npieces_, uint16_t *gout_, uint32_t &opos_,
                                             uint32_t cap_, int32_t &status)
{
    const uint32_t lane = lane_id();
    GAS const uint32_t *const grow = rdfirst_gptr(grow_);
    GAS uint16_t *const gout = rdfirst_gptr(gout_);
    const uint32_t ntok = rdfirst(ntok_), npieces = rdfirst(npieces_), cap = rdfirst(cap_);
    uint32_t opos = rdfirst(opos_);
    if (ntok == 0) return true;
    const uint32_t pfirst = lane < npieces ? L.fl.pk[2u * lane] : 0xffffffffu;
    const uint32_t pdelta = lane < npieces ? L.fl.pk[2u * lane + 1u] : 0u;
    for (uint32_t g = 0; g < ntok; g += 64u) {
        const uint32_t nvalid = ntok - g < 64u ? ntok - g : 64u;
        const uint32_t t = g + lane < ntok ? g + lane : ntok - 1u;
        uint32_t k = 0;  // pieces that start at or before token t
        for (uint32_t q = 0; q < npieces; q++) k += rdlane(pfirst, q) <= t ? 1u : 0u;
        const uint32_t d = lane_gather(pdelta, k - 1u);
        const uint32_t tok = grow[(d >> 16) + row_word((t + d) & 0xffffu)];
        const bool ismatch = (tok & 512u) != 0, pair = (int32_t)tok < 0;
        const uint32_t len = tok & 0x1ffu, dist = __builtin_amdgcn_ubfe(tok, 10, 16) + 1u;
        const uint32_t olen = lane < nvalid ? tok_olen(tok) : 0u;
        const uint32_t incl = wave_incl_scan(olen);
        const uint32_t start = opos + incl - olen;
        const uint64_t validm = nvalid == 64u ? ~0ull : (1ull << nvalid) - 1ull;
        const uint64_t nofit = __ballot(olen > cap - start || start > cap) & validm;
        const uint64_t badm = __ballot(ismatch && dist > start + MARK_WINDOW) & validm;
        const uint64_t stopm = nofit | badm;
        const uint32_t nacc = stopm ? (uint32_t)__ffsll((long long)stopm) - 1u : nvalid;
        if (lane < nacc && !ismatch) gout[start] = (uint16_t)(tok & 0xffu);
        if (lane < nacc && !ismatch && pair) gout[start + 1u] = (uint16_t)((tok >> 16) & 0xffu);
        MSYNC();
        // The matches, as round_finish() takes them: every element below the first pending match is final, so every pending match
        // whose source ends there (and is short) is copied by its own lane, all of them at once; when the first pending one is not
        // among them (long, self-overlapping, or fed by a match of this pass) the whole wave copies it.
        uint64_t pend = __ballot(lane < nacc && ismatch);
        const int32_t sx = (int32_t)start - (int32_t)dist;
        while (pend) {
            const uint32_t f = (uint32_t)__ffsll((long long)pend) - 1u;
            const uint32_t wp = rdlane(start, f);
            const bool ready = ((pend >> lane) & 1ull) && len <= LANE_COPY16 && sx + (int32_t)len <= (int32_t)wp;
            const uint64_t rm = __ballot(ready);
            if (!((rm >> f) & 1ull)) {
                copy_match16(gout, wp, rdlane(len, f), rdlane(dist, f));
                pend &= pend - 1ull;
                continue;
            }
            const uint32_t n = ready ? len : 0u;
            for (uint32_t i0 = 0; __any(i0 < n); i0 += 8u) {
                uint16_t v[8];
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    const int32_t s = sx + (int32_t)(i0 + j);
                    v[j] = 0;
                    if (i0 + j < n) v[j] = s < 0 ? (uint16_t)(MARK | (uint32_t)(s + (int32_t)MARK_WINDOW)) : gout[s];
                }
#pragma unroll
                for (uint32_t j = 0; j < 8; j++)
                    if (i0 + j < n) gout[start + i0 + j] = v[j];
            }
            MSYNC();
            pend &= ~rm;
        }
        opos = nacc == 64u ? opos + rdlane(incl, 63u) : rdlane(start, nacc);
        if (stopm) {
            opos_ = opos;
            status = ((badm & ~nofit) >> nacc) & 1ull ? Z_DATA_ERROR : (int32_t)CHIP_NEED_OUTPUT;
            return false;
        }
    }
    opos_ = opos;
    return true;
}

// a stored block's payload, widened: n bytes from byte offset `so` of the unit's input to n elements at gdst
__device__ __forceinline__ void wave_copy_stored16(uint16_t *gdst, const uint32_t *g32, uint32_t so, uint32_t n)
{
    const uint8_t *gsrc = (const uint8_t *)g32 + so;
    for (uint32_t i = lane_id(); i < n; i += 64u) gdst[i] = gsrc[i];
    MSYNC();
}
#endif

// ---- a block's tokens: super-rounds of walk, path resolve, execution ------------------------------------
// Decode the tokens of one deflate block from bit `pos` on (tables are in LDS), executing them into gout.  On return `pos` is
// behind the end-of-block code (status stays ST_RUNNING) or status holds the reason decoding stopped.
// SIZES (the size pass): the tokens are counted into `osize` instead; gout, opos and cap are not used.
template <bool SIZES>
__device__ CHIP_PHASE_FN void decode_block(WaveLds &L, InWin &w, uint32_t &pos, const uint32_t end_bit, uint8_t *gout, uint32_t &opos,
                                           const uint32_t cap, int32_t &status, uint32_t *rows, const uint32_t xt_bits, const uint32_t eob_len,
                                           const uint32_t flags, uint64_t &osize STAT_PARAM SPEC_PARAM)
{
    pos = rdfirst(pos);
    opos = rdfirst(opos);
    for (;;) {
        if (pos >= end_bit) {
            status = CHIP_NEED_INPUT;
            return;
        }
        STAT_T0();
        uint32_t ntok = 0, why = 0, tpos = 0;
        const uint32_t npk = walk_round(L, w, pos, end_bit, rows, xt_bits, ntok, why, tpos STAT_ARG);
        int32_t st2 = ST_RUNNING;
        bool flushed = true;
        uint32_t ovf[3] = {0, 0, 0};
#ifdef CHIP_EXP_NO_FLUSH  // ablation (no output): the walk alone -- header, tables, walk, path resolve, token rows
        asm volatile("" ::"s"(npk), "s"(ntok));
#else
        if constexpr (SIZES) {
            if (npk) flushed = count_tokens(L, rows, ntok, npk, osize, st2 SPEC_ARG);
        } else {
#if CHIP_INFLATE_MARKERS
            if (npk) flushed = flush_tokens16(L, rows, ntok, npk, (uint16_t *)gout, opos, cap, st2);
#else
            if (npk) flushed = flush_tokens(L, rows, ntok, npk, gout, opos, cap, st2, ovf STAT_ARG);
#endif
        }
#endif
        w.win0 = 0xffffffffu;  // the phases used the header window's place
        STAT_ACC(20);
        if (!flushed) {
            status = st2;
            // CHIP_F_COMPU_STATUS: zlib's position when the output filled (else the position stays at the round's start)
            if (!SIZES && (flags & F_COMPU_STATUS) && st2 == CHIP_NEED_OUTPUT) pos = overflow_bit(L, w, rows, ntok, npk, ovf[0], ovf[1], ovf[2], pos);
            return;
        }
        if (why == R_NEED_INPUT) {
            status = CHIP_NEED_INPUT;
            return;
        }
        if (why == R_EOB) {
            pos = tpos + eob_len;
            return;
        }
        if (why != R_LIMIT || tpos <= pos) {  // invalid code (a super-round always gets past its first token otherwise)
            status = Z_DATA_ERROR;
            return;
        }
        pos = tpos;  // on from where the true stream stopped
    }
}

#ifndef CHIP_WAVES_PER_SIMD
#define CHIP_WAVES_PER_SIMD 5  // (18 waves per CU: two SIMDs hold five; 96 lane registers)
#endif
// one unit, start to finish, by the calling wave; scratch = the wave's token rows in HBM
// SIZES (the size pass, chip_decode_batch_sizes): the same unit loop, wrapper, block headers, table builds and walk, but nothing is
// written: the decoded length is counted in 64 bits and goes to out_size[u]; the unit's output description is never read.
// CHIP_INFLATE_MEMBERS (inflate_members.hip, CHIP_F_MEMBERS): a gzip member that ends with CHIP_FINISHED and has `1f 8b` behind its
// trailer is followed by the next one (the walk of include/compu_hip.h): the output base and the room move past the member, the
// member's state (wrapper, tables, block flags, output position) starts over, the input position goes on where it stands.  Every
// check that is relative to the output base -- a distance "too far back", CRC-32, ISIZE -- thereby becomes the member's own.  The
// code of the member loop is compiled only there: without the macro this file's tokens are what they were.
#ifndef CHIP_INFLATE_MEMBERS
#define CHIP_INFLATE_MEMBERS 0
#endif
// CHIP_INFLATE_INDEX (inflate_index.hip, chip_inflate_index_build): the unit loop records the block boundaries that are points of
// the checkpoint index (the walk of include/compu_hip.h) -- lane 0's stores of (bit, out) into the launch's point list, a count, and
// the bit behind the final block.  Compiled only there, as the member loop is.
#ifndef CHIP_INFLATE_INDEX
#define CHIP_INFLATE_INDEX 0
#endif
#if CHIP_INFLATE_INDEX
struct IndexRec {
    uint64_t *pt_bit, *pt_out;  // the first max_points points (device arrays of the caller, may be null with max_points == 0)
    uint64_t max_points;
    uint32_t spacing;           // >= 1
    uint32_t *walk;             // [0] the points of the whole walk, [1] the bit behind the final block (0: the unit did not finish),
                                // [2] the wrapper kind the unit turned out to have
};
#define INDEX_PARAM , const IndexRec &ix
#else
#define INDEX_PARAM
#endif
#if CHIP_INFLATE_SPEC
// how a unit of the speculative size pass ended, and what it found
enum : uint32_t { SPEC_RAN = 0, SPEC_LINKED = 1, SPEC_GAVE_UP = 2 };  // RAN: to the status it answers (finished, error, end of input)
constexpr uint32_t SPEC_PASS_MAX = 8;  // starts a unit walks over without linking before it gives up
struct SpecOut {
    uint64_t size;     // decoded length
    uint64_t end_bit;  // of the stream: the boundary it linked at; the bit behind the final block; else the last boundary reached
    uint32_t kind, link;  // SPEC_*; LINKED: the unit it linked to (1 + the start's index)
    int32_t status;
    uint32_t reach;    // the farthest a match reached in front of the unit's first byte
    uint32_t wrap, first_bit;  // unit 0: the wrapper kind, the bit of the first block header
};
struct SpecRec {
    const uint64_t *starts;  // the finder's answer, ascending; unit u >= 1 begins at starts[u - 1], unit 0 at the stream's beginning
    uint32_t n_starts;
    SpecOut *out;            // one per unit
    uint32_t bit0 = 0;       // unit 0: the bit of its first byte it begins at (a stream taken up at a block boundary: no wrapper, raw format)
};
#define SPEC_REC_PARAM , const SpecRec &sp
#else
#define SPEC_REC_PARAM
#endif
#if CHIP_INFLATE_MARKERS
#define MARK_PARAM , const uint32_t *mk_bit0  // per unit: the bit of its first block header in its first input byte
#else
#define MARK_PARAM
#endif
template <bool SIZES>
__device__ __attribute__((always_inline)) void inflate_unit(const BatchArgs &a, const uint32_t u, WaveLds &L, uint32_t *scratch, uint64_t *out_size INDEX_PARAM SPEC_REC_PARAM MARK_PARAM)
{
    const uint32_t lane = lane_id();

    const uint8_t *gin = a.in_base + a.in_off[u];
    const uint32_t in_len = a.in_len[u];
    uint8_t *gout = nullptr;
    uint32_t cap_ = 0xffffffffu;
    if constexpr (!SIZES) {
        gout = a.out_base + a.out_off[u];
        cap_ = a.out_cap[u];
    }
#if CHIP_INFLATE_MEMBERS
    uint32_t cap = cap_;        // room left behind the finished members
    uint32_t opos_members = 0;  // output bytes of the finished members
    uint64_t osize_members = 0;
#else
    const uint32_t cap = cap_;
#endif
    uint64_t osize = 0;  // SIZES: the decoded length so far

    InWin w;
    const uint32_t mis = (uint32_t)((uintptr_t)gin & 3u);
    w.g32 = (const uint32_t *)(gin - mis);
    w.total_dw = (mis + in_len + 3u) >> 2;
    w.win0 = 0xffffffffu;
    const uint32_t start_bit = mis * 8u;
    const uint32_t end_bit = start_bit + in_len * 8u;

    uint32_t pos = start_bit;
    uint32_t opos = 0;
    int32_t status = ST_RUNNING;
    bool last = false;
    int tables = 0;  // 0 none, 1 fixed, 2 dynamic
    uint32_t eob_len = 0;   // length of the block's end-of-block code

    STAT_DECL;
    STAT_T0();
    uint32_t wrap = 0;
    int32_t format = a.format;
    uint32_t ck_bit = 0, ck_opos = 0;  // last block boundary reached (streaming decoder: where the next call resumes)
    bool resumed = false;
    uint32_t run_check = 0, run_cov = 0, out_dropped = 0;  // running trailer check: value, stream bytes covered; bytes dropped in front
#if CHIP_INFLATE_INDEX
    uint32_t ix_n = 0, ix_out = 0, ix_end = 0;  // points so far, the last point's output count, the bit behind the final block
#endif
    if (!SIZES && a.resume) {
        const uint32_t *rs = a.resume + RESUME_WORDS * u;
        const uint32_t r0 = rs[0], r1 = rs[1], r2 = rs[2];
        if (r0 != 0 && r0 <= in_len * 8u && r1 <= cap) {
            resumed = true;
            pos = start_bit + r0;
            opos = r1;
            wrap = r2 & 3u;
            ck_bit = r0;
            ck_opos = r1;
            run_check = rs[3];
            run_cov = rs[4];
            out_dropped = rs[5];
        }
    }
#if CHIP_INFLATE_SPEC
    uint32_t sp_next = u;  // the first start behind the unit's own
    uint32_t sp_passed = 0, sp_kind = SPEC_RAN, sp_link = 0, sp_reach = 0, sp_first = 0, sp_end = 0;
    const uint64_t sp_bit0 = 8ull * a.in_off[u];  // the unit's first byte in bits of the stream
    if (u) {
        resumed = true;  // no wrapper: a block header, at the bit the start names
        pos = start_bit + (uint32_t)(sp.starts[u - 1u] & 7u);
    } else {
        pos += sp.bit0;
    }
#endif
#if CHIP_INFLATE_MARKERS
    resumed = true;
    pos = start_bit + mk_bit0[u];
#endif
#if CHIP_INFLATE_MEMBERS
next_member:
#endif
    if (!resumed && format != CHIP_FMT_DEFLATE) {
        uint32_t hdr = 0;
#if CHIP_INFLATE_MEMBERS
        const uint32_t k0 = (pos - start_bit) >> 3;  // (a member starts at a byte: 0, or behind a trailer)
        status = parse_wrapper((LDS_AS uint32_t *)&L, gin + k0, in_len - k0, format, wrap, hdr);
#else
        status = parse_wrapper((LDS_AS uint32_t *)&L, gin, in_len, format, wrap, hdr);
#endif
        status = (int32_t)rdfirst((uint32_t)status);
        wrap = rdfirst(wrap);
        pos += rdfirst(hdr) * 8u;
    }
    if (status == ST_RUNNING) win_load(L, w, pos >> 5);
#if CHIP_INFLATE_SPEC
    sp_first = pos - start_bit;
#endif

    __builtin_amdgcn_s_setprio(2);
    while (status == ST_RUNNING) {
        if (last) {
#if CHIP_INFLATE_INDEX
            ix_end = pos - start_bit;
#endif
#if CHIP_INFLATE_SPEC
            sp_end = pos - start_bit;
#endif
            status = CHIP_FINISHED;
            break;
        }
        ck_bit = pos - start_bit;
        ck_opos = opos;
#if CHIP_INFLATE_INDEX
        if (ix_n == 0 || opos - ix_out >= ix.spacing) {  // (uniform) this boundary is a point
            if (lane == 0 && ix_n < ix.max_points) {
                ix.pt_bit[ix_n] = ck_bit;
                ix.pt_out[ix_n] = opos;
            }
            ix_out = opos;
            ix_n++;
        }
#endif
#if CHIP_INFLATE_SPEC
        {  // (uniform) is this boundary a start behind the unit's own?
            const uint64_t b = sp_bit0 + ck_bit;
            while (sp_next < sp.n_starts && sp.starts[sp_next] < b) sp_next++, sp_passed++;
            if (sp_next < sp.n_starts && sp.starts[sp_next] == b) {
                sp_kind = SPEC_LINKED;
                sp_link = sp_next + 1u;
                break;
            }
            if (sp_passed > SPEC_PASS_MAX) {
                sp_kind = SPEC_GAVE_UP;
                break;
            }
        }
#endif
        win_ensure(L, w, pos);
        if (pos + 3 > end_bit) {
            status = CHIP_NEED_INPUT;
            break;
        }
        uint32_t lo, hi;
        win_bits_uniform(L, w, pos, lo, hi);
        last = lo & 1u;
        uint32_t type = (lo >> 1) & 3u;
        pos += 3;
        if (type == 0) {
            // stored block, RFC 1951 sec. 3.2.4
            pos = (pos + 7u) & ~7u;
            if (pos + 32 > end_bit) {
                status = CHIP_NEED_INPUT;
                break;
            }
            win_ensure(L, w, pos);
            win_bits_uniform(L, w, pos, lo, hi);
            uint32_t blen = lo & 0xffffu, nlen = lo >> 16;
            if (blen != (nlen ^ 0xffffu)) {
                status = Z_DATA_ERROR;
                break;
            }
            pos += 32;
            uint32_t avail = (end_bit - pos) >> 3;
            uint32_t ncopy = blen < avail ? blen : avail;
            if constexpr (SIZES) {
                osize += ncopy;  // LEN bytes are skipped
            } else {
                uint32_t room = cap - opos;
                if (ncopy > room) ncopy = room;
#if CHIP_INFLATE_MARKERS
                wave_copy_stored16((uint16_t *)gout + opos, w.g32, pos >> 3, ncopy);
#else
                wave_copy_stored(gout + opos, w.g32, w.total_dw, pos >> 3, ncopy);
#endif
                opos += ncopy;
            }
            pos += ncopy * 8u;
            if (ncopy < blen) {
                // zlib reports Z_OK here; compu calls it NeedInput when no input is left (mod.rs:476-479)
                status = ncopy == avail ? CHIP_NEED_INPUT : CHIP_NEED_OUTPUT;
                break;
            }
            continue;
        }
        if (type == 3) {
            status = Z_DATA_ERROR;
            break;
        }
        uint32_t nlen = 288, ndist = 32;
        bool build = true;
        if (type == 1) {
            if (tables != 1) {  // RFC 1951 sec. 3.2.6 (a run of fixed blocks keeps its tables)
                for (uint32_t s = lane; s < 320; s += 64) L.hdr.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
                WSYNC();
                tables = 1;
            } else build = false;
        } else {
            // dynamic block header, RFC 1951 sec. 3.2.7
            tables = 2;
            if (pos + 14 > end_bit) {
                status = CHIP_NEED_INPUT;
                break;
            }
            win_ensure(L, w, pos);
            win_bits_uniform(L, w, pos, lo, hi);
            nlen = (lo & 31u) + 257;
            ndist = ((lo >> 5) & 31u) + 1;
            const uint32_t ncode = ((lo >> 10) & 15u) + 4;
            pos += 14;
            if (nlen > 286 || ndist > 30) {
                status = Z_DATA_ERROR;
                break;
            }
            if (pos + 3 * ncode > end_bit) {
                status = CHIP_NEED_INPUT;
                break;
            }
            win_ensure(L, w, pos, 128);
            if (lane < 19) L.hdr.lens[lane] = 0;
            WSYNC();
            if (lane < ncode) {
                static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                uint32_t l2, h2;
                win_bits(L, w, pos + 3 * lane, l2, h2);
                L.hdr.lens[order[lane]] = (uint8_t)(l2 & 7u);
            }
            WSYNC();
            pos += 3 * ncode;
            if (build_cl_table(L STAT_ARG)) {
                status = Z_DATA_ERROR;
                break;
            }
            // Code lengths of the two alphabets, 64 bit positions per round: lane i decodes the code-length symbol
            // that would start at bit pos + i; the symbols really present are the chain 0 -> 0 + bits(0) -> ...,
            // found by pointer doubling; a prefix sum of the run lengths along the chain gives every symbol
            // its place in lens[], and a running maximum hands each "repeat previous" symbol the last explicit
            // length in front of it.  (zlib reads these one by one; errors keep its order: the first bad symbol.)
            uint32_t have = 0, total = nlen + ndist, prevlen = 0;
            win_ensure(L, w, pos, 316 * 14 + 160);
            static_assert(offsetof(WaveLds, hdr.lens) % 4 == 0 && sizeof(L.hdr.lens) == 320, "lens[] is zeroed a dword at a time");
            for (uint32_t k = lane; k < 320 / 4; k += 64) ((uint32_t *)L.hdr.lens)[k] = 0;  // zero runs (17/18) then need no stores
            WSYNC();
            while (have < total) {
                STAT_ADD(7, 1);
                const uint32_t bp = pos + lane;
                uint32_t lo, hi;
                win_bits(L, w, bp, lo, hi);
                const uint32_t e = L.hdr.cl_lut[lo & 127u];
                const uint32_t cl = e & 15u, sym = e >> 16;
                const uint32_t eb = sym < 16 ? 0u : sym == 16 ? 2u : sym == 17 ? 3u : 7u;
                const uint32_t tl = cl + eb;
                const uint32_t run = sym < 16 ? 1u : (sym == 18 ? 11u : 3u) + bfe(lo, cl, eb);
                const uint32_t nx = lane + tl;
                // The symbols really present start at 0, nx(0), nx(nx(0)), ...: lane n finds the n-th of these positions (powers of nx
                // by doubling, composed along the bits of n; 64 = the chain has left the 64 positions) and flags it.  (Measured and
                // not kept, profiles/block_headers_ab.md: fewer doubling steps by the shortest code, the chain followed with scalar
                // lane reads, flags pushed through LDS with one gather per step.)
                uint32_t nth = 0;
                {
                    uint32_t pw = nx < 64u ? nx : 64u;
#pragma unroll
                    for (int r = 0; r < 6; r++) {
                        const uint32_t g1 = lane_gather(pw, nth & 63u), g2 = lane_gather(pw, pw & 63u);
                        if ((lane >> r) & 1u) nth = nth < 64u ? g1 : 64u;
                        pw = pw < 64u ? g2 : 64u;
                    }
                }
                uint8_t *const onflag = (uint8_t *)L.hdr.count;  // 64 bytes (the counts are not in use here)
                if (lane < 16) L.hdr.count[lane] = 0;
                LSYNC();
                if (nth < 64u) onflag[nth] = 1;
                LSYNC();
                const bool on = onflag[lane] != 0;
                const uint32_t c = on ? run : 0u;
                const uint32_t incl = wave_incl_scan(c);
                const uint32_t start = have + incl - c;
                const bool need = on && start < total;
                uint32_t bad = 0;  // zlib's checks, in its order, for the symbol this lane holds
                if (need && bp + tl > end_bit) bad = 1;
                else if (need && sym == 16 && start == 0) bad = 2;
                else if (need && sym >= 16 && start + run > total) bad = 2;
                const uint64_t badm = __ballot(bad != 0);
                const uint32_t fb = badm ? (uint32_t)__ffsll((long long)badm) - 1u : 64u;
                const bool ok = need && lane < fb;
                const uint32_t expl = sym < 16 ? sym : 0u;  // the length this symbol leaves as "previous"
                const uint32_t m = wave_incl_max_scan((ok && sym != 16) ? (((lane + 1u) << 8) | expl) : 0u);
                const uint32_t v = sym == 16 ? (m ? m & 0xffu : prevlen) : expl;
                if (ok && sym < 16) L.hdr.lens[start] = (uint8_t)sym;
                if (ok && sym == 16)
                    for (uint32_t j = 0; j < run; j++) L.hdr.lens[start + j] = (uint8_t)v;
                if (badm) {
                    status = rdlane(bad, fb) == 1 ? (int32_t)CHIP_NEED_INPUT : Z_DATA_ERROR;
                    break;
                }
                const uint64_t okm = __ballot(ok);
                const uint32_t lv = 63u - (uint32_t)__clzll((long long)okm);  // lane 0 is always ok here
                have = rdlane(start + run, lv);
                pos += lv + rdlane(tl, lv);
                prevlen = rdlane(v, lv);
            }
            if (status != ST_RUNNING) break;
            WSYNC();
            STAT_ACC(4);
            if (rdfirst(L.hdr.lens[256]) == 0) {
                status = Z_DATA_ERROR;
                break;
            }
        }
        if (build) {
            eob_len = rdfirst(L.hdr.lens[256]);
            uint32_t used = 0;
            const int r1 = build_litlen(L, L.hdr.lens, (int)nlen, used STAT_ARG);
            const int r2 = r1 ? r1 : build_dist(L, L.hdr.lens + nlen, (int)ndist, used STAT_ARG);
            if (r1 || r2) {  // an invalid set of code lengths (the pool cannot overflow: see POOL_WORDS)
                status = Z_DATA_ERROR;
                break;
            }
            STAT_ACC(5);
        }
        STAT_ACC(0);
        __builtin_amdgcn_s_setprio(0);
        decode_block<SIZES>(L, w, pos, end_bit, gout, opos, cap, status, scratch, tables == 1 ? XT_BITS_FIXED : XT_BITS, eob_len, a.flags, osize STAT_ARG SPEC_ARG);
        __builtin_amdgcn_s_setprio(2);  // block headers and table builds are short dependent chains: ahead of the other waves' bulk work
        STAT_T0();
    }
    __builtin_amdgcn_s_setprio(0);
    STAT_ACC(0);
    if (SIZES && status == CHIP_FINISHED && wrap) {
        // trailer, without the check that needs the decoded bytes (Adler-32 / CRC-32): its presence, and gzip's ISIZE against
        // the counted length.  The decoder's order is 4 bytes present, CRC, 8 bytes present, ISIZE; without the CRC step the two
        // presence checks are one, so a gzip unit with a wrong CRC AND a cut or wrong ISIZE reads CHIP_NEED_INPUT / length error
        // here where the decoder reports the data check first (rule 2's exemption)
        uint32_t k = (pos - start_bit + 7u) >> 3;
        if (wrap == 1) {
            if (in_len - k < 4) status = CHIP_NEED_INPUT;
            k += 4;
        } else {
            if (in_len - k < 8) status = CHIP_NEED_INPUT;
            else {
                uint32_t isize = gin[k + 4] | ((uint32_t)gin[k + 5] << 8) | ((uint32_t)gin[k + 6] << 16) | ((uint32_t)gin[k + 7] << 24);
                if (rdfirst(isize) != (uint32_t)osize) status = Z_DATA_ERROR;  // incorrect length check
            }
            k += 8;
        }
        pos = start_bit + k * 8u;
    }
    if (!SIZES && status == CHIP_FINISHED && wrap) {
        // trailer: gzip CRC-32 + ISIZE (little endian), zlib Adler-32 (big endian)
        uint32_t k = (pos - start_bit + 7u) >> 3;
        uint32_t need = wrap == 2 ? 8u : 4u;
        if (in_len - k < need && wrap == 1) {
            status = CHIP_NEED_INPUT;
        } else if (wrap == 1) {
            uint32_t want = ((uint32_t)gin[k] << 24) | ((uint32_t)gin[k + 1] << 16) | ((uint32_t)gin[k + 2] << 8) | gin[k + 3];
            const uint32_t c0 = run_cov - out_dropped;  // offset the running value (seed) covers up to; 0 and seed 1 for a whole stream
            if (rdfirst(wave_adler32(gout + c0, opos - c0, resumed ? run_check : 1u)) != rdfirst(want)) status = Z_DATA_ERROR;  // incorrect data check
            k += 4;
        } else if (in_len - k < 4) {
            status = CHIP_NEED_INPUT;
        } else {
            uint32_t want = gin[k] | ((uint32_t)gin[k + 1] << 8) | ((uint32_t)gin[k + 2] << 16) | ((uint32_t)gin[k + 3] << 24);
            const uint32_t c0 = run_cov - out_dropped;
            if (rdfirst(wave_crc32((LDS_AS uint32_t *)&L, gout + c0, opos - c0, resumed ? run_check : 0u)) != rdfirst(want)) status = Z_DATA_ERROR;  // incorrect data check
            else if (in_len - k < 8) status = CHIP_NEED_INPUT;
            else {
                uint32_t isize = gin[k + 4] | ((uint32_t)gin[k + 5] << 8) | ((uint32_t)gin[k + 6] << 16) | ((uint32_t)gin[k + 7] << 24);
                if (rdfirst(isize) != out_dropped + opos) status = Z_DATA_ERROR;  // incorrect length check
            }
            k += 8;
        }
        pos = start_bit + k * 8u;
    }
#if CHIP_INFLATE_MEMBERS
    if (status == CHIP_FINISHED && wrap == 2) {
        const uint32_t k = (pos - start_bit) >> 3;
        if (in_len - k >= 2 && rdfirst(gin[k]) == 0x1fu && rdfirst(gin[k + 1]) == 0x8bu) {  // another member starts here
            WSYNC();  // (the checksum's tables took the whole LDS; every lane is done with them)
            if constexpr (SIZES) {
                osize_members += osize;
                osize = 0;
            } else {
                gout += opos;
                cap -= opos;
                opos_members += opos;
                opos = 0;
            }
            format = CHIP_FMT_GZIP;
            status = ST_RUNNING;
            last = false;
            tables = 0;
            w.win0 = 0xffffffffu;
            goto next_member;
        }
    }
    opos += opos_members;  // (nothing below reads the output)
    osize += osize_members;
#endif
    STAT_ACC(6);
#ifdef CHIP_STATS
    if (a.stats && lane == 0)
        for (int k = 0; k < 24; k++) a.stats[(size_t)u * 24 + k] = st_[k];
#endif
    if (!SIZES && a.resume) {
        // the stream goes on in a later call: bring the running check up to the boundary it will resume from (the bytes in
        // front of it are final; the caller may drop them once it has handed them on)
        const bool cont = status == CHIP_NEED_INPUT || status == CHIP_NEED_OUTPUT;
        uint32_t *rs = a.resume + RESUME_WORDS * u;
        if (!resumed) run_check = wrap == 1 ? 1u : 0u;
        const uint32_t c0 = run_cov - out_dropped;
        if (cont && wrap && ck_bit != 0 && ck_opos > c0) {
            run_check = wrap == 1 ? wave_adler32(gout + c0, ck_opos - c0, run_check) : wave_crc32((LDS_AS uint32_t *)&L, gout + c0, ck_opos - c0, run_check);
            run_cov = out_dropped + ck_opos;
        }
        if (lane == 0) {
            rs[0] = cont ? ck_bit : 0u;
            rs[1] = cont ? ck_opos : 0u;
            rs[2] = wrap;
            rs[3] = run_check;
            rs[4] = run_cov;
            rs[5] = out_dropped;
        }
    }
    uint32_t used = (pos - start_bit + 7u) >> 3;
    if (used > in_len) used = in_len;
    if (!SIZES && (a.flags & F_COMPU_STATUS)) {
        // compu's reading of zlib's return code, src/decoder/mod.rs:475-483: Z_OK with avail_in == 0 is NeedInput whatever
        // else ran out, and a call that could not move (no input at all: Z_BUF_ERROR) is NeedOutput
        if (status == CHIP_NEED_OUTPUT && used == in_len) status = CHIP_NEED_INPUT;
        else if (status == CHIP_NEED_INPUT && in_len == 0) status = CHIP_NEED_OUTPUT;
    }
#if CHIP_INFLATE_INDEX
    if (lane == 0) {
        ix.walk[0] = ix_n;
        ix.walk[1] = status == CHIP_FINISHED ? ix_end : 0u;
        ix.walk[2] = wrap;
    }
#endif
#if CHIP_INFLATE_SPEC
    if (lane == 0)
        sp.out[u] = SpecOut{osize, sp_bit0 + (status == CHIP_FINISHED ? sp_end : ck_bit), sp_kind, sp_link, status, sp_reach, wrap, sp_first};
#endif
    if (lane == 0) {
        if constexpr (SIZES) out_size[u] = osize;
        else a.out_len[u] = opos;
        a.in_used[u] = status == CHIP_NEED_INPUT ? in_len : used;
        a.status[u] = status;
    }
}

}  // namespace chip
