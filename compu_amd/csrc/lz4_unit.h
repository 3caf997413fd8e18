// The device code of the batched LZ4 decode for gfx950 (MI355X), shared by the decode kernel and the size kernel of lz4.hip: one
// wavefront decodes one unit, a raw block (CHIP_FMT_LZ4_BLOCK) or a frame (CHIP_FMT_LZ4).  DESIGN.md sec. 4.26.
//
// A block is a chain of sequences (token, length extensions, literals, offset, length extensions): where a sequence starts is known
// only once the one in front of it has been parsed.  That chain is the only serial part.  The wave parses it wave-uniformly, in
// scalar registers, out of a 2 KiB window of the input staged in LDS (lz4_core.h's parse_seq, the same code as the host decoder
// runs), 64 sequences at a time: lane k keeps sequence k's literal source, lengths, offset and destinations.  Every verdict --
// truncation, offsets, the room, the block maximum -- depends on positions only, so the parse alone decides status, out_len and
// in_used, and the size pass is the parse without the copies.
// Then the group is executed wave-wide.  Phase A copies the literal bytes of all 64 sequences, 256 per step: their sources are
// input bytes, so nothing orders them.  Phase B copies the matches in steps of up to 256 bytes: a step takes the longest run of
// consecutive matches none of which reads a byte at or behind the first one's destination (the dependency rule of the zstd
// executor, zstd_unit.h), so that all loads of a step are issued before its first store.  In both phases a byte finds its
// sequence through a byte-wide owner map scattered into LDS and a running maximum across the wave.  A match whose offset is below
// its length replicates a period: byte i reads byte i % offset of the period.  Literal runs of 64 bytes and more are copied when
// they are parsed, 16 bytes per lane; matches above 256 bytes go one at a time in their turn, a byte per lane and trip.
// A wave's global stores are seen by its later loads in program order (the lanes of one wave share the CU's L1), so no step waits
// for its stores to be acknowledged.
// LDS: 5 376 bytes per wave (window 2 KiB, owner map 256 B, parameters 1 KiB, XXH32 staging 2 KiB), which never limits the occupancy.
// Registers (hipcc 7, the kernels' metadata): the decode kernel 80 VGPRs, no scratch: 6 waves per SIMD; the size kernel 32 VGPRs: 8
// waves per SIMD.
#pragma once
#include "chip_internal.h"
#include "lz4_core.h"

namespace chip {

namespace {

constexpr uint32_t LZ4_WIN = 2048;        // bytes of input staged in LDS
constexpr uint32_t LZ4_LONG_LIT = 64;     // literal runs from here on are copied when they are parsed
constexpr uint32_t LZ4_LONG_MATCH = 256;  // matches above this are copied on their own
constexpr uint32_t LZ4_STAGE = 512;       // dwords of XXH32 staging: 128 stripes

struct Lz4Lds {
    uint32_t win[LZ4_WIN / 4];
    uint32_t heads[64];    // owner map of a step: 256 bytes, lane + 1 of the sequence whose run starts at that byte
    uint32_t par[64 * 4];  // per sequence: destination, source / offset, bytes in front of it in the group, length
    uint32_t stage[LZ4_STAGE];
};

struct __attribute__((packed, aligned(1))) Lz4U32 {
    uint32_t v;
};
typedef uint32_t lz4_u32x4 __attribute__((ext_vector_type(4)));
typedef lz4_u32x4 Lz4U128 __attribute__((aligned(1)));  // 16 bytes at any address (gfx950 does unaligned global accesses)

// Fills the window with the aligned dwords from in + base on (base: a unit position, in + base 4-byte aligned, possibly -3 .. -1);
// dwords that hold no byte of the unit are not loaded.  Out of line: the parse reaches it from every byte it reads, and inlined
// there it was most of the kernels' code.
__device__ __attribute__((noinline)) void lz4_refill(LDS_AS uint32_t *win, const GAS uint8_t *in, uint32_t len, int64_t base)
{
    const uint32_t lane = lane_id();
    LSYNC();
#pragma unroll
    for (uint32_t k = 0; k < LZ4_WIN / 256; k++) {
        const int64_t pos = base + 4 * (int64_t)(lane + 64u * k);
        uint32_t v = 0;
        if (pos < (int64_t)len) v = *(const GAS uint32_t *)(in + pos);
        win[lane + 64u * k] = v;
    }
    LSYNC();
}

// The unit's input through the LDS window.  Positions are offsets into the unit; everything here is wave-uniform.
struct Lz4Reader {
    LDS_AS uint8_t *win;
    const GAS uint8_t *in;
    uint32_t len;   // of the unit: loads stay inside the aligned dwords that hold bytes of it
    int64_t base;   // the window holds unit positions [base, base + LZ4_WIN); base may be -3 .. -1 (an aligned dword in front)
    __device__ __forceinline__ uint32_t byte(uint64_t q)
    {
        if ((uint64_t)((int64_t)q - base) >= LZ4_WIN) {
            base = (int64_t)q - (int64_t)((uintptr_t)(in + q) & 3u);
            lz4_refill((LDS_AS uint32_t *)win, in, len, base);
        }
        return rdfirst(win[(uint32_t)((int64_t)q - base)]);
    }
};

// forward copy of n bytes between disjoint ranges by the whole wave: 16 bytes per lane and trip at any alignment
__device__ __forceinline__ void lz4_wave_copy(GAS uint8_t *dst, const GAS uint8_t *src, uint32_t n)
{
    const uint32_t lane = lane_id(), whole = n & ~15u;
    for (uint32_t j = 16u * lane; j < whole; j += 1024u) {
        const Lz4U128 v = *(const GAS Lz4U128 *)(src + j);
        *(GAS Lz4U128 *)(dst + j) = v;
    }
    if (whole + lane < n) dst[whole + lane] = src[whole + lane];
}

// one long match by the whole wave, a byte per lane and trip; trips of 64 bytes never read what the same trip writes
__device__ __forceinline__ void lz4_wave_match(GAS uint8_t *dst, uint32_t offset, uint32_t n)
{
    const uint32_t lane = lane_id();
    const GAS uint8_t *src = dst - offset;
    if (offset >= 64) {
        for (uint32_t b = 0; b < n; b += 64) {
            const uint32_t j = b + lane;
            if (j < n) dst[j] = src[j];
        }
    } else {
        for (uint32_t j = lane; j < n; j += 64) dst[j] = src[j % offset];  // every byte is one of the `offset` bytes before dst
    }
}

// XXH32 (seed 0 in the frame format, any seed in chip_xxh32_batch) of p[0 .. n) on one wave.  The accumulator recurrence
// acc = rotl(acc + in * P2, 13) * P1 is serial per 4-byte column, the products in * P2 are not: all 64 lanes form them for up to 128
// stripes at a time into `stage`, then lanes 0..3 run their columns over the staged products.
__device__ __attribute__((noinline, unused)) uint32_t wave_xxh32(uint32_t *stage_, const uint8_t *p_, uint64_t n, uint32_t seed)
{
    LDS_AS uint32_t *const stage = (LDS_AS uint32_t *)stage_;
    const GAS uint8_t *const p = (const GAS uint8_t *)p_;
    const uint32_t lane = lane_id();
    uint32_t acc = lane == 0 ? seed + lz4::XP1 + lz4::XP2 : lane == 1 ? seed + lz4::XP2 : lane == 2 ? seed : seed - lz4::XP1;
    const uint64_t stripes = n >> 4;
    for (uint64_t s0 = 0; s0 < stripes; s0 += LZ4_STAGE / 4) {
        const uint32_t ns = stripes - s0 < LZ4_STAGE / 4 ? (uint32_t)(stripes - s0) : LZ4_STAGE / 4;
        LSYNC();
        uint32_t in[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t q = 64u * k + lane;  // dword of the batch: stripe q / 4, column q % 4
            in[k] = q < 4u * ns ? ((const GAS Lz4U32 *)(p + 16u * s0 + 4u * q))->v : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t q = 64u * k + lane;
            if (q < 4u * ns) stage[q] = in[k] * lz4::XP2;
        }
        LSYNC();
        if (lane < 4)
            for (uint32_t i = 0; i < ns; i++) acc = lz4::rotl32(acc + stage[4u * i + lane], 13) * lz4::XP1;
    }
    LSYNC();
    uint32_t h;
    if (n >= 16) h = lz4::rotl32(rdlane(acc, 0), 1) + lz4::rotl32(rdlane(acc, 1), 7) + lz4::rotl32(rdlane(acc, 2), 12) + lz4::rotl32(rdlane(acc, 3), 18);
    else h = seed + lz4::XP5;
    h += (uint32_t)n;
    // the tail, below 16 bytes: every lane runs the same few steps over the same bytes
    lz4::MemReader rd{p_ + (stripes << 4)};
    return rdfirst(lz4::xxh32_tail(rd, 0, (uint32_t)(n & 15u), h));
}

// What one unit's decode keeps across blocks; wave-uniform.
template <bool SIZES>
struct Lz4Unit {
    Lz4Lds &L;
    Lz4Reader rd;
    const GAS uint8_t *in;
    GAS uint8_t *out;
    uint64_t cap;  // NO_LIMIT in the size pass
    uint64_t o;    // bytes produced

    // Executes the group: lane k < cnt holds sequence k.  lit_pos / ll: the literal run still to copy (ll == 0 where it was copied
    // at parse time); ldst its destination; ml, off, mdst the match.
    __device__ void execute(uint32_t lit_pos, uint32_t ll, uint32_t ldst, uint32_t ml, uint32_t off, uint32_t mdst)
    {
        const uint32_t lane = lane_id();
        // ---- phase A: the literal bytes of the group, 256 per step --------------------------------------------------------------
        {
            const uint32_t lbi = wave_incl_scan(ll), lbx = lbi - ll, LB = rdlane(lbi, 63);
            if (LB) {
                LSYNC();
                L.par[4 * lane] = ldst;
                L.par[4 * lane + 1] = lit_pos;
                L.par[4 * lane + 2] = lbx;
                uint32_t carry = 0;
                for (uint32_t wb = 0; wb < LB; wb += 256) {
                    L.heads[lane] = 0;
                    LSYNC();
                    if (ll && lbx >= wb && lbx < wb + 256) ((LDS_AS uint8_t *)L.heads)[lbx - wb] = (uint8_t)(lane + 1);
                    LSYNC();
                    const uint32_t h = L.heads[lane];
                    uint32_t r[4] = {h & 0xffu, (h >> 8) & 0xffu, (h >> 16) & 0xffu, h >> 24};
                    r[1] = r[1] > r[0] ? r[1] : r[0];
                    r[2] = r[2] > r[1] ? r[2] : r[1];
                    r[3] = r[3] > r[2] ? r[3] : r[2];
                    uint32_t cin = wave_shr1(wave_incl_max_scan(r[3]));
                    cin = cin > carry ? cin : carry;
#pragma unroll
                    for (int j = 0; j < 4; j++) r[j] = r[j] > cin ? r[j] : cin;
                    carry = rdlane(r[3], 63);
                    uint32_t dsts[4];
                    uint8_t bytes[4];
                    bool has[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t q = wb + 4u * lane + j;
                        has[j] = q < LB && r[j] != 0;
                        const uint32_t w = has[j] ? r[j] - 1u : 0u;
                        const uint32_t i = q - L.par[4 * w + 2];
                        dsts[j] = L.par[4 * w] + i;
                        bytes[j] = 0;
                        if (has[j]) bytes[j] = in[L.par[4 * w + 1] + i];
                    }
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (has[j]) out[dsts[j]] = bytes[j];
                    LSYNC();
                }
            }
        }
        // ---- phase B: the matches, several per step as long as none reads what the step writes ----------------------------------
        uint64_t mm = __ballot(ml != 0);
        if (!mm) return;
        const uint32_t mbi = wave_incl_scan(ml), mbx = mbi - ml;
        const uint32_t srcend = mdst - off + (ml < off ? ml : off);
        LSYNC();
        L.par[4 * lane] = mdst;
        L.par[4 * lane + 1] = off;
        L.par[4 * lane + 2] = mbx;
        L.par[4 * lane + 3] = ml;
        while (mm) {
            const uint32_t k0 = (uint32_t)__ffsll((long long)mm) - 1;
            const uint32_t d0 = rdlane(mdst, k0), b0 = rdlane(mbx, k0), l0 = rdlane(ml, k0);
            if (l0 > LZ4_LONG_MATCH) {  // a long match is copied on its own, in its turn
                lz4_wave_match(out + d0, rdlane(off, k0), l0);
                mm &= ~(1ull << k0);
                continue;
            }
            const uint64_t okm = __ballot(ml && (mbi - b0 <= 256u) && (lane == k0 || srcend <= d0));
            const uint64_t rem = mm & ~okm;
            const uint64_t inc = rem ? (mm & ((1ull << ((uint32_t)__ffsll((long long)rem) - 1)) - 1ull)) : mm;
            const uint32_t lastl = 63u - (uint32_t)__clzll((long long)inc);
            const uint32_t nbytes = rdlane(mbi, lastl) - b0;
            L.heads[lane] = 0;
            LSYNC();
            if ((inc >> lane) & 1ull) ((LDS_AS uint8_t *)L.heads)[mbx - b0] = (uint8_t)(lane + 1);
            LSYNC();
            const uint32_t h = L.heads[lane];
            uint32_t r[4] = {h & 0xffu, (h >> 8) & 0xffu, (h >> 16) & 0xffu, h >> 24};
            r[1] = r[1] > r[0] ? r[1] : r[0];
            r[2] = r[2] > r[1] ? r[2] : r[1];
            r[3] = r[3] > r[2] ? r[3] : r[2];
            const uint32_t cin = wave_shr1(wave_incl_max_scan(r[3]));
            uint32_t srcs[4], dsts[4];
            uint8_t bytes[4];
            bool has[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                r[j] = r[j] > cin ? r[j] : cin;
                const uint32_t q = 4u * lane + j;
                has[j] = q < nbytes && r[j] != 0;
                const uint32_t w = has[j] ? r[j] - 1u : 0u;
                const uint32_t st = L.par[4 * w], ds = L.par[4 * w + 1], ln = L.par[4 * w + 3];
                const uint32_t i = q + b0 - L.par[4 * w + 2];
                dsts[j] = st + i;
                srcs[j] = st - ds + ((ds >= ln || !has[j]) ? i : i % ds);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                bytes[j] = 0;
                if (has[j]) bytes[j] = out[srcs[j]];
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (has[j]) out[dsts[j]] = bytes[j];
            LSYNC();
            mm &= ~inc;
        }
    }

    // One block's sequences, in[p .. end): the block rules.  hist0: the bytes an offset may reach in front of the block's first
    // byte; blk_max / e_size: the block maximum and its verdict (NO_LIMIT: a lone block).  Answers the status; p is left at the token
    // of the sequence that stopped the block (at `end` on CHIP_FINISHED), o counts what was produced.
    __device__ int32_t block(uint32_t &p, uint32_t end, uint64_t hist0, uint64_t blk_max, int32_t e_size)
    {
        const uint32_t lane = lane_id();
        const uint64_t o0 = o;
        for (;;) {
            uint32_t v_lit = 0, v_ll = 0, v_ldst = 0, v_ml = 0, v_off = 1, v_mdst = 0;
            int32_t st = lz4::SEQ_OK;
            for (uint32_t cnt = 0; cnt < 64 && st == lz4::SEQ_OK; cnt++) {
                lz4::Seq s;
                const uint64_t done = o - o0;
                st = lz4::parse_seq(rd, end, p, hist0 + done, SIZES ? lz4::NO_LIMIT : cap - o, blk_max == lz4::NO_LIMIT ? lz4::NO_LIMIT : blk_max - done,
                                    e_size, s);
                if (!SIZES) {
                    uint32_t ll = (uint32_t)s.ll;
                    if (ll >= LZ4_LONG_LIT) {
                        lz4_wave_copy(out + o, in + s.lit_pos, ll);
                        ll = 0;
                    }
                    if (lane == cnt) {
                        v_lit = s.lit_pos;
                        v_ll = ll;
                        v_ldst = (uint32_t)o;
                        v_ml = (uint32_t)s.ml;
                        v_off = s.ml ? s.off : 1u;
                        v_mdst = (uint32_t)(o + s.ll);
                    }
                }
                o += s.ll + s.ml;
            }
            if (!SIZES) execute(v_lit, v_ll, v_ldst, v_ml, v_off, v_mdst);
            if (st != lz4::SEQ_OK) return st;
        }
    }
};

// One unit: the wave's whole work.  out_size != nullptr in the size pass only.
template <bool SIZES>
__device__ __forceinline__ void lz4_unit(const BatchArgs &a, uint64_t *out_size)
{
    __shared__ Lz4Lds L;
    const uint32_t u = blockIdx.x, lane = lane_id();
    const uint32_t len = a.in_len[u];
    const uint8_t *const in_ = a.in_base + a.in_off[u];
    uint8_t *const out_ = SIZES ? nullptr : a.out_base + a.out_off[u];
    Lz4Unit<SIZES> U{L, Lz4Reader{(LDS_AS uint8_t *)L.win, (const GAS uint8_t *)in_, len, -((int64_t)1 << 40)}, (const GAS uint8_t *)in_, (GAS uint8_t *)out_,
                     SIZES ? lz4::NO_LIMIT : (uint64_t)a.out_cap[u], 0};
    int32_t status;
    uint32_t used = 0;
    uint64_t out_len = 0;
    if (a.format == CHIP_FMT_LZ4_BLOCK) {
        uint32_t p = 0;
        status = U.block(p, len, 0, lz4::NO_LIMIT, 0);
        used = p;
        out_len = U.o;
    } else {
        lz4::FrameHeader h;
        status = lz4::frame_header(U.rd, len, h);
        if (status == lz4::HDR_OK) {
            const uint32_t extra = h.block_checksum() ? 4u : 0u;
            uint32_t q = h.header_bytes;
            status = lz4::SEQ_OK;
            for (;;) {
                used = q;
                out_len = U.o;
                if (len - q < 4) {
                    status = CHIP_NEED_INPUT;
                    break;
                }
                const uint32_t w = lz4::le32(U.rd, q);
                if (w == 0) {
                    q += 4;
                    break;
                }
                const uint32_t size = w & 0x7fffffffu;
                if (size > h.block_max) {
                    status = CHIP_LZ4_E_BLOCK_SIZE;
                    break;
                }
                if ((uint64_t)(len - q - 4) < (uint64_t)size + extra) {
                    status = CHIP_NEED_INPUT;
                    break;
                }
                const uint32_t body = q + 4;
                if (w >> 31) {
                    if (!SIZES) {
                        if (size > U.cap - U.o) {
                            status = CHIP_NEED_OUTPUT;
                            break;
                        }
                        lz4_wave_copy(U.out + U.o, U.in + body, size);
                    }
                    U.o += size;
                } else {
                    uint32_t p = body;
                    const int32_t bs = U.block(p, body + size, h.indep() ? 0 : U.o, h.block_max, CHIP_LZ4_E_BLOCK_SIZE);
                    if (bs != CHIP_FINISHED) {
                        status = bs == CHIP_NEED_INPUT ? CHIP_LZ4_E_BLOCK : bs;
                        out_len = U.o;
                        break;
                    }
                }
                if (extra && !SIZES) {
                    const uint32_t want = lz4::le32(U.rd, body + size);
                    if (wave_xxh32(L.stage, in_ + body, size, 0) != want) {
                        status = CHIP_LZ4_E_BLOCK_CHECKSUM;
                        break;
                    }
                }
                q = body + size + extra;
            }
            if (status == lz4::SEQ_OK) {  // behind the EndMark; `used` is the EndMark's offset
                out_len = U.o;
                if (h.content_checksum() && len - q < 4) {
                    status = CHIP_NEED_INPUT;
                } else if (h.has_size() && h.content_size != U.o) {
                    status = CHIP_LZ4_E_CONTENT_SIZE;
                    used = q + (h.content_checksum() ? 4u : 0u);
                } else if (h.content_checksum()) {
                    const uint32_t want = lz4::le32(U.rd, q);
                    q += 4;
                    used = q;
                    status = CHIP_FINISHED;
                    if (!SIZES && wave_xxh32(L.stage, out_, U.o, 0) != want) status = CHIP_LZ4_E_CONTENT_CHECKSUM;
                } else {
                    used = q;
                    status = CHIP_FINISHED;
                }
            }
        }
    }
    if (lane == 0) {
        a.in_used[u] = used;
        a.status[u] = status;
        if (SIZES) out_size[u] = out_len;
        else a.out_len[u] = (uint32_t)out_len;
    }
}

}  // namespace

}  // namespace chip
