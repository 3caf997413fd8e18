// The device code of the batched Snappy decode for gfx950 (MI355X), shared by the decode kernel and the size kernel of snappy.hip:
// one wavefront decodes one unit, a raw block (CHIP_FMT_SNAPPY_BLOCK) or a framed stream (CHIP_FMT_SNAPPY).  DESIGN.md sec. 4.28.
//
// A block is a varint and a chain of elements, each a literal or a copy: where an element starts is known only once the one in
// front of it has been parsed.  That chain is the only serial part.  The wave parses it wave-uniformly, in scalar registers, out of
// a 2 KiB window of the input staged in LDS (snappy_core.h's parse_element, the same code as the host decoder runs).  A tag and
// the at most four bytes behind it lie in two aligned dwords of the window: they come in ONE LDS round trip, are brought together
// by a 64-bit scalar shift, and every field is scalar arithmetic on that word (the LZ4 parse makes three dependent round trips per
// sequence: sec. 4.26).  64 elements form a group: lane k keeps element k's kind, source position or offset, length and destination.
// Every verdict depends on positions only, so the parse alone decides status, out_len and in_used, and the size pass is the parse
// without the copies.
// Then the group is executed wave-wide, the two phases from the one kind flag per lane.  Phase A copies the bytes of all literals of
// the group, 256 per step: their sources are input bytes, so nothing orders them.  Phase B copies the copies in steps of up to 256
// bytes: a step takes the longest run of consecutive copies none of which reads a byte at or behind the first one's destination
// (the srcend <= d0 rule of lz4_unit.h and zstd_unit.h), so that all loads of a step are issued before its first store.  In both
// phases a byte finds its element through a byte-wide owner map scattered into LDS and a running maximum across the wave.  A copy
// whose offset is below its length replicates a period: byte i reads byte i % offset of the period.  Literals of 64 bytes and more
// are copied when they are parsed, 16 bytes per lane; a copy is at most 64 bytes long, so none needs a turn of its own.
// A wave's global stores are seen by its later loads in program order (the lanes of one wave share the CU's L1), so no step waits
// for its stores to be acknowledged.
// A framed stream adds the hop over the chunk headers (snappy_core.h's chunk_header) and, per data chunk, CRC-32C of its content on
// the wave: slicing by four out of 4 KiB of LDS tables, a piece per lane, the pieces combined by carry-less multiplications.
#pragma once
#include "chip_internal.h"
#include "snappy_core.h"
#include "wave_checksums.h"

namespace chip {

namespace {

constexpr uint32_t SNAPPY_WIN = 2048;     // bytes of input staged in LDS
constexpr uint32_t SNAPPY_LONG_LIT = 64;  // literals from here on are copied when they are parsed

template <bool SIZES>
struct SnappyLds {
    uint32_t win[SNAPPY_WIN / 4];
    uint32_t heads[64];             // owner map of a step: 256 bytes, lane + 1 of the element whose bytes start at that byte
    uint32_t par[64 * 4];           // per element: destination, source / offset, bytes in front of it in the group, length
    uint32_t crc[SIZES ? 1 : 1024]; // the four CRC-32C tables (the size pass compares no CRC)
};

struct __attribute__((packed, aligned(1))) SnappyU32 {
    uint32_t v;
};
typedef uint32_t snappy_u32x4 __attribute__((ext_vector_type(4)));
typedef snappy_u32x4 SnappyU128 __attribute__((aligned(1)));  // 16 bytes at any address (gfx950 does unaligned global accesses)

// Fills the window with the aligned dwords from in + base on (base: a unit position, in + base 4-byte aligned, possibly -3 .. -1);
// dwords that hold no byte of the unit are not loaded.  Out of line: the parse reaches it from every byte it reads.
__device__ __attribute__((noinline)) void snappy_refill(LDS_AS uint32_t *win, const GAS uint8_t *in, uint32_t len, int64_t base)
{
    const uint32_t lane = lane_id();
    LSYNC();
#pragma unroll
    for (uint32_t k = 0; k < SNAPPY_WIN / 256; k++) {
        const int64_t pos = base + 4 * (int64_t)(lane + 64u * k);
        uint32_t v = 0;
        if (pos < (int64_t)len) v = *(const GAS uint32_t *)(in + pos);
        win[lane + 64u * k] = v;
    }
    LSYNC();
}

// The unit's input through the LDS window.  Positions are offsets into the unit; everything here is wave-uniform.
struct SnappyReader {
    LDS_AS uint8_t *win;
    const GAS uint8_t *in;
    uint32_t len;  // of the unit: loads stay inside the aligned dwords that hold bytes of it
    int64_t base;  // the window holds unit positions [base, base + SNAPPY_WIN); base may be -3 .. -1 (an aligned dword in front)
    // brings [q, q + need) into the window; answers q's offset in it
    __device__ __forceinline__ uint32_t at(uint64_t q, uint32_t need)
    {
        if ((uint64_t)((int64_t)q - base) > SNAPPY_WIN - need) {
            base = (int64_t)q - (int64_t)((uintptr_t)(in + q) & 3u);
            snappy_refill((LDS_AS uint32_t *)win, in, len, base);
        }
        return (uint32_t)((int64_t)q - base);
    }
    __device__ __forceinline__ uint32_t byte(uint64_t q) { return rdfirst(win[at(q, 1)]); }
    // a tag and the four bytes behind it: the two aligned dwords that hold them, one round trip, and a scalar funnel shift
    __device__ __forceinline__ uint64_t head(uint64_t q)
    {
        const uint32_t x = at(q, 8);
        const LDS_AS uint32_t *const w = (const LDS_AS uint32_t *)win + (x >> 2);
        const uint32_t lo = w[0], hi = w[1];
        return ((((uint64_t)rdfirst(hi)) << 32) | rdfirst(lo)) >> (8u * (x & 3u));
    }
};

// forward copy of n bytes between disjoint ranges by the whole wave: 16 bytes per lane and trip at any alignment
__device__ __forceinline__ void snappy_wave_copy(GAS uint8_t *dst, const GAS uint8_t *src, uint32_t n)
{
    const uint32_t lane = lane_id(), whole = n & ~15u;
    for (uint32_t j = 16u * lane; j < whole; j += 1024u) {
        const SnappyU128 v = *(const GAS SnappyU128 *)(src + j);
        *(GAS SnappyU128 *)(dst + j) = v;
    }
    if (whole + lane < n) dst[whole + lane] = src[whole + lane];
}

// ---- CRC-32C on one wave -----------------------------------------------------------------------------------------------------------
// x^(2^k) mod P for the reflected CRC-32C polynomial 0x82F63B78 (bit 31 = x^0); P = (x + 1) * a primitive polynomial of degree 31,
// so the row repeats after 31 entries: the table is as long as the index can get (3 + 26 + 5)
__device__ __constant__ static const uint32_t SNAPPY_X2N[36] = {
    0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u, 0x82f63b78u, 0x6ea2d55cu, 0x18b8ea18u, 0x510ac59au,
    0xb82be955u, 0xb8fdb1e7u, 0x88e56f72u, 0x74c360a4u, 0xe4172b16u, 0x0d65762au, 0x35d73a62u, 0x28461564u, 0xbf455269u,
    0xe2ea32dcu, 0xfe7740e6u, 0xf946610bu, 0x3c204f8fu, 0x538586e3u, 0x59726915u, 0x734d5309u, 0xbc1ac763u, 0x7d0722ccu,
    0xd289cabeu, 0xe94ca9bcu, 0x05b74f3fu, 0xa51e1f42u, 0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u};

// a(x) * b(x) mod P, reflected representation
__device__ __forceinline__ uint32_t snappy_multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll 8
    for (int i = 0; i < 32; i++) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? snappy::CRC32C_POLY : 0u);
    }
    return p;
}

// the four 256-entry tables of slicing by four (table k advances the register over a byte that lies k bytes further on)
__device__ __attribute__((noinline, unused)) void snappy_crc_tables(LDS_AS uint32_t *tab)
{
    const uint32_t lane = lane_id();
    LSYNC();
    for (uint32_t i = lane; i < 256; i += 64) tab[i] = snappy::crc32c_byte(0, i);
    LSYNC();
    for (uint32_t k = 1; k < 4; k++) {
        for (uint32_t i = lane; i < 256; i += 64) {
            const uint32_t c = tab[(k - 1) * 256 + i];
            tab[k * 256 + i] = (c >> 8) ^ tab[c & 0xffu];
        }
        LSYNC();
    }
}

// CRC-32C (unmasked) of p[0 .. n) over the tables of snappy_crc_tables: lane i runs over the i-th of 64 right-aligned pieces of
// 2^lg bytes (wave_checksums.h's lane_chunk) with 16-byte loads, four bytes per dependent step; the pieces' registers are then
// combined across the lanes, state(A || B) = state(A) * x^(8 |B|) + raw(B).
__device__ __attribute__((noinline, unused)) uint32_t wave_crc32c(LDS_AS uint32_t *tab, const uint8_t *p_, uint32_t n)
{
    const uint32_t lane = lane_id();
    const GAS uint8_t *const p = (const GAS uint8_t *)p_;
    uint32_t lg, beg, end;
    lane_chunk(n, lg, beg, end);
    uint32_t c = (beg == 0 && end > 0) ? 0xFFFFFFFFu : 0u;  // the lane that owns byte 0 carries the initial value
    if (n == 0 && lane == 63) c = 0xFFFFFFFFu;
    uint32_t k = beg;
    while (k < end && (((uintptr_t)(p + k)) & 15u) != 0) {
        c = tab[(c ^ p[k]) & 0xffu] ^ (c >> 8);
        k++;
    }
    for (; k + 16 <= end; k += 16) {
        const snappy_u32x4 d = *(const GAS snappy_u32x4 *)(p + k);
        const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t v = w[j] ^ c;
            c = tab[3 * 256 + (v & 0xffu)] ^ tab[2 * 256 + ((v >> 8) & 0xffu)] ^ tab[256 + ((v >> 16) & 0xffu)] ^ tab[v >> 24];
        }
    }
    for (; k < end; k++) c = tab[(c ^ p[k]) & 0xffu] ^ (c >> 8);
#pragma unroll
    for (int k2 = 0; k2 < 6; k2++) {
        const uint32_t left = (uint32_t)__shfl_up((int)c, 1 << k2, 64);
        const uint32_t comb = snappy_multmodp(SNAPPY_X2N[3 + lg + k2], left) ^ c;
        if ((lane & ((2u << k2) - 1)) == ((2u << k2) - 1)) c = comb;
    }
    return ~rdlane(c, 63);
}

// ---- one unit ----------------------------------------------------------------------------------------------------------------------
// What one unit's decode keeps across chunks; wave-uniform.
template <bool SIZES>
struct SnappyUnit {
    SnappyLds<SIZES> &L;
    SnappyReader rd;
    const GAS uint8_t *in;
    GAS uint8_t *out;
    uint64_t cap;  // NO_LIMIT in the size pass
    uint64_t o;    // bytes produced

    // Executes the group: lane k < cnt holds element k -- lit: a literal (a = the position of its bytes in the input) or a copy
    // (a = its offset); n its length (0: none, or a literal that was copied when it was parsed); dst its destination.
    __device__ void execute(bool lit, uint32_t a, uint32_t n, uint32_t dst)
    {
        const uint32_t lane = lane_id();
        const uint32_t ll = lit ? n : 0u, ml = lit ? 0u : n, off = lit ? 1u : a;
        // ---- phase A: the literal bytes of the group, 256 per step --------------------------------------------------------------
        {
            const uint32_t lbi = wave_incl_scan(ll), lbx = lbi - ll, LB = rdlane(lbi, 63);
            if (LB) {
                LSYNC();
                L.par[4 * lane] = dst;
                L.par[4 * lane + 1] = a;
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
        // ---- phase B: the copies, several per step as long as none reads what the step writes ------------------------------------
        uint64_t mm = __ballot(ml != 0);
        if (!mm) return;
        const uint32_t mbi = wave_incl_scan(ml), mbx = mbi - ml;
        const uint32_t srcend = dst - off + (ml < off ? ml : off);
        LSYNC();
        L.par[4 * lane] = dst;
        L.par[4 * lane + 1] = off;
        L.par[4 * lane + 2] = mbx;
        L.par[4 * lane + 3] = ml;
        while (mm) {
            const uint32_t k0 = (uint32_t)__ffsll((long long)mm) - 1;
            const uint32_t d0 = rdlane(dst, k0), b0 = rdlane(mbx, k0);
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

    // One block, in[p .. end): the block rules.  framed: the changes a chunk of the framing format makes (n at most 65 536, the room
    // is what is left of it; CHIP_NEED_INPUT stays the caller's to rename).  Answers the status; p is left at the tag of the element
    // that stopped the block (where it was, inside the preamble; at `end` on CHIP_FINISHED), o counts what was produced.
    __device__ int32_t block(uint32_t &p, uint32_t end, bool framed)
    {
        const uint32_t lane = lane_id(), p0 = p;
        const uint64_t o0 = o;
        uint64_t n;
        int32_t st = snappy::preamble(rd, end, p, n);
        if (st == snappy::OK && framed && n > snappy::CHUNK_MAX) st = CHIP_SNAPPY_E_CHUNK_SIZE;
        if (st == snappy::OK && !SIZES && n > cap - o0) st = CHIP_NEED_OUTPUT;
        if (st != snappy::OK) {
            p = p0;
            return st;
        }
        uint64_t ob = 0;  // produced by this block
        for (;;) {
            bool v_lit = false;
            uint32_t v_a = 0, v_n = 0, v_dst = 0;
            for (uint32_t cnt = 0; cnt < 64; cnt++) {
                snappy::Elem e;
                st = snappy::parse_element(rd, end, p, ob, n, e);
                if (st != snappy::OK) break;
                if (!SIZES) {
                    uint32_t len = (uint32_t)e.n;
                    if (e.lit && len >= SNAPPY_LONG_LIT) {
                        snappy_wave_copy(out + o0 + ob, in + e.src, len);
                        len = 0;
                    }
                    if (lane == cnt) {
                        v_lit = e.lit;
                        v_a = e.lit ? e.src : e.off;
                        v_n = len;
                        v_dst = (uint32_t)(o0 + ob);
                    }
                }
                ob += e.n;
            }
            if (!SIZES) execute(v_lit, v_a, v_n, v_dst);
            if (st != snappy::OK) {
                o = o0 + ob;
                return st;
            }
        }
    }
};

// One unit: the wave's whole work.  out_size != nullptr in the size pass only.
template <bool SIZES>
__device__ __forceinline__ void snappy_unit(const BatchArgs &a, uint64_t *out_size)
{
    __shared__ SnappyLds<SIZES> L;
    const uint32_t u = blockIdx.x, lane = lane_id();
    const uint32_t len = a.in_len[u];
    const uint8_t *const in_ = a.in_base + a.in_off[u];
    uint8_t *const out_ = SIZES ? nullptr : a.out_base + a.out_off[u];
    SnappyUnit<SIZES> U{L, SnappyReader{(LDS_AS uint8_t *)L.win, (const GAS uint8_t *)in_, len, -((int64_t)1 << 40)}, (const GAS uint8_t *)in_,
                        (GAS uint8_t *)out_, SIZES ? snappy::NO_LIMIT : (uint64_t)a.out_cap[u], 0};
    int32_t status;
    uint32_t used = 0;
    uint64_t out_len = 0;
    if (a.format == CHIP_FMT_SNAPPY_BLOCK) {
        uint32_t p = 0;
        status = U.block(p, len, false);
        used = p;
        out_len = U.o;
    } else {
        status = snappy::stream_start(U.rd, len);
        if (status == snappy::OK) {
            bool tables = false;
            uint32_t q = 10;
            for (;;) {
                used = q;
                out_len = U.o;
                uint32_t type, s, want;
                status = snappy::chunk_header(U.rd, len, q, type, s, want);
                if (status == snappy::CHUNK_SKIP) {
                    q += 4 + s;
                    continue;
                }
                if (status != snappy::OK) break;  // (CHIP_FINISHED at the end of the input: used == len)
                const uint32_t body = q + 8, size = s - 4;
                const uint8_t *content = in_ + body;  // what the CRC covers: the input of an uncompressed chunk, the output of a block
                uint32_t n_content = size;
                if (type == 1) {
                    if (size > snappy::CHUNK_MAX) {
                        status = CHIP_SNAPPY_E_CHUNK_SIZE;
                        break;
                    }
                    if (!SIZES) {
                        if (size > U.cap - U.o) {
                            status = CHIP_NEED_OUTPUT;
                            break;
                        }
                        snappy_wave_copy(U.out + U.o, U.in + body, size);
                    }
                    U.o += size;
                } else {
                    uint32_t p = body;
                    const int32_t bs = U.block(p, body + size, true);
                    if (bs != CHIP_FINISHED) {
                        status = bs == CHIP_NEED_INPUT ? CHIP_SNAPPY_E_BLOCK : bs;
                        out_len = U.o;
                        break;
                    }
                    n_content = (uint32_t)(U.o - out_len);
                    content = out_ + out_len;
                }
                if (!SIZES) {
                    if (!tables) snappy_crc_tables((LDS_AS uint32_t *)L.crc);
                    tables = true;
                    if (snappy::mask(wave_crc32c((LDS_AS uint32_t *)L.crc, content, n_content)) != want) {
                        status = CHIP_SNAPPY_E_CHECKSUM;
                        break;
                    }
                }
                q += 4 + s;
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
