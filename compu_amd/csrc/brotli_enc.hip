// brotli encoder (RFC 7932): one wavefront encodes one unit into one complete stream (or, for the streaming encoder, one byte-
// aligned segment of a stream).  Persistent grid: each wave takes the next unit from a counter and keeps the metablock being built
// (commands, literals, prefix codes) in a per-wave HBM scratch; the match finder's hash table lives in LDS.  The lanes share the
// match finder (zstd_enc_core.h's 64-position chunks), the literal copy and histogram, the command codes and their histograms, the
// code lengths (rank sort, pointer jumping), the sizes, the bit emission (per-item bit counts, a wave scan, ORs into an LDS bit
// buffer) and the copies of uncompressed metablocks.  Lane 0 keeps what is serial: the distance ring chain, the Huffman merge and
// length limit, the code descriptions and headers.
#include <mutex>

#include "chip_internal.h"
#include "launch_slots.h"
#include "brotli_enc_core.h"

namespace chip {

namespace {

struct BEncArgs {
    BatchArgs b;
    uint32_t group;
    uint32_t lgwin;
    uint32_t flags;        // ZF_FIRST (WBITS, a fresh ring), ZF_LAST (close the stream)
    BEncStream *stream;    // streaming encoder only: the distance ring carried between segments (n == 1)
};

constexpr size_t CMD_BYTES = (size_t)benc::MAX_CMD * sizeof(benc::Cmd);
constexpr size_t WAVE_SCRATCH = ((CMD_BYTES + benc::MB_MAX + sizeof(benc::Work)) + 255) & ~(size_t)255;

constexpr uint32_t OBUF = 256;  // dwords of the emission's bit buffer; a group of 64 items adds at most 64 x 63 bits

struct alignas(16) BLds {
    uint16_t ht[zenc::HSIZE];  // 16 KiB
    union {
        zenc::Chunk k;  // 1.5 KiB: the match finder's chunk
        struct {
            uint32_t obuf[OBUF];  // the bit buffer of the emission
            uint32_t ws[64];      // the emission's window of 64 commands: first item,
            uint32_t wl[64];      // and first literal
        } e;
    };
    uint32_t cnt[256];  // the metablock's literal histogram; during the emission the literal codes (code | length << 16)
};
static_assert(sizeof(zenc::Chunk) == (OBUF + 128) * 4, "the emission's buffers take the chunk's place");

// lane 0's global stores made visible to the other lanes (and theirs to lane 0) before the next step reads them
#define BFENCE() do { __threadfence(); WSYNC(); } while (0)

// the output position and the bit writer's pending bits, as lane 0 left them, to every lane
__device__ __forceinline__ void bits_from_lane0(zenc::Out &o, benc::Bits &b)
{
    o.pos = rdfirst(o.pos);
    o.ovf = rdfirst(o.ovf);
    b.n = rdfirst(b.n);
    b.acc = ((uint64_t)rdfirst((uint32_t)(b.acc >> 32)) << 32) | rdfirst((uint32_t)b.acc);
}

__device__ __forceinline__ uint32_t bwave_sum(uint32_t v) { return rdlane(wave_incl_scan(v), 63); }

// Code lengths of cnt[0 .. nsym) by the wave, the same as benc::huff_lengths: the lanes rank the used symbols by (count, symbol)
// and find the depths by pointer jumping; lane 0 merges (the two queues are a chain) and limits the lengths.
__device__ uint32_t huff_lengths_wave(benc::Work &w, const uint32_t *cnt, uint32_t nsym, uint8_t *len)
{
    const uint32_t lane = lane_id();
    uint32_t n = 0;
    for (uint32_t s = lane; s < nsym; s += 64) {
        len[s] = 0;
        n += cnt[s] ? 1u : 0u;
    }
    n = bwave_sum(n);
    if (n < 2) {
        BFENCE();
        return n;
    }
    for (uint32_t s = lane; s < nsym; s += 64) {
        const uint32_t c = cnt[s];
        if (!c) continue;
        const uint32_t key = (c << 10) | s;
        uint32_t r = 0;
        for (uint32_t t = 0; t < nsym; t++) {
            const uint32_t ct = cnt[t];  // the same address in all lanes
            r += (ct && ((ct << 10) | t) < key) ? 1u : 0u;
        }
        w.key[r] = key;
    }
    BFENCE();
    if (lane == 0) benc::huff_merge(w, n);
    BFENCE();
    // after a round a node knows its distance to the ancestor it points at, and points twice as far up
    const uint32_t nn = 2 * n - 1, root = nn - 1;
    for (uint32_t i = lane; i < nn; i += 64) {
        w.jd[0][i] = i < root ? 1u : 0u;
        w.jp[0][i] = w.node_p[i];
    }
    BFENCE();
    uint32_t cur = 0;
    for (;;) {
        bool open = false;
        for (uint32_t i = lane; i < nn; i += 64) {
            const uint32_t p = w.jp[cur][i], pp = w.jp[cur][p];
            w.jd[cur ^ 1][i] = w.jd[cur][i] + w.jd[cur][p];
            w.jp[cur ^ 1][i] = (uint16_t)pp;
            open |= pp != root;
        }
        BFENCE();
        cur ^= 1;
        if (__ballot(open) == 0) break;
    }
    for (uint32_t i = lane; i < nn; i += 64) {
        const uint32_t d = w.jd[cur][i];
        w.depth[i] = (uint8_t)(d > 255 ? 255 : d);
    }
    BFENCE();
    if (lane == 0) benc::huff_limit(w, n, benc::MAXBITS, len);
    BFENCE();
    return n;
}

// one value of nb <= 64 bits per lane (nb = 0: none), appended in lane order
__device__ __forceinline__ void put_lanes(BLds &L, uint32_t &nbits, uint64_t bits, uint32_t nb)
{
    const uint32_t incl = wave_incl_scan(nb);
    if (nb) {
        const uint32_t at = nbits + incl - nb, wd = at >> 5, sh = at & 31u;
        const uint64_t lo = bits << sh;
        atomicOr(&L.e.obuf[wd], (uint32_t)lo);
        if (sh + nb > 32) atomicOr(&L.e.obuf[wd + 1], (uint32_t)(lo >> 32));
        if (sh + nb > 64) atomicOr(&L.e.obuf[wd + 2], (uint32_t)(bits >> (64u - sh)));
    }
    nbits += rdlane(incl, 63);
}

// the first nbytes bytes of the bit buffer to o.p[at ..], nothing at or past o.cap
__device__ void store_obuf(BLds &L, const zenc::Out &o, uint32_t at, uint32_t nbytes)
{
    struct __attribute__((packed, aligned(1))) U32u {
        uint32_t v;
    };
    const uint32_t lane = lane_id(), ndw = nbytes >> 2;
    const uint8_t *src = (const uint8_t *)L.e.obuf;
    for (uint32_t j = lane; j < ndw; j += 64) {
        const uint32_t a = at + 4u * j;
        if (a + 4u <= o.cap) {
            ((U32u *)(o.p + a))->v = L.e.obuf[j];
        } else {
            for (uint32_t k = 0; k < 4; k++)
                if (a + k < o.cap) o.p[a + k] = src[4u * j + k];
        }
    }
    for (uint32_t j = 4u * ndw + lane; j < nbytes; j += 64)
        if (at + j < o.cap) o.p[at + j] = src[j];
}

// The commands and literals of a compressed metablock (benc::emit_commands, the same bits): the items in order -- per command its
// head, its literals, its distance (0 bits when it has none) -- 64 at a time, one per lane; a lane finds its command in a window of
// 64 commands (first item and first literal by a scan of the insert lengths) and the bits land in the LDS bit buffer by put_lanes.
// The writer's pending bits go in front and the last partial byte comes back to it.
__device__ void emit_body(BLds &L, const benc::Scratch &sc, uint32_t nc, uint32_t nl, zenc::Out &o, benc::Bits &b)
{
    const uint32_t lane = lane_id();
    const benc::Work &w = *sc.w;
    for (uint32_t j = lane; j < OBUF; j += 64) L.e.obuf[j] = j == 0 ? (uint32_t)b.acc : 0u;
    LSYNC();
    uint32_t nbits = b.n, obytes = o.pos;
    const uint32_t total = nl + 2 * nc;
    uint32_t cur = 0, scur = 0, lcur = 0;
    for (uint32_t t0 = 0; t0 < total; t0 += 64) {
        const uint32_t ci = cur + lane;
        const uint32_t ins = ci < nc ? sc.cmd[ci].ins : 0u;
        const uint32_t ex = wave_incl_scan(ins) - ins;
        const uint32_t first = ci < nc ? scur + 2 * lane + ex : 0xffffffffu, flit = lcur + ex;
        L.e.ws[lane] = first;
        L.e.wl[lane] = flit;
        LSYNC();
        const uint32_t t = t0 + lane;
        uint64_t bits = 0;
        uint32_t nb = 0;
        if (t < total) {
            uint32_t i = 0;
            for (uint32_t step = 32; step; step >>= 1)
                if (L.e.ws[i + step] <= t) i += step;
            const benc::Cmd &c = sc.cmd[cur + i];
            const uint32_t j = t - L.e.ws[i];
            if (j == 0) {
                uint32_t inb, ibase, cnb, cbase;
                const uint32_t cl = c.len ? c.len : 4u;
                benc::ins_code(c.ins, inb, ibase);
                benc::copy_code(cl, cnb, cbase);
                nb = w.len_ic[c.ic];
                bits = w.code_ic[c.ic];
                bits |= (uint64_t)(c.ins - ibase) << nb;
                nb += inb;
                bits |= (uint64_t)(cl - cbase) << nb;
                nb += cnb;
            } else if (j <= c.ins) {
                const uint32_t e = L.cnt[sc.lit[L.e.wl[i] + j - 1]];
                bits = e & 0xffffu;
                nb = e >> 16;
            } else if (c.dsym != benc::NO_DIST) {
                nb = w.len_d[c.dsym];
                bits = w.code_d[c.dsym] | ((uint64_t)c.dextra << nb);
                nb += c.dnb;
            }
        }
        put_lanes(L, nbits, bits, nb);
        // the next window starts at the command that holds item t0 + 64
        const uint32_t k = (uint32_t)__popcll(__ballot(first <= t0 + 64)) - 1u;
        cur += k;
        scur = rdlane(first, k);
        lcur = rdlane(flit, k);
        LSYNC();
        if (nbits > (OBUF - 128) * 32) {  // whole dwords out, the partial one to the front
            const uint32_t nw = nbits >> 5;
            store_obuf(L, o, obytes, 4 * nw);
            const uint32_t carry = L.e.obuf[nw];
            LSYNC();
            for (uint32_t j = lane; j < OBUF; j += 64) L.e.obuf[j] = j == 0 ? carry : 0u;
            LSYNC();
            obytes += 4 * nw;
            nbits &= 31u;
        }
    }
    const uint32_t nbytes = nbits >> 3;
    store_obuf(L, o, obytes, nbytes);
    b.n = nbits & 7u;
    b.acc = ((const uint8_t *)L.e.obuf)[nbytes] & ((1u << b.n) - 1u);
    o.pos = obytes + nbytes;
    if (o.pos > o.cap) o.ovf = true;
    LSYNC();
}

// All 64 lanes run this (control flow is uniform); the serial steps write from lane 0 only.  The kernel form of
// benc::compress_segment (same steps, same bytes).
__device__ bool encode_segment_wave(const zenc::Cfg &c, BLds &L, const benc::Scratch &sc, const uint8_t *src, uint32_t n, bool first,
                                    bool last, uint32_t lgwin, uint32_t *ring, zenc::Out &o)
{
    const uint32_t lane = lane_id();
    benc::Bits b = {&o, 0, 0};
    if (first && lane == 0) benc::write_wbits(b, lgwin);
    bits_from_lane0(o, b);
    for (uint32_t bs = 0; bs < n; bs += benc::MB_MAX) {
        const uint32_t be = n - bs > benc::MB_MAX ? bs + benc::MB_MAX : n, bn = be - bs;
        const bool islast = last && be == n;
        for (uint32_t i = lane; i < 256; i += 64) L.cnt[i] = 0;
        LSYNC();
        uint32_t nc = 0, nl = 0, anchor = bs, rep0 = ring[0], ip = bs;
        auto lits = [&](uint32_t a, uint32_t e) {  // lanes copy and count the literals src[a .. e)
            for (uint32_t i = a + lane; i < e; i += 64) {
                const uint8_t v = src[i];
                sc.lit[nl + (i - a)] = v;
                atomicAdd(&L.cnt[v], 1u);
            }
            nl += e - a;
        };
        auto emit = [&](uint32_t anc, uint32_t p, uint32_t ml, uint32_t off) {
            lits(anc, p);
            if (lane == 0) {
                sc.cmd[nc].ins = p - anc;
                sc.cmd[nc].len = ml;
                sc.cmd[nc].dist = off;
            }
            nc++;
        };
        while ((uint64_t)ip + 8 <= be) {
            zenc::chunk_hash(c, src, ip, be, lane, L.k);
            LSYNC();
            zenc::chunk_read(c, L.ht, ip, lane, L.k);
            LSYNC();
            zenc::chunk_update(c, L.ht, ip, lane, L.k);
            zenc::chunk_match(c, src, ip, be, rep0, lane, L.k);
            LSYNC();
            ip = rdfirst(zenc::chunk_walk(c, src, L.k, ip, be, anchor, rep0, emit));
            anchor = rdfirst(anchor);
            rep0 = rdfirst(rep0);
            LSYNC();  // the next chunk overwrites L.k
        }
        if (anchor < be) {  // the closing literal-only command
            if (lane == 0) {
                sc.cmd[nc].ins = be - anchor;
                sc.cmd[nc].len = 0;
                sc.cmd[nc].dist = 0;
            }
            nc++;
            lits(anchor, be);
        }
        LSYNC();
        for (uint32_t i = lane; i < 256; i += 64) sc.w->cnt_l[i] = L.cnt[i];
        BFENCE();
        benc::Work &w = *sc.w;
        // command codes: the ring chain on lane 0, the rest and the histograms on the lanes
        uint32_t nring[4] = {ring[0], ring[1], ring[2], ring[3]};
        if (lane == 0) benc::ring_codes(sc.cmd, nc, nring);
        for (uint32_t i = lane; i < benc::NIC; i += 64) w.cnt_ic[i] = 0;
        if (lane < benc::NDIST) w.cnt_d[lane] = 0;
        BFENCE();
        for (uint32_t i = lane; i < nc; i += 64) {
            benc::cmd_code_one(sc.cmd[i]);
            atomicAdd(&w.cnt_ic[sc.cmd[i].ic], 1u);
            if (sc.cmd[i].dsym != benc::NO_DIST) atomicAdd(&w.cnt_d[sc.cmd[i].dsym], 1u);
        }
        BFENCE();
        const uint32_t used[3] = {huff_lengths_wave(w, w.cnt_l, benc::NLIT, w.len_l), huff_lengths_wave(w, w.cnt_ic, benc::NIC, w.len_ic),
                                  huff_lengths_wave(w, w.cnt_d, benc::NDIST, w.len_d)};
        // lane 0: header and code descriptions (canonical codes with them)
        uint64_t raw_end = 0;
        benc::Bits b0 = b;
        uint32_t pos0 = o.pos;
        if (lane == 0) {
            raw_end = ((b.bitpos() + benc::uncompressed_header_bits(bn) + 7) & ~7ull) + 8ull * bn + (islast ? 2u : 0u);
            benc::metablock_head(w, b, bn, islast, used);
        }
        BFENCE();
        // lanes: the size of the commands' bits, to choose the metablock's form before any of them is written
        for (uint32_t s = lane; s < 256; s += 64) L.cnt[s] = w.code_l[s] | ((uint32_t)w.len_l[s] << 16);
        LSYNC();
        uint32_t body = 0;
        for (uint32_t i = lane; i < nc; i += 64) body += benc::cmd_bits(w, sc.cmd[i]);
        for (uint32_t i = lane; i < nl; i += 64) body += L.cnt[sc.lit[i]] >> 16;
        body = bwave_sum(body);
        uint32_t raw_at = 0xffffffffu, comp = 0;
        if (lane == 0) {
            comp = !o.ovf && b.bitpos() + body < raw_end;
            if (!comp) {  // uncompressed: the lanes copy the bytes; a last one is followed by an empty last metablock
                o.pos = pos0;
                o.ovf = false;
                b = b0;
                benc::mlen_header(b, bn, false, true);
                b.align();
                raw_at = o.pos;
                if (o.pos + (uint64_t)bn > o.cap) o.ovf = true;
                o.pos += bn;
                if (islast) b.add(3, 2);
            }
        }
        comp = rdfirst(comp);
        bits_from_lane0(o, b);
        if (comp) {
            emit_body(L, sc, nc, nl, o, b);
            for (int r = 0; r < 4; r++) ring[r] = nring[r];  // (lane 0's, made uniform below)
        }
        bits_from_lane0(o, b);
        for (int r = 0; r < 4; r++) ring[r] = rdfirst(ring[r]);
        raw_at = rdfirst(raw_at);
        if (o.ovf) return false;
        if (raw_at != 0xffffffffu)
            for (uint32_t i = lane; i < bn; i += 64) o.p[raw_at + i] = src[bs + i];  // raw_at + bn <= o.cap (no overflow)
        BFENCE();
    }
    if (lane == 0) {
        if (last) {
            if (n == 0) b.add(3, 2);
            b.align();
        } else if (b.n) {
            benc::empty_metadata(b);
        }
    }
    bits_from_lane0(o, b);
    return !o.ovf;
}

__device__ void encode_unit(const BEncArgs &a, uint32_t u, BLds &L, uint8_t *scratch)
{
    const uint32_t lane = lane_id();
    for (uint32_t i = lane; i < zenc::HSIZE; i += 64) L.ht[i] = 0;
    WSYNC();
    const uint32_t n = a.b.in_len[u], cap = a.b.out_cap[u];
    const uint8_t *src = a.b.in_base + a.b.in_off[u];
    zenc::Out o = {a.b.out_base + a.b.out_off[u], 0, cap, false};
    const bool first = a.flags & ZF_FIRST, last = a.flags & ZF_LAST;
    const zenc::Cfg c = benc::make_cfg(a.group, a.lgwin);
    uint32_t ring[4] = {4, 11, 15, 16};  // last distance first (RFC 7932 4)
    if (!first)
        for (int r = 0; r < 4; r++) ring[r] = a.stream->ring[r];
    benc::Scratch sc;
    sc.ht = L.ht;
    sc.cmd = (benc::Cmd *)scratch;
    sc.lit = scratch + CMD_BYTES;
    sc.w = (benc::Work *)(scratch + CMD_BYTES + benc::MB_MAX);
    const bool ok = encode_segment_wave(c, L, sc, src, n, first, last, a.lgwin, ring, o);
    if (lane != 0) return;
    if (a.stream)
        for (int r = 0; r < 4; r++) a.stream->ring[r] = ring[r];
    a.b.out_len[u] = ok ? o.pos : 0;
    a.b.status[u] = ok ? CHIP_ENC_FINISHED : CHIP_ENC_NEED_OUTPUT;
}

__global__ __launch_bounds__(64) void brotli_enc_kernel(BEncArgs a, uint8_t *scratch, uint32_t *next_unit)
{
    __shared__ BLds L;
    uint8_t *mine = scratch + (size_t)blockIdx.x * WAVE_SCRATCH;
    for (;;) {
        uint32_t i = 0;
        if (lane_id() == 0) i = atomicAdd(next_unit, 1u);
        i = rdfirst(i);
        if (i >= a.b.n) break;
        encode_unit(a, i, L, mine);
        WSYNC();  // the next unit reuses the LDS
    }
}

// per-wave scratch and the unit counter: a launch slot ("Launch slots")
SlotCache<WaveScratch> g_benc_cache;
ResidentWaves g_benc_resident;

}  // namespace

hipError_t launch_brotli_encode(const BatchArgs &b, int quality, int lgwin, uint32_t flags, BEncStream *stream_state, hipStream_t stream)
{
    if (b.n == 0) return hipSuccess;
    BEncArgs a;
    a.b = b;
    a.group = benc::quality_group((uint32_t)quality);
    a.lgwin = (uint32_t)lgwin;
    a.flags = flags;
    a.stream = stream_state;
    std::lock_guard<std::mutex> lk(g_benc_cache.mu);  // from the slot's lookup to the launch
    WaveScratch *sl = nullptr;
    int max_blocks = 0;
    hipError_t e = g_benc_cache.at(stream, sl);
    if (e == hipSuccess) e = g_benc_resident.get((const void *)brotli_enc_kernel, max_blocks);
    if (e == hipSuccess) e = sl->reserve(stream, b.n, max_blocks, WAVE_SCRATCH);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(sl->counter, 0, 4, stream)) != hipSuccess) return e;
    const uint32_t blocks = b.n < (uint32_t)sl->blocks ? b.n : (uint32_t)sl->blocks;
    hipLaunchKernelGGL(brotli_enc_kernel, dim3(blocks), dim3(64), 0, stream, a, sl->scratch, sl->counter);
    return hipGetLastError();
}

}  // namespace chip
