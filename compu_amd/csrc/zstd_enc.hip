// zstd encoder (RFC 8878): one wavefront encodes one unit into one complete frame (or, for the streaming encoder, one segment
// of a frame).  Persistent grid: each wave takes the next unit from a counter and keeps the block being built (sequences,
// literals, Huffman / FSE tables) in a per-wave HBM scratch; the hash table of the match finder lives in LDS.  The lanes share
// the match finder (64-position chunks, zstd_enc_core.h), the literal copy and histogram, the Huffman stream sizes and the Raw
// copies; the Huffman code and bit emission, the FSE state chain and the headers run on lane 0.
#include <mutex>

#include "chip_internal.h"
#include "launch_slots.h"
#include "zstd_enc_core.h"

namespace chip {

namespace {

struct ZEncArgs {
    BatchArgs b;
    uint32_t group, skip_shift;
    uint32_t wlog_single;  // a one-shot unit of at most 2^wlog_single bytes is a single-segment frame
    uint32_t wlog_window;  // any other frame declares a window of 2^wlog_window (and no match reaches further)
    uint32_t flags;        // ZF_*
    ZEncStream *stream;    // streaming encoder only: the state carried between segments (n == 1)
};

constexpr size_t SEQ_BYTES = (size_t)zenc::MAX_SEQ * sizeof(zenc::Seq);
constexpr size_t WAVE_SCRATCH = ((SEQ_BYTES + zenc::BLOCK_MAX + sizeof(zenc::Work)) + 255) & ~(size_t)255;

struct alignas(16) ZLds {
    uint16_t ht[zenc::HSIZE];  // 16 KiB
    zenc::Chunk k;             // 1.5 KiB
    uint32_t cnt[256];         // the block's literal histogram
};

// lane 0's global stores made visible to the other lanes (and theirs to lane 0) before the next step reads them
#define ZFENCE() do { __threadfence(); WSYNC(); } while (0)

__device__ __forceinline__ uint32_t zwave_sum(uint32_t v) { return rdlane(wave_incl_scan(v), 63); }

// All 64 lanes run this (control flow is uniform); the steps that must be serial -- the walk's decisions are computed by every lane
// alike, Huffman code construction and bit emission, the FSE chain, headers -- write from lane 0 only.  The kernel form of
// zenc::compress_segment (same steps, same bytes).
__device__ bool encode_segment_wave(const zenc::Cfg &c, ZLds &L, const zenc::Scratch &sc, const uint8_t *src, uint32_t n, bool last,
                                    uint32_t *rep, zenc::Out &o, unsigned long long *st)
{
    const uint32_t lane = lane_id();
    if (n == 0) {
        if (lane == 0 && last) o.put_le(1u, 3);
        o.pos = rdfirst(o.pos);
        o.ovf = rdfirst(o.ovf);
        return !o.ovf;
    }
    for (uint32_t bs = 0; bs < n; bs += c.block_max) {
        const uint32_t be = n - bs > c.block_max ? bs + c.block_max : n, bn = be - bs;
        const uint32_t lastbit = (last && be == n) ? 1u : 0u;
        const uint32_t hpos = o.pos;
        bool diff = false;
        for (uint32_t i = bs + 1 + lane; i < be; i += 64) diff |= src[i] != src[bs];
        if (bn > 1 && __ballot(diff) == 0) {  // RLE block
            if (lane == 0) {
                o.put_le(lastbit | (1u << 1) | (bn << 3), 3);
                o.put(src[bs]);
            }
            o.pos = rdfirst(o.pos);
            o.ovf = rdfirst(o.ovf);
            if (o.ovf) return false;
            continue;
        }
        const unsigned long long t0 = ZE_CLK();
        for (uint32_t i = lane; i < 256; i += 64) L.cnt[i] = 0;
        LSYNC();
        uint32_t ns = 0, nl = 0, anchor = bs, rep0 = rep[0], ip = bs;
        auto lits = [&](uint32_t a, uint32_t e) {  // lanes copy and count the literals src[a .. e)
            for (uint32_t i = a + lane; i < e; i += 64) {
                const uint8_t b = src[i];
                sc.lit[nl + (i - a)] = b;
                atomicAdd(&L.cnt[b], 1u);
            }
            nl += e - a;
        };
        auto emit = [&](uint32_t anc, uint32_t p, uint32_t ml, uint32_t off) {
            lits(anc, p);
            if (lane == 0) {
                sc.seq[ns].ll = p - anc;
                sc.seq[ns].ml = ml;
                sc.seq[ns].off = off;
            }
            ns++;
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
        lits(anchor, be);
        LSYNC();
        for (uint32_t i = lane; i < 256; i += 64) sc.w->cnt[i] = L.cnt[i];
        ZFENCE();
        const unsigned long long t1 = ZE_CLK();
        if (st && lane == 0) st[0] += t1 - t0;
        // lane 0: sequence codes (the repeat-offset history is a chain), the Huffman code
        uint32_t nrep[3] = {rep[0], rep[1], rep[2]}, maxl = 0;
        if (lane == 0) {
            zenc::seq_codes(sc.seq, ns, nrep);
            maxl = zenc::lit_prepare(*sc.w, sc.lit, nl);
        }
        maxl = rdfirst(maxl);
        ZFENCE();
        // lanes: the code lengths of the four stream segments
        uint32_t bits[5] = {0, 0, 0, 0, 0};
        if (maxl) {
            const uint32_t seg = (nl + 3) / 4;
            for (uint32_t kq = 0; kq < 4; kq++) {
                const uint32_t a = kq * seg, e = kq == 3 ? nl : (a + seg < nl ? a + seg : nl);
                uint32_t v = 0;
                for (uint32_t i = a + lane; i < e; i += 64) v += sc.w->hlen[sc.lit[i]];
                bits[kq] = zwave_sum(v);
            }
            bits[4] = bits[0] + bits[1] + bits[2] + bits[3];
        }
        const unsigned long long t2 = ZE_CLK();
        // lane 0: Huffman streams, sequences (FSE), the block header; Raw literals and a Raw block are copied by all lanes
        uint32_t raw_lit = 0xffffffffu, raw_blk = 0xffffffffu;
        unsigned long long t3 = t2;
        if (lane == 0) {
            o.pos = hpos + 3;
            zenc::lit_emit(*sc.w, o, sc.lit, nl, maxl, bits, false, &raw_lit);
            t3 = ZE_CLK();
            zenc::write_sequences(*sc.w, o, sc.seq, ns);
            const uint32_t csize = o.pos - hpos - 3;
            if (!o.ovf && csize < bn) {
                o.set(hpos, (lastbit | (2u << 1) | (csize << 3)) & 0xff);
                o.set(hpos + 1, (csize << 3 >> 8) & 0xff);
                o.set(hpos + 2, (csize << 3 >> 16) & 0xff);
                rep[0] = nrep[0];
                rep[1] = nrep[1];
                rep[2] = nrep[2];
            } else {  // raw block: the repeat offsets stay as they were
                raw_lit = 0xffffffffu;
                o.pos = hpos;
                o.ovf = false;
                o.put_le(lastbit | (bn << 3), 3);
                raw_blk = o.pos;
                if (o.pos + (uint64_t)bn > o.cap) o.ovf = true;
                o.pos += bn;
            }
        }
        o.pos = rdfirst(o.pos);
        o.ovf = rdfirst(o.ovf);
        rep[0] = rdfirst(rep[0]);
        rep[1] = rdfirst(rep[1]);
        rep[2] = rdfirst(rep[2]);
        raw_lit = rdfirst(raw_lit);
        raw_blk = rdfirst(raw_blk);
        if (o.ovf) return false;
        if (raw_lit != 0xffffffffu)
            for (uint32_t i = lane; i < nl; i += 64) o.p[raw_lit + i] = sc.lit[i];  // raw_lit + nl <= o.cap (no overflow)
        if (raw_blk != 0xffffffffu)
            for (uint32_t i = lane; i < bn; i += 64) o.p[raw_blk + i] = src[bs + i];
        ZFENCE();
        if (st && lane == 0) {
            const unsigned long long t4 = ZE_CLK();
            st[1] += (t2 - t1) + (t3 - t2);  // histogram follows the walk; code lengths, segment sums, Huffman streams
            st[2] += t4 - t3;
        }
    }
    return !o.ovf;
}

__device__ void encode_unit(const ZEncArgs &a, uint32_t u, ZLds &L, uint8_t *scratch)
{
    const uint32_t lane = lane_id();
    for (uint32_t i = lane; i < zenc::HSIZE; i += 64) L.ht[i] = 0;
    WSYNC();
    const uint32_t n = a.b.in_len[u], cap = a.b.out_cap[u];
    const uint8_t *src = a.b.in_base + a.b.in_off[u];
    zenc::Out o = {a.b.out_base + a.b.out_off[u], 0, cap, false};
    unsigned long long *st = a.b.stats ? a.b.stats + (size_t)u * 16 : nullptr;
    const unsigned long long t0 = ZE_CLK();
    const bool first = a.flags & ZF_FIRST, last = a.flags & ZF_LAST;
    const bool single = (a.flags & ZF_ONESHOT) && (uint64_t)n <= (1ull << a.wlog_single);
    zenc::Cfg c;
    c.group = a.group;
    c.skip_shift = a.skip_shift;
    const uint32_t window = single ? n : 1u << a.wlog_window;
    c.maxdist = window;
    c.block_max = window < zenc::BLOCK_MAX ? (window ? window : 1u) : zenc::BLOCK_MAX;
    uint32_t rep[3] = {1, 4, 8};
    if (!first) {
        rep[0] = a.stream->rep[0];
        rep[1] = a.stream->rep[1];
        rep[2] = a.stream->rep[2];
    }
    if (first && lane == 0) zenc::frame_header(o, single, n, a.wlog_window);
    o.pos = rdfirst(o.pos);
    o.ovf = rdfirst(o.ovf);
    zenc::Scratch sc;
    sc.ht = L.ht;
    sc.seq = (zenc::Seq *)scratch;
    sc.lit = scratch + SEQ_BYTES;
    sc.w = (zenc::Work *)(scratch + SEQ_BYTES + zenc::BLOCK_MAX);
    const unsigned long long t1 = ZE_CLK();
    bool ok = encode_segment_wave(c, L, sc, src, n, last, rep, o, st);
    const unsigned long long t2 = ZE_CLK();
    if (lane != 0) return;
    // XXH64 of the segment (four accumulators in a chain per 32-byte stripe: lane 0)
    zenc::Xxh x;
    if (first) zenc::xxh_init(x);
    else x = a.stream->xxh;
    zenc::xxh_update(x, src, n);
    if (last) o.put_le((uint32_t)zenc::xxh_digest(x), 4);
    ok = ok && !o.ovf;
    if (a.stream) {
        a.stream->rep[0] = rep[0];
        a.stream->rep[1] = rep[1];
        a.stream->rep[2] = rep[2];
        a.stream->xxh = x;
    }
    a.b.out_len[u] = ok ? o.pos : 0;
    a.b.status[u] = ok ? CHIP_ENC_FINISHED : CHIP_ENC_NEED_OUTPUT;
    if (st) {
        // [0] match finding + literal copy / histogram, [1] Huffman, [2] sequences / FSE + block, [3] frame: header, checksum, rest
        const unsigned long long t3 = ZE_CLK();
        st[3] += (t1 - t0) + (t3 - t2) + ((t2 - t1) - st[0] - st[1] - st[2]);
        st[4] += n;
        st[5] += o.pos;
    }
}

__global__ __launch_bounds__(64) void zstd_enc_kernel(ZEncArgs a, uint8_t *scratch, uint32_t *next_unit)
{
    __shared__ ZLds L;
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
SlotCache<WaveScratch> g_zenc_cache;
ResidentWaves g_zenc_resident;

}  // namespace

void zstd_enc_group(int level, int strategy, uint32_t &group, uint32_t &skip_shift)
{
    if (level == 0) level = 3;
    if (level > 22) level = 22;
    skip_shift = level < 0 ? (level < -6 ? 2u : (uint32_t)(8 + level)) : 8u;  // negative levels skip faster over misses
    switch (strategy) {
    case CHIP_ZSTD_STRATEGY_FAST: group = 0; return;
    case CHIP_ZSTD_STRATEGY_DFAST:
    case CHIP_ZSTD_STRATEGY_GREEDY: group = 1; return;
    case CHIP_ZSTD_STRATEGY_LAZY:
    case CHIP_ZSTD_STRATEGY_LAZY2: group = 2; return;
    case CHIP_ZSTD_STRATEGY_BTLAZY2:
    case CHIP_ZSTD_STRATEGY_BTOPT:
    case CHIP_ZSTD_STRATEGY_BTULTRA:
    case CHIP_ZSTD_STRATEGY_BTULTRA2: group = 3; return;
    default: break;
    }
    group = level < 3 ? 0u : level < 6 ? 1u : level < 13 ? 2u : 3u;
}

hipError_t launch_zstd_encode(const BatchArgs &b, int level, int strategy, uint32_t wlog_single, uint32_t wlog_window, uint32_t flags,
                              ZEncStream *stream_state, hipStream_t stream)
{
    if (b.n == 0) return hipSuccess;
    ZEncArgs a;
    a.b = b;
    zstd_enc_group(level, strategy, a.group, a.skip_shift);
    a.wlog_single = wlog_single;
    a.wlog_window = wlog_window;
    a.flags = flags;
    a.stream = stream_state;
    std::lock_guard<std::mutex> lk(g_zenc_cache.mu);  // from the slot's lookup to the launch
    WaveScratch *sl = nullptr;
    int max_blocks = 0;
    hipError_t e = g_zenc_cache.at(stream, sl);
    if (e == hipSuccess) e = g_zenc_resident.get((const void *)zstd_enc_kernel, max_blocks);
    if (e == hipSuccess) e = sl->reserve(stream, b.n, max_blocks, WAVE_SCRATCH);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(sl->counter, 0, 4, stream)) != hipSuccess) return e;
    const uint32_t blocks = b.n < (uint32_t)sl->blocks ? b.n : (uint32_t)sl->blocks;
    hipLaunchKernelGGL(zstd_enc_kernel, dim3(blocks), dim3(64), 0, stream, a, sl->scratch, sl->counter);
    return hipGetLastError();
}

}  // namespace chip
