// One large zstd frame, block by block: chip_zstd_parallel and its launches, and the first pass on its own,
// the description of the frame's blocks: chip_zstd_blocks_host on the host and chip_zstd_blocks on the GPU.  The token pass is
// zstd_unit.h's kernel body in zstd_tokens.hip; place, jump and deliver are below, behind the description.
//
// The description of a buffer is DEFINED by the walk of include/compu_hip.h.  walk_blocks, describe_block and defines below are
// its one text for host and device.
//   hop       zblocks_hop_kernel: one lane reads the frame header and then one 3-byte block header per block (chip_zstd_plan's
//             walk of one frame); offset, size, type and the last-block flag of every block, the summary
//   describe  zblocks_describe_kernel: one lane per block; a compressed block's literals section header and sequences section
//             header, and per kind whether the block defines a table (its own index) or not (-1)
//   sources   zblocks_sources_kernel: one workgroup; the exclusive running maximum of those four columns is the nearest earlier
//             definer
// Nothing is decoded.  No byte outside [0, len) is loaded, and what the later kernels read lies inside the body the hop has
// checked against len.  No wave waits for another.
// chip_zstd_parallel_next (sec. 4.20, at the end) runs the same passes over a SLAB of a frame of any length, from a cursor the caller
// carries: walk_slab is the hop from a block boundary, the place pass reads what lies in front of the slab from the window ring,
// and chip_zstd_slab_blocks_host, chip_zstd_cursor_header_host and the chip_xxh64 pair are the host twins of its steps.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chip_internal.h"
#include "launch_slots.h"
#include "plan_common.h"

namespace chip {

namespace {

constexpr uint32_t ZSTD_FRAME_MAGIC = 0xFD2FB528u;
constexpr uint32_t SRC_THREADS = 1024;

__host__ __device__ __forceinline__ uint64_t le_field(const uint8_t *b, uint32_t n)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < n; k++) v |= (uint64_t)b[k] << (8 * k);
    return v;
}

// The walk: the summary, and offset / size / type / flags of the first min(n_blocks, max_blocks) blocks.  Reads bytes of [0, len).
__host__ __device__ __forceinline__ chip_zstd_blocks_summary walk_blocks(const uint8_t *in, uint64_t len, uint64_t max_blocks, chip_zstd_block *blocks)
{
    chip_zstd_blocks_summary r{0, 0, CHIP_ZBLOCKS_UNSIZED, 0, CHIP_ZPLAN_OK, 0, 0, 0};
    if (len < 4) return r.status = CHIP_ZPLAN_TRUNCATED, r;
    if ((uint32_t)le_field(in, 4) != ZSTD_FRAME_MAGIC) return r.status = CHIP_ZPLAN_BAD_HEADER, r;
    if (len < 5) return r.status = CHIP_ZPLAN_TRUNCATED, r;
    const uint32_t fhd = in[4], f = fhd >> 6, ss = (fhd >> 5) & 1u, d = fhd & 3u;
    const uint32_t did_bytes = d == 3 ? 4u : d, fcs_bytes = f == 0 ? ss : 1u << f, fcs_at = 5u + (ss ? 0u : 1u) + did_bytes;
    const uint32_t hs = fcs_at + fcs_bytes;
    r.descriptor = fhd;
    if (len < hs) return r.status = CHIP_ZPLAN_TRUNCATED, r;
    r.header_bytes = hs;
    if (fcs_bytes) r.content_size = le_field(in + fcs_at, fcs_bytes) + (fcs_bytes == 2 ? 256u : 0u);
    if (ss) {
        r.window_size = r.content_size;
    } else {
        const uint32_t wd = in[5], wl = 10u + (wd >> 3);
        r.window_size = (1ull << wl) + ((1ull << wl) >> 3) * (wd & 7u);
    }
    uint64_t q = hs, n = 0;
    for (;;) {
        if (len - q < 3) return r.n_blocks = n, r.status = CHIP_ZPLAN_TRUNCATED, r;
        const uint32_t h = (uint32_t)le_field(in + q, 3), type = (h >> 1) & 3u;
        if (type == 3) return r.n_blocks = n, r.status = CHIP_ZPLAN_BAD_HEADER, r;
        if (n + 1 > CHIP_ZPLAN_MAX_BLOCKS) return r.n_blocks = n, r.status = CHIP_ZPLAN_TOO_LARGE, r;
        const uint64_t body = type == 1 ? 1u : h >> 3;
        if (body > len - q - 3) return r.n_blocks = n, r.status = CHIP_ZPLAN_TRUNCATED, r;
        if (n < max_blocks) {
            chip_zstd_block b{};
            b.offset = q;
            b.size = h >> 3;
            b.type = (uint8_t)type;
            b.flags = (uint8_t)(h & 1u);
            blocks[n] = b;
        }
        n++;
        q += 3 + body;
        if (h & 1u) break;
    }
    r.n_blocks = n;
    if (fhd & 4u) {
        if (len - q < 4) return r.status = CHIP_ZPLAN_TRUNCATED, r;
        q += 4;
    }
    r.in_used = q;
    return r;
}

// The section headers of a compressed block whose offset, size and type the walk has filled; a raw or RLE block is left as it is.
// Reads bytes of the block's body only.
__host__ __device__ __forceinline__ void describe_block(const uint8_t *in, chip_zstd_block &b)
{
    if (b.type != 2) return;
    const uint8_t *p = in + b.offset + 3;
    const uint32_t size = b.size;
    b.flags |= CHIP_ZBLOCK_MALFORMED;  // until both headers have been read
    if (size < 1) return;
    const uint32_t b0 = p[0], lt = b0 & 3u, sf = (b0 >> 2) & 3u;
    uint32_t lh, regen, comp;
    if (lt < 2) {
        lh = sf == 1 ? 2u : sf == 3 ? 3u : 1u;
        if (size < lh) return;
        regen = lh == 1 ? b0 >> 3 : (uint32_t)le_field(p, lh) >> 4;
        comp = lt == 0 ? regen : 1u;
    } else {
        lh = sf < 2 ? 3u : sf + 2u;
        if (size < lh) return;
        const uint32_t bits = sf < 2 ? 10u : sf == 2 ? 14u : 18u;
        const uint64_t v = le_field(p, lh);
        regen = (uint32_t)(v >> 4) & ((1u << bits) - 1u);
        comp = (uint32_t)(v >> (4 + bits)) & ((1u << bits) - 1u);
    }
    b.lit_type = (uint8_t)lt;
    b.lit_regen = regen;
    b.lit_comp = comp;
    const uint64_t sq = (uint64_t)lh + comp;  // where the sequences section begins
    if (sq >= size) return;
    const uint32_t s0 = p[sq];
    uint32_t nseq = s0, sh = 1;
    if (s0 >= 128) {
        sh = s0 == 255 ? 3u : 2u;
        if (size - sq < sh) return;
        nseq = s0 == 255 ? (uint32_t)p[sq + 1] + ((uint32_t)p[sq + 2] << 8) + 0x7F00u : ((s0 - 128u) << 8) + p[sq + 1];
    }
    if (nseq) {
        if (size - sq < sh + 1) return;
        const uint32_t m = p[sq + sh];
        b.mode[0] = (uint8_t)(m >> 6);
        b.mode[1] = (uint8_t)((m >> 4) & 3u);
        b.mode[2] = (uint8_t)((m >> 2) & 3u);
    }
    b.n_seq = nseq;
    b.flags &= (uint8_t)~CHIP_ZBLOCK_MALFORMED;
}

// does the described block define the table of kind k (CHIP_ZSRC_*)
__host__ __device__ __forceinline__ bool defines(const chip_zstd_block &b, uint32_t k)
{
    if (b.type != 2 || (b.flags & CHIP_ZBLOCK_MALFORMED)) return false;
    if (k == CHIP_ZSRC_HUF) return b.lit_type == 2;
    return b.n_seq > 0 && b.mode[k - 1] != 3;
}

// The walk from a block boundary (chip_zstd_parallel_next, sec. 4.20): no frame header in front, whole blocks only.  It stops behind
// the last block, at a cut block (which is no error), at a reserved type or a Block_Size above block_max, or with stop_at blocks.
__host__ __device__ __forceinline__ chip_zstd_slab_summary walk_slab(const uint8_t *in, uint64_t len, uint64_t block_max, uint64_t max_blocks,
                                                                     uint64_t stop_at, chip_zstd_block *blocks)
{
    chip_zstd_slab_summary r{0, 0, CHIP_ZPLAN_TRUNCATED, 0};
    uint64_t q = 0, n = 0;
    for (;;) {
        if (len - q < 3) break;
        const uint32_t h = (uint32_t)le_field(in + q, 3), type = (h >> 1) & 3u;
        if (type == 3 || (h >> 3) > block_max) {
            r.status = CHIP_ZPLAN_BAD_HEADER;
            break;
        }
        if (n + 1 > stop_at) {
            r.status = CHIP_ZPLAN_TOO_LARGE;
            break;
        }
        const uint64_t body = type == 1 ? 1u : h >> 3;
        if (body > len - q - 3) break;
        if (n < max_blocks) {
            chip_zstd_block b{};
            b.offset = q;
            b.size = h >> 3;
            b.type = (uint8_t)type;
            b.flags = (uint8_t)(h & 1u);
            blocks[n] = b;
        }
        n++;
        q += 3 + body;
        if (h & 1u) {
            r.status = CHIP_ZPLAN_OK;
            r.last = 1;
            break;
        }
    }
    r.n_blocks = n;
    r.in_used = q;
    return r;
}

__global__ __launch_bounds__(64) void zslab_hop_kernel(const uint8_t *in, uint64_t len, uint64_t block_max, uint64_t cap, chip_zstd_block *blocks,
                                                       chip_zstd_slab_summary *sum)
{
    if (threadIdx.x == 0) *sum = walk_slab(in, len, block_max, cap, cap, blocks);
}

__global__ __launch_bounds__(64) void zblocks_hop_kernel(const uint8_t *in, uint64_t len, uint64_t max_blocks, chip_zstd_block *blocks,
                                                         chip_zstd_blocks_summary *sum)
{
    if (threadIdx.x == 0) *sum = walk_blocks(in, len, max_blocks, blocks);
}

// src[k] of block i becomes i where the block defines kind k, else -1
__global__ __launch_bounds__(256) void zblocks_describe_kernel(const uint8_t *in, chip_zstd_block *blocks, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    chip_zstd_block b = blocks[i];
    describe_block(in, b);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) b.src[k] = defines(b, k) ? (int32_t)i : -1;
    blocks[i] = b;
}

// src[k] of block i becomes the maximum of the column over the blocks in front of i (-1: there is none).  One workgroup: a tile of
// SRC_THREADS blocks per trip, the running maximum inside a wave, over the waves of the tile and carried from tile to tile.
__global__ __launch_bounds__(SRC_THREADS) void zblocks_sources_kernel(chip_zstd_block *blocks, uint32_t n)
{
    constexpr uint32_t NW = SRC_THREADS / 64;
    __shared__ int32_t s_wave[4][NW];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    int32_t carry[4] = {-1, -1, -1, -1};
    for (uint32_t t0 = 0; t0 < n; t0 += SRC_THREADS) {
        const uint32_t i = t0 + threadIdx.x;
        int32_t exc[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            int32_t inc = i < n ? blocks[i].src[k] : -1;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const int32_t t = __shfl_up(inc, d, 64);
                if (lane >= d) inc = inc > t ? inc : t;
            }
            exc[k] = __shfl_up(inc, 1, 64);
            if (lane == 0) exc[k] = -1;
            if (lane == 63) s_wave[k][wave] = inc;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            int32_t before = carry[k], total = carry[k];
            for (uint32_t w = 0; w < NW; w++) {
                const int32_t c = s_wave[k][w];
                if (w < wave) before = before > c ? before : c;
                total = total > c ? total : c;
            }
            if (i < n) blocks[i].src[k] = exc[k] > before ? exc[k] : before;
            carry[k] = total;
        }
        __syncthreads();  // (the next trip's maxima stay behind these reads)
    }
}

// the summary only; a launch slot
using ZblocksSlot = SummarySlot<chip_zstd_blocks_summary>;
SlotCache<ZblocksSlot> g_zblocks_cache;

constexpr chip_zstd_blocks_summary NO_FRAME{0, 0, CHIP_ZBLOCKS_UNSIZED, 0, CHIP_ZPLAN_TRUNCATED, 0, 0, 0};

// ---- chip_zstd_parallel: place, jump, deliver (the token pass is zstd_tokens.hip) -----------------------------------------------
// One 32-bit word per content byte: W_FINAL | byte, or the position the byte is a copy of (always a smaller one).
constexpr uint32_t W_FINAL = 0x80000000u, TOK_SYM = 0x80000000u;

constexpr uint32_t NO_BAD = 0xFFFFFFFFu;
struct ZparDev {
    uint32_t bad;   // place: the first block with a token that does not fit it or an offset beyond the content before it or the window
    uint32_t left;  // jump: words that are still not final after the round
    uint32_t xxh;   // the low 32 bits of the content's XXH64
    uint32_t pad;
    chip_zstd_slab_summary slab;  // chip_zstd_parallel_next: the walk from the cursor
    chip_xxh64_state state;       // and the running checksum behind the call's bytes
};

// Place: one wave per block.  Raw and RLE blocks are final bytes.  A compressed block's sequences are taken 64 at a time: the
// symbolic offsets get the block's incoming repeat offsets, a wave prefix sum of literal length + match length places them, and the
// words of the group are written destination-driven (lane d finds the sequence that owns byte d by a search over the 64 sums), as
// pack_copy.h's copy is: sequences average a few tens of bytes.  Every offset is checked here against the content before the match
// and the window.  Nothing outside [pos[u], pos[u] + size[u]) is written.
// HIST (chip_zstd_parallel_next): position 0 is not the frame's first byte.  `hist` bytes of content lie in front of it in `ring`, a
// ring of `window` bytes whose next free byte is ring_at: a destination whose source lies there reads the byte and is final at once.
template <bool HIST>
__global__ __launch_bounds__(64) void zpar_place_kernel(const uint8_t *in, const chip_zstd_block *blocks, const uint32_t *pos, const uint32_t *size,
                                                        const uint32_t *seq_base, const uint32_t *tok, const uint32_t *res, const uint32_t *rep_in,
                                                        const uint64_t *unit_off, const uint8_t *slots, const uint64_t *slot_off, uint64_t window, uint32_t *W, ZparDev *dv, uint64_t hist, const uint8_t *ring, uint64_t ring_at)
{
    __shared__ uint32_t s_incl[64], s_ll[64], s_litb[64], s_off[64];
    const uint32_t u = blockIdx.x, lane = lane_id();
    const chip_zstd_block b = blocks[u];
    const uint32_t P = pos[u], n = size[u];
    if (b.type != 2) {
        const uint8_t *src = in + b.offset + 3;
        for (uint32_t j = lane; j < n; j += 64) W[P + j] = W_FINAL | src[b.type == 0 ? j : 0];
        return;
    }
    const uint32_t *r = res + 8 * u;
    const uint32_t lit_mode = r[3], lit_at = r[4], regen = r[5];
    const uint8_t *lit = lit_mode == 0 ? in + unit_off[u] + lit_at : slots + slot_off[u] + lit_at;
    const uint32_t r0 = rep_in[3 * u], r1 = rep_in[3 * u + 1], r2 = rep_in[3 * u + 2];
    const uint32_t nseq = b.n_seq;
    const uint32_t *t = tok + 3 * (size_t)seq_base[u];
    uint32_t opos = 0, lpos = 0;
    bool bad = false;
    for (uint32_t i0 = 0; i0 < nseq && !bad; i0 += 64) {
        const uint32_t cn = nseq - i0 < 64 ? nseq - i0 : 64;
        uint32_t ll = 0, ml = 0, off = 1;
        if (lane < cn) {
            ll = t[3 * (i0 + lane)];
            ml = t[3 * (i0 + lane) + 1];
            off = t[3 * (i0 + lane) + 2];
            if (off & TOK_SYM) {
                const uint32_t k = (off >> 29) & 3u, back = off & 0x1FFFFFFFu, rr = k == 0 ? r0 : k == 1 ? r1 : r2;
                off = rr > back ? rr - back : 1u;
            }
        }
        const uint32_t tot = ll + ml;
        uint32_t incl = tot, lincl = ll;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t a = __shfl_up(incl, d, 64), c = __shfl_up(lincl, d, 64);
            if (lane >= d) {
                incl += a;
                lincl += c;
            }
        }
        const uint32_t OB = __shfl(incl, 63, 64), LB = __shfl(lincl, 63, 64);
        const uint32_t mstart = opos + incl - tot + ll;
        bool mine_bad = lane < cn && ((uint64_t)off > (HIST ? hist : 0ull) + P + mstart || off > window || off == 0);
        if ((uint64_t)opos + OB > n || (uint64_t)lpos + LB > regen) mine_bad = true;
        if (__any(mine_bad)) {
            bad = true;
            break;
        }
        s_incl[lane] = incl;
        s_ll[lane] = ll;
        s_litb[lane] = lincl - ll;
        s_off[lane] = off;
        __syncthreads();
        for (uint32_t d = lane; d < OB; d += 64) {
            uint32_t s = 0;
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1)
                if (s_incl[s + step - 1] <= d) s += step;
            const uint32_t rel = d - (s ? s_incl[s - 1] : 0u), p = P + opos + d;
            if (HIST && rel >= s_ll[s] && s_off[s] > p) {  // (s_off - p <= hist <= window)
                uint64_t at = ring_at + window - (s_off[s] - p);
                at -= at >= window ? window : 0ull;
                W[p] = W_FINAL | ring[at];
                continue;
            }
            W[p] = rel < s_ll[s] ? (W_FINAL | (lit_mode == 1 ? lit_at : lit[lpos + s_litb[s] + rel])) : p - s_off[s];
        }
        __syncthreads();
        opos += OB;
        lpos += LB;
    }
    if (!bad) {
        const uint32_t restl = regen - lpos;
        if ((uint64_t)opos + restl != n) bad = true;
        else
            for (uint32_t j = lane; j < restl; j += 64) W[P + opos + j] = W_FINAL | (lit_mode == 1 ? lit_at : lit[lpos + j]);
    }
    if (bad && lane == 0) atomicMin(&dv->bad, u);
}

// Jump: W[p] = W[W[p]] for every word that is not final, in place.  A racing read sees the old or the new word of its target, both
// of which are correct states of it (a final byte, or a smaller position with the same byte), and aligned 32-bit accesses do not
// tear: the result is deterministic, the round count need not be.  Four words per lane in one 16-byte load; only the words that
// are not final gather.  dv->left counts what is still open.
__global__ __launch_bounds__(256) void zpar_jump_kernel(uint32_t *W, uint32_t n, ZparDev *dv)
{
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    uint32_t left = 0;
    if (i < n) {
        uint32_t w[4] = {W_FINAL, W_FINAL, W_FINAL, W_FINAL};
        const uint32_t have = n - i < 4 ? (uint32_t)(n - i) : 4u;  // (the room is padded to a multiple of four words)
        const uint4 v = *(const uint4 *)(W + i);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (k < have && !(w[k] & W_FINAL)) {
                const uint32_t t = W[w[k]];
                W[i + k] = t;
                left += (t & W_FINAL) ? 0u : 1u;
            }
        }
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) left += __shfl_down(left, d, 64);
    if (lane_id() == 0 && left) atomicAdd(&dv->left, left);
}

// Deliver: the low bytes of the words
__global__ __launch_bounds__(256) void zpar_deliver_kernel(const uint32_t *W, uint32_t n, uint8_t *out)
{
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i >= n) return;
    const uint4 v = *(const uint4 *)(W + i);
    if (n - i >= 4 && ((uintptr_t)(out + i) & 3u) == 0) {
        *(uint32_t *)(out + i) = (v.x & 255u) | ((v.y & 255u) << 8) | ((v.z & 255u) << 16) | (v.w << 24);
    } else {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t k = 0; k < 4 && i + k < n; k++) out[i + k] = (uint8_t)w[k];
    }
}

// buffer 0: the block arrays, the tokens and the literal slots; buffer 1: the words
// (blk: the block records of chip_zstd_parallel_next's walk, which are written before the rest of a call's room is known)
struct ZparSlot : SummarySlot<ZparDev> {
    uint8_t *blk = nullptr;
    size_t blk_cap = 0;
    void free()
    {
        (void)hipFree(blk);
        blk = nullptr;
        blk_cap = 0;
        SummarySlot<ZparDev>::free();
    }
};
SlotCache<ZparSlot> g_zpar_cache;

struct ZparCall {
    const uint8_t *in;
    uint64_t len;
    uint8_t *out;
    uint64_t out_cap;
    int wlog_max;
    uint32_t flags;
    chip_zstd_parallel_summary *sum;
};

// phase times on stderr with CHIP_ZPAR_TIMING=1 (tools/time_zstd_parallel.py reads them); each mark waits for the stream
struct ZparClock {
    bool on;
    hipStream_t s;
    std::chrono::steady_clock::time_point t;
    ZparClock(hipStream_t stream) : on(getenv("CHIP_ZPAR_TIMING") != nullptr), s(stream), t(std::chrono::steady_clock::now()) {}
    void mark(const char *what, long long extra = -1)
    {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t).count();
        if (extra >= 0) fprintf(stderr, "zpar %s %.3f ms left %lld\n", what, ms, extra);
        else fprintf(stderr, "zpar %s %.3f ms\n", what, ms);
        t = std::chrono::steady_clock::now();
    }
};

// The serial path: the one-unit batch decode, whose answer this is.
hipError_t zpar_serial(ZparSlot &sl, const ZparCall &c, uint64_t unit_len, hipStream_t s)
{
    chip_zstd_parallel_summary &o = *c.sum;
    o = chip_zstd_parallel_summary{0, 0, 0, 0, 0, 0, CHIP_ZPAR_SERIAL, 0, 0};
    if (unit_len > ((uint64_t)1 << 28) || c.out_cap > 0xFFFFFFFFull) {  // does not fit a unit
        o.path = CHIP_ZPAR_REFUSED;
        return hipSuccess;
    }
    hipError_t e = sl.grow(0, 64);
    if (e != hipSuccess) return e;
    struct Unit {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len, in_used;
        int32_t status;
        uint32_t pad;
    } h{0, 0, (uint32_t)unit_len, (uint32_t)c.out_cap, 0, 0, 0, 0};
    Unit *d = (Unit *)sl.buf[0];
    if ((e = hipMemcpyAsync(d, &h, sizeof h, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    BatchArgs a{};
    a.in_base = c.in;
    a.in_off = &d->in_off;
    a.in_len = &d->in_len;
    a.out_base = c.out;
    a.out_off = &d->out_off;
    a.out_cap = &d->out_cap;
    a.out_len = &d->out_len;
    a.in_used = &d->in_used;
    a.status = &d->status;
    a.n = 1;
    a.format = CHIP_FMT_ZSTD;
    if ((e = launch_zstd(a, nullptr, c.wlog_max, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    o.out_len = o.total_out = h.out_len;
    o.in_used = h.in_used;
    o.status = h.status;
    return hipSuccess;
}

inline uint32_t sym_value(uint32_t v, const uint32_t rep[3])
{
    if (!(v & TOK_SYM)) return v;
    const uint32_t rr = rep[(v >> 29) & 3u], back = v & 0x1FFFFFFFu;
    return rr > back ? rr - back : 1u;
}

// The parallel path.  serial = true on return: the frame is not one for it (or not clean) and nothing the caller sees was decided.
hipError_t zpar_parallel(ZparSlot &sl, const ZparCall &c, hipStream_t s, bool &serial, uint64_t &unit_len)
{
    serial = true;
    ZparClock clock(s);
    if (c.len < 8) return hipSuccess;
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    // 1. describe
    chip_zstd_blocks_summary bs;
    if (const int rc = chip_zstd_blocks(c.in, c.len, 0, nullptr, &bs, s)) return rc == CHIP_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;
    const int wl = c.wlog_max ? c.wlog_max : 27;
    if (bs.status == CHIP_ZPLAN_OK) unit_len = bs.in_used;  // a whole first frame: what follows it is not the unit's business
    if (bs.status != CHIP_ZPLAN_OK || bs.n_blocks < 2 || (bs.descriptor & 8u) || wl > 31 || bs.window_size > ((uint64_t)1 << wl)) return hipSuccess;
    if (bs.content_size != CHIP_ZBLOCKS_UNSIZED && bs.content_size >= ((uint64_t)1 << 31)) return hipSuccess;
    uint8_t head[24] = {0};
    if ((e = hipMemcpyAsync(head, c.in, bs.header_bytes < 24 ? bs.header_bytes : 24, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    {
        const uint32_t d = bs.descriptor & 3u, did_bytes = d == 3 ? 4u : d, at = 5u + ((bs.descriptor >> 5) & 1u ? 0u : 1u);
        for (uint32_t k = 0; k < did_bytes; k++)
            if (head[at + k]) return hipSuccess;  // a dictionary: the serial decode says what that is
    }
    const uint32_t n = (uint32_t)bs.n_blocks;
    if ((e = sl.grow(0, (size_t)n * sizeof(chip_zstd_block))) != hipSuccess) return e;
    if (const int rc = chip_zstd_blocks(c.in, c.len, n, (chip_zstd_block *)sl.buf[0], &bs, s)) return rc == CHIP_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;
    if (bs.status != CHIP_ZPLAN_OK || bs.n_blocks != n) return hipSuccess;  // (input that changed)
    std::vector<chip_zstd_block> recs(n);
    if ((e = hipMemcpyAsync(recs.data(), sl.buf[0], (size_t)n * sizeof(chip_zstd_block), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    clock.mark("describe");
    // the room: block arrays, tokens, literal slots
    const uint64_t bmax = bs.window_size < 131072 ? bs.window_size : 131072;
    // A unit of the token pass is the span from the earliest block its wave reads (the sources of the tables its block reuses)
    // to the end of its own block, from a 4-byte boundary: the kernel body's cursors are 32-bit BIT positions, so the span, not
    // the frame, has to stay below 2^28 bytes.
    std::vector<uint32_t> seq_base(n), span_len(n);
    std::vector<uint64_t> slot_off(n), unit_off(n);
    uint64_t n_seq = 0, slot_total = 0;
    for (uint32_t i = 0; i < n; i++) {
        const chip_zstd_block &b = recs[i];
        if ((b.flags & CHIP_ZBLOCK_MALFORMED) || b.lit_regen > 131072 || (b.type != 2 && b.size > bmax)) return hipSuccess;
        uint64_t first = b.offset;
        if (b.type == 2) {
            for (uint32_t k = 0; k < 4; k++) {
                if (!(k == 0 ? b.lit_type == 3 : (b.n_seq != 0 && b.mode[k - 1] == 3))) continue;
                if (b.src[k] < 0 || (uint32_t)b.src[k] >= i) return hipSuccess;  // a reuse without a source
                if (recs[b.src[k]].offset < first) first = recs[b.src[k]].offset;
            }
        }
        first &= ~(uint64_t)3;
        const uint64_t span = b.offset + 3 + (b.type == 1 ? 1u : b.size) - first;
        if (span > ((uint64_t)1 << 28)) return hipSuccess;  // (sources 256 MiB back: the serial decode's, if it fits a unit)
        unit_off[i] = first;
        span_len[i] = (uint32_t)span;
        seq_base[i] = (uint32_t)n_seq;
        slot_off[i] = slot_total;
        n_seq += b.n_seq;
        if (b.type == 2 && b.lit_type >= 2) slot_total += up16((size_t)b.lit_regen + ZTOK_SLOT_SLACK);
        if (n_seq > ((uint64_t)1 << 30)) return hipSuccess;
    }
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += up16(bytes);
        return at;
    };
    const size_t o_blocks = take((size_t)n * sizeof(chip_zstd_block)), o_in_off = take((size_t)n * 8), o_out_off = take((size_t)n * 8),
                 o_in_len = take((size_t)n * 4), o_out_cap = take((size_t)n * 4), o_seq = take((size_t)n * 4), o_up_end = o,
                 o_out_len = take((size_t)n * 4), o_in_used = take((size_t)n * 4), o_status = take((size_t)n * 4), o_res = take((size_t)n * 32),
                 o_pos = take((size_t)n * 4), o_rep = take((size_t)n * 12), o_tok = take((size_t)n_seq * 12 + 16), o_slots = take((size_t)slot_total + 16);
    if ((e = sl.grow(0, o)) != hipSuccess) return e;
    uint8_t *const base = sl.buf[0];
    {
        std::vector<uint8_t> up(o_up_end, 0);
        memcpy(&up[o_blocks], recs.data(), (size_t)n * sizeof(chip_zstd_block));
        for (uint32_t i = 0; i < n; i++) {
            const chip_zstd_block &b = recs[i];
            const uint32_t cap = b.type == 2 && b.lit_type >= 2 ? (uint32_t)up16((size_t)b.lit_regen + ZTOK_SLOT_SLACK) : 0u;
            ((uint64_t *)&up[o_out_off])[i] = slot_off[i];
            ((uint64_t *)&up[o_in_off])[i] = unit_off[i];
            ((uint32_t *)&up[o_in_len])[i] = span_len[i];
            ((uint32_t *)&up[o_out_cap])[i] = cap;
            ((uint32_t *)&up[o_seq])[i] = seq_base[i];
        }
        if ((e = hipMemcpyAsync(base, up.data(), o_up_end, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;  // (the staging vector goes away)
    }
    // 2. tokens
    BatchArgs a{};
    a.in_base = c.in;
    a.in_off = (const uint64_t *)(base + o_in_off);
    a.in_len = (const uint32_t *)(base + o_in_len);
    a.out_base = base + o_slots;
    a.out_off = (const uint64_t *)(base + o_out_off);
    a.out_cap = (const uint32_t *)(base + o_out_cap);
    a.out_len = (uint32_t *)(base + o_out_len);
    a.in_used = (uint32_t *)(base + o_in_used);
    a.status = (int32_t *)(base + o_status);
    a.n = n;
    a.format = CHIP_FMT_ZSTD;
    const ZTokArgs tk{(const chip_zstd_block *)(base + o_blocks), (const uint32_t *)(base + o_seq), (uint32_t *)(base + o_tok), (uint32_t *)(base + o_res),
                      bs.window_size};
    if ((e = launch_zstd_tokens(a, tk, s)) != hipSuccess) return e;
    std::vector<uint32_t> out_len(n), res((size_t)n * 8);
    std::vector<int32_t> status(n);
    if ((e = hipMemcpyAsync(out_len.data(), base + o_out_len, (size_t)n * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(status.data(), base + o_status, (size_t)n * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(res.data(), base + o_res, (size_t)n * 32, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    clock.mark("tokens");
    // 3. compose
    std::vector<uint32_t> pos(n), rep_in((size_t)n * 3);
    uint64_t total = 0;
    uint32_t rep[3] = {1, 4, 8};
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] != CHIP_FINISHED || out_len[i] > bmax) return hipSuccess;
        if (total >= ((uint64_t)1 << 31)) return hipSuccess;
        pos[i] = (uint32_t)total;
        total += out_len[i];
        for (uint32_t k = 0; k < 3; k++) rep_in[3 * (size_t)i + k] = rep[k];
        if (recs[i].type == 2) {
            const uint32_t nr[3] = {sym_value(res[8 * (size_t)i], rep), sym_value(res[8 * (size_t)i + 1], rep), sym_value(res[8 * (size_t)i + 2], rep)};
            rep[0] = nr[0];
            rep[1] = nr[1];
            rep[2] = nr[2];
        }
    }
    if (total >= ((uint64_t)1 << 31) || (bs.content_size != CHIP_ZBLOCKS_UNSIZED && bs.content_size != total)) return hipSuccess;
    if ((e = hipMemcpyAsync(base + o_pos, pos.data(), (size_t)n * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(base + o_rep, rep_in.data(), (size_t)n * 12, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    // (where the checksum is compared the bytes are delivered behind the words first: the room sees them once they are verified)
    const bool compare = (bs.descriptor & 4u) != 0 && !(c.flags & CHIP_ZPAR_NO_CHECKSUM);
    const size_t w_bytes = up16(((size_t)total + 4) * 4);
    if ((e = sl.grow(1, w_bytes + (compare ? up16((size_t)total) : 0))) != hipSuccess) return e;
    uint32_t *const W = (uint32_t *)sl.buf[1];
    // 4. place
    if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(ZparDev), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(&sl.d_sum->bad, 0xFF, 4, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(zpar_place_kernel<false>, dim3(n), dim3(64), 0, s, c.in, tk.blocks, (const uint32_t *)(base + o_pos), (const uint32_t *)a.out_len, tk.seq_base,
                       (const uint32_t *)tk.tok, (const uint32_t *)tk.res, (const uint32_t *)(base + o_rep), a.in_off, (const uint8_t *)a.out_base, a.out_off,
                       bs.window_size, W, sl.d_sum, (uint64_t)0, (const uint8_t *)nullptr, (uint64_t)0);
    if ((e = sl.fetch(s)) != hipSuccess) return e;  // (pos and rep_in have left the host by now)
    clock.mark("place");
    if (sl.h_sum->bad != NO_BAD) return hipSuccess;
    chip_zstd_parallel_summary &r = *c.sum;
    r = chip_zstd_parallel_summary{n, n_seq, 0, bs.in_used, total, CHIP_FINISHED, CHIP_ZPAR_PARALLEL, 0, 0};
    if (total > c.out_cap) {  // the exact size to come back with (a checksum is compared by the call that has the room)
        r.status = CHIP_NEED_OUTPUT;
        serial = false;
        return hipSuccess;
    }
    // 5. jump
    const uint32_t n_words = (uint32_t)total, grid = (uint32_t)((total + 1023) / 1024);
    uint32_t rounds = 0, left = n_words ? 1u : 0u;
    while (left && rounds < CHIP_ZPAR_ROUNDS_MAX) {
        if ((e = hipMemsetAsync(&sl.d_sum->left, 0, 4, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(zpar_jump_kernel, dim3(grid), dim3(256), 0, s, W, n_words, sl.d_sum);
        if ((e = sl.fetch(s)) != hipSuccess) return e;
        left = sl.h_sum->left;
        rounds++;
        clock.mark("jump", left);
    }
    if (left) return hipSuccess;  // (cannot happen below 2^31 bytes: the reach of every pointer at least doubles per round)
    // 6. deliver
    uint8_t *const bytes = compare ? sl.buf[1] + w_bytes : c.out;
    if (n_words) hipLaunchKernelGGL(zpar_deliver_kernel, dim3(grid), dim3(256), 0, s, (const uint32_t *)W, n_words, bytes);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    clock.mark("deliver");
    if (compare) {
        uint8_t want[4];
        if ((e = launch_zstd_xxh(bytes, n_words, &sl.d_sum->xxh, s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(want, c.in + bs.in_used - 4, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = sl.fetch(s)) != hipSuccess) return e;
        clock.mark("checksum");
        if (sl.h_sum->xxh != ((uint32_t)want[0] | ((uint32_t)want[1] << 8) | ((uint32_t)want[2] << 16) | ((uint32_t)want[3] << 24))) return hipSuccess;
        if (n_words && (e = hipMemcpyAsync(c.out, bytes, n_words, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        clock.mark("copy");
    } else if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    r.out_len = total;
    r.rounds = rounds;
    serial = false;
    return hipSuccess;
}

// ---- chip_zstd_parallel_next: the same passes over a SLAB of a frame, from a carried cursor -------------------
static_assert(sizeof(chip_xxh64_state) == sizeof(zenc::Xxh) && offsetof(chip_xxh64_state, tail) == offsetof(zenc::Xxh, mem) &&
                  offsetof(chip_xxh64_state, tail_n) == offsetof(zenc::Xxh, memsize) && offsetof(chip_xxh64_state, total) == offsetof(zenc::Xxh, total),
              "chip_xxh64_state is the encoder's running XXH64");
static_assert(CHIP_ZCUR_SLOT_BYTES >= 131072 + 3 && CHIP_ZCUR_SLOT_BYTES % 16 == 0, "a carry slot holds a block of Block_Maximum_Size");

constexpr uint64_t BLOCK_MAX_BYTES = 131072;

inline uint64_t ring_mod(uint64_t v, uint64_t window) { return window ? v % window : 0; }

// Is the cursor one a call has left?
bool cursor_ok(const chip_zstd_cursor &c)
{
    if (c.phase > CHIP_ZCUR_ERROR) return false;
    if (c.phase == CHIP_ZCUR_HEADER) return c.in_total == 0 && c.out_total == 0;
    if (c.phase == CHIP_ZCUR_ERROR) return c.error < 0;
    if (c.hist != (c.out_total < c.window_size ? c.out_total : c.window_size) || c.ring != ring_mod(c.out_total, c.window_size)) return false;
    if (c.waived > 1 || c.xxh.tail_n > 31 || !c.rep[0] || !c.rep[1] || !c.rep[2]) return false;
    if ((c.descriptor & 4u) && !c.waived && (c.xxh.total != c.out_total || c.xxh.tail_n != (c.out_total & 31u))) return false;
    for (uint32_t k = 0; k < 4; k++)
        if (c.carry_len[k] && (c.carry_len[k] < 3 || c.carry_len[k] > BLOCK_MAX_BYTES + 3 || c.carry_at[k] + c.carry_len[k] > c.in_total)) return false;
    return true;
}

// The header step on the first n bytes of the frame.  CHIP_FINISHED: the cursor is filled and stands at the first block;
// CHIP_NEED_INPUT: the header is not whole, nothing changed; negative: the batch decode's code for this header, made sticky.
int32_t header_step(chip_zstd_cursor &cur, const uint8_t *in, uint64_t n, int wlog_max, uint32_t flags, uint32_t &header_bytes, uint64_t &need_state)
{
    const auto fail = [&](int32_t code) {
        cur.phase = CHIP_ZCUR_ERROR;
        cur.error = -code;
        return -code;
    };
    header_bytes = 0;
    need_state = 0;
    if (n < 4) return CHIP_NEED_INPUT;
    if ((uint32_t)le_field(in, 4) != ZSTD_FRAME_MAGIC) return fail(ZSTD_E_PREFIX_UNKNOWN);
    if (n < 5) return CHIP_NEED_INPUT;
    const uint32_t fhd = in[4], f = fhd >> 6, ss = (fhd >> 5) & 1u, d = fhd & 3u;
    const uint32_t did_bytes = d == 3 ? 4u : d, fcs_bytes = f == 0 ? ss : 1u << f, did_at = 5u + (ss ? 0u : 1u), fcs_at = did_at + did_bytes;
    const uint32_t hs = fcs_at + fcs_bytes;
    if (n < hs) return CHIP_NEED_INPUT;
    if (fhd & 8u) return fail(ZSTD_E_FRAMEPARAM_UNSUPPORTED);
    uint64_t fcs = CHIP_ZBLOCKS_UNSIZED, window;
    if (fcs_bytes) fcs = le_field(in + fcs_at, fcs_bytes) + (fcs_bytes == 2 ? 256u : 0u);
    if (ss) {
        window = fcs;
    } else {
        const uint32_t wd = in[5], wl = 10u + (wd >> 3);
        if (wl > 31) return fail(ZSTD_E_WINDOW_TOO_LARGE);
        window = (1ull << wl) + ((1ull << wl) >> 3) * (wd & 7u);
    }
    if (window > (1ull << (wlog_max ? wlog_max : 27))) return fail(ZSTD_E_WINDOW_TOO_LARGE);
    if (le_field(in + did_at, did_bytes) != 0) return fail(ZSTD_E_DICT_WRONG);
    cur = chip_zstd_cursor{};
    cur.in_total = hs;
    cur.window_size = window;
    cur.content_size = fcs;
    cur.rep[0] = 1;
    cur.rep[1] = 4;
    cur.rep[2] = 8;
    cur.phase = CHIP_ZCUR_BLOCKS;
    cur.descriptor = fhd;
    cur.waived = (flags & CHIP_ZPAR_NO_CHECKSUM) ? 1u : 0u;
    header_bytes = hs;
    need_state = (uint64_t)CHIP_ZCUR_CARRY_BYTES + window;
    return CHIP_FINISHED;
}

void xxh_update_host(chip_xxh64_state &st, const uint8_t *p, uint64_t n)
{
    zenc::Xxh &x = reinterpret_cast<zenc::Xxh &>(st);
    if (st.total == 0) zenc::xxh_init(x);
    while (n) {
        const uint32_t k = n < (1u << 30) ? (uint32_t)n : 1u << 30;
        zenc::xxh_update(x, p, k);
        p += k;
        n -= k;
    }
}

uint64_t xxh_digest_host(const chip_xxh64_state &st)
{
    zenc::Xxh x;
    memcpy(&x, &st, sizeof x);
    if (st.total == 0) zenc::xxh_init(x);
    return zenc::xxh_digest(x);
}

struct ZnextCall {
    chip_zstd_cursor *cur;
    uint8_t *state;
    uint64_t state_cap;
    const uint8_t *in;
    uint64_t len;
    uint8_t *out;
    uint64_t out_cap;
    int wlog_max;
    uint32_t flags;
};

// One call.  The caller's cursor is written once, at the end of a call that did not fail in the runtime.
hipError_t znext_locked(ZparSlot &sl, const ZnextCall &c, chip_zstd_next_summary &o, hipStream_t s)
{
    ZparClock clock(s);
    chip_zstd_cursor cur = *c.cur;
    const auto leave = [&](int32_t status) {
        o.status = status;
        if (status < 0) {
            cur.phase = CHIP_ZCUR_ERROR;
            cur.error = status;
        }
        *c.cur = cur;
        return hipSuccess;
    };
    if (cur.phase == CHIP_ZCUR_ERROR) return leave(cur.error);
    if (cur.phase == CHIP_ZCUR_DONE) return leave(CHIP_FINISHED);
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    uint64_t q = 0;  // bytes of the slab in front of the cursor
    if (cur.phase == CHIP_ZCUR_HEADER) {
        uint8_t head[18] = {0};
        const uint64_t hn = c.len < sizeof head ? c.len : sizeof head;
        if (hn && (e = hipMemcpyAsync(head, c.in, hn, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        uint32_t hb = 0;
        uint64_t need = 0;
        const int32_t rc = header_step(cur, head, hn, c.wlog_max, c.flags, hb, need);
        if (rc == CHIP_NEED_INPUT) return leave(CHIP_NEED_INPUT);
        if (rc < 0) return leave(rc);
        q = o.in_used = hb;
    }
    const uint64_t window = cur.window_size;
    if (cur.phase == CHIP_ZCUR_BLOCKS && c.state_cap < (uint64_t)CHIP_ZCUR_CARRY_BYTES + window) {  // (the checksum phase reads no state)
        o.need_state = (uint64_t)CHIP_ZCUR_CARRY_BYTES + window;
        return leave(CHIP_NEED_OUTPUT);
    }
    uint8_t *const ring = c.state + CHIP_ZCUR_CARRY_BYTES;
    const bool compare = (cur.descriptor & 4u) != 0 && !cur.waived;
    bool room_cut = false;
    if (cur.phase == CHIP_ZCUR_BLOCKS) {
        const uint8_t *const in = c.in + q;
        const uint64_t len = c.len - q, bmax = window < BLOCK_MAX_BYTES ? window : BLOCK_MAX_BYTES;
        // 1. the walk from the cursor
        if ((e = grow_buffer(sl.blk, sl.blk_cap, (size_t)16384 * sizeof(chip_zstd_block))) != hipSuccess) return e;
        chip_zstd_slab_summary ws;
        uint64_t cap;
        for (;;) {  // (more blocks than records: the walk runs again with four times the records, up to the limit of a call)
            cap = sl.blk_cap / sizeof(chip_zstd_block) < CHIP_ZPLAN_MAX_BLOCKS ? sl.blk_cap / sizeof(chip_zstd_block) : CHIP_ZPLAN_MAX_BLOCKS;
            hipLaunchKernelGGL(zslab_hop_kernel, dim3(1), dim3(64), 0, s, in, len, bmax, cap, (chip_zstd_block *)sl.blk, &sl.d_sum->slab);
            if ((e = sl.fetch(s)) != hipSuccess) return e;
            ws = sl.h_sum->slab;
            if (ws.status != CHIP_ZPLAN_TOO_LARGE || cap >= CHIP_ZPLAN_MAX_BLOCKS) break;
            if ((e = grow_buffer(sl.blk, sl.blk_cap, sl.blk_cap * 4)) != hipSuccess) return e;
        }
        const uint32_t n = (uint32_t)(ws.n_blocks < cap ? ws.n_blocks : cap);
        int32_t tail_err = ws.status == CHIP_ZPLAN_BAD_HEADER ? -ZSTD_E_CORRUPTION : 0;  // the verdict on block n, once the blocks in front are out
        chip_zstd_block *const d_rec = (chip_zstd_block *)sl.blk;
        if (n == 0) {
            if (tail_err) return leave(tail_err);
            return leave(CHIP_NEED_INPUT);
        }
        hipLaunchKernelGGL(zblocks_describe_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, in, d_rec, n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // the carried definers, in the order of the frame, in front of the slab's blocks
        uint32_t nc = 0, slot_of[4];
        for (uint32_t k = 0; k < 4; k++) {
            if (!cur.carry_len[k]) continue;
            uint32_t j = 0;
            while (j < nc && cur.carry_at[slot_of[j]] != cur.carry_at[k]) j++;
            if (j == nc) slot_of[nc++] = k;
        }
        for (uint32_t a = 1; a < nc; a++)
            for (uint32_t b = a; b > 0 && cur.carry_at[slot_of[b]] < cur.carry_at[slot_of[b - 1]]; b--) std::swap(slot_of[b], slot_of[b - 1]);
        std::vector<chip_zstd_block> recs((size_t)nc + n);
        for (uint32_t j = 0; j < nc; j++) {  // replay-only: its offset is all the token pass reads; a raw block of no bytes to every other pass
            chip_zstd_block b{};
            b.offset = (uint64_t)slot_of[j] * CHIP_ZCUR_SLOT_BYTES;
            for (uint32_t k = 0; k < 4; k++) b.src[k] = -1;
            recs[j] = b;
        }
        if ((e = hipMemcpyAsync(recs.data() + nc, d_rec, (size_t)n * sizeof(chip_zstd_block), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        clock.mark("walk");
        int32_t last[4] = {-1, -1, -1, -1};
        for (uint32_t k = 0; k < 4; k++)
            for (uint32_t j = 0; j < nc; j++)
                if (cur.carry_len[k] && cur.carry_at[slot_of[j]] == cur.carry_at[k]) last[k] = (int32_t)j;
        // what the token pass needs of every block, and where the call stops taking blocks
        std::vector<uint32_t> seq_base((size_t)nc + n, 0), span_len((size_t)nc + n, 0);
        std::vector<uint64_t> slot_off((size_t)nc + n, 0), unit_off((size_t)nc + n, 0);
        uint64_t n_seq = 0, slot_total = 0;
        uint32_t run = 0;  // blocks of the slab the token pass takes
        for (; run < n; run++) {
            chip_zstd_block &b = recs[(size_t)nc + run];
            const uint32_t i = nc + run;
            b.offset += CHIP_ZCUR_CARRY_BYTES;  // (where the block lies in the staged input)
            for (uint32_t k = 0; k < 4; k++) b.src[k] = last[k];
            if ((b.flags & CHIP_ZBLOCK_MALFORMED) || b.lit_regen > BLOCK_MAX_BYTES) {
                tail_err = -ZSTD_E_CORRUPTION;
                break;
            }
            if (b.type == 2 && b.lit_type == 3 && last[0] < 0) {  // (the batch decode's code for a treeless block without a table)
                tail_err = -30;
                break;
            }
            uint64_t first = b.offset;
            if (b.type == 2)
                for (uint32_t k = 0; k < 4; k++)
                    if ((k == 0 ? b.lit_type == 3 : (b.n_seq != 0 && b.mode[k - 1] == 3)) && b.src[k] >= 0 && recs[b.src[k]].offset < first) first = recs[b.src[k]].offset;
            first &= ~(uint64_t)3;
            const uint64_t span = b.offset + 3 + (b.type == 1 ? 1u : b.size) - first;
            if (span > ((uint64_t)1 << 28) || n_seq + b.n_seq > ((uint64_t)1 << 30)) {  // (never the first block: the next call has the definer in its carry)
                tail_err = 0;
                break;
            }
            unit_off[i] = first;
            span_len[i] = (uint32_t)span;
            seq_base[i] = (uint32_t)n_seq;
            slot_off[i] = slot_total;
            n_seq += b.n_seq;
            if (b.type == 2 && b.lit_type >= 2) slot_total += up16((size_t)b.lit_regen + ZTOK_SLOT_SLACK);
            for (uint32_t k = 0; k < 4; k++)
                if (defines(b, k)) last[k] = (int32_t)i;
        }
        if (run == n && ws.status != CHIP_ZPLAN_BAD_HEADER) tail_err = 0;
        if (run == 0) return leave(tail_err ? tail_err : CHIP_NEED_INPUT);
        const uint32_t nj = nc + run;
        const uint64_t run_bytes = recs[nj - 1].offset - CHIP_ZCUR_CARRY_BYTES + 3 + (recs[nj - 1].type == 1 ? 1u : recs[nj - 1].size);
        size_t off = 0;
        auto take = [&](size_t bytes) {
            const size_t at = off;
            off += up16(bytes);
            return at;
        };
        const size_t o_stage = take((size_t)CHIP_ZCUR_CARRY_BYTES + run_bytes + 16), o_blocks = take((size_t)nj * sizeof(chip_zstd_block)),
                     o_in_off = take((size_t)nj * 8), o_out_off = take((size_t)nj * 8), o_in_len = take((size_t)nj * 4), o_out_cap = take((size_t)nj * 4),
                     o_seq = take((size_t)nj * 4), o_up_end = off, o_out_len = take((size_t)nj * 4), o_in_used = take((size_t)nj * 4),
                     o_status = take((size_t)nj * 4), o_res = take((size_t)nj * 32), o_pos = take((size_t)nj * 4), o_rep = take((size_t)nj * 12),
                     o_tok = take((size_t)n_seq * 12 + 16), o_slots = take((size_t)slot_total + 16);
        if ((e = sl.grow(0, off)) != hipSuccess) return e;
        uint8_t *const base = sl.buf[0], *const stage = base + o_stage;
        {
            std::vector<uint8_t> up(o_up_end - o_blocks, 0);
            const auto at = [&](size_t o_what) { return up.data() + (o_what - o_blocks); };
            memcpy(at(o_blocks), recs.data(), (size_t)nj * sizeof(chip_zstd_block));
            for (uint32_t i = 0; i < nj; i++) {
                const chip_zstd_block &b = recs[i];
                ((uint64_t *)at(o_out_off))[i] = slot_off[i];
                ((uint64_t *)at(o_in_off))[i] = unit_off[i];
                ((uint32_t *)at(o_in_len))[i] = span_len[i];
                ((uint32_t *)at(o_out_cap))[i] = i >= nc && b.type == 2 && b.lit_type >= 2 ? (uint32_t)up16((size_t)b.lit_regen + ZTOK_SLOT_SLACK) : 0u;
                ((uint32_t *)at(o_seq))[i] = seq_base[i];
            }
            if ((e = hipMemcpyAsync(base + o_blocks, up.data(), up.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
            if (nc && (e = hipMemcpyAsync(stage, c.state, CHIP_ZCUR_CARRY_BYTES, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(stage + CHIP_ZCUR_CARRY_BYTES, in, run_bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;  // (the staging vector goes away)
        }
        // 2. tokens
        BatchArgs a{};
        a.in_base = stage;
        a.in_off = (const uint64_t *)(base + o_in_off);
        a.in_len = (const uint32_t *)(base + o_in_len);
        a.out_base = base + o_slots;
        a.out_off = (const uint64_t *)(base + o_out_off);
        a.out_cap = (const uint32_t *)(base + o_out_cap);
        a.out_len = (uint32_t *)(base + o_out_len);
        a.in_used = (uint32_t *)(base + o_in_used);
        a.status = (int32_t *)(base + o_status);
        a.n = nj;
        a.format = CHIP_FMT_ZSTD;
        const ZTokArgs tk{(const chip_zstd_block *)(base + o_blocks), (const uint32_t *)(base + o_seq), (uint32_t *)(base + o_tok), (uint32_t *)(base + o_res), window};
        if ((e = launch_zstd_tokens(a, tk, s)) != hipSuccess) return e;
        std::vector<uint32_t> out_len(nj), res((size_t)nj * 8);
        std::vector<int32_t> status(nj);
        if ((e = hipMemcpyAsync(out_len.data(), base + o_out_len, (size_t)nj * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(status.data(), base + o_status, (size_t)nj * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(res.data(), base + o_res, (size_t)nj * 32, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        clock.mark("tokens");
        // 3. compose: the leading blocks that are clean and fit the room
        std::vector<uint32_t> pos(nj, 0), rep_in((size_t)nj * 3, 1);
        std::vector<uint32_t> rep_after((size_t)nj * 3, 1);
        uint64_t total = 0, need_out = 0;
        uint32_t rep[3] = {cur.rep[0], cur.rep[1], cur.rep[2]}, taken = nc;  // joint index behind the last block taken
        int32_t err = 0;
        for (; taken < nj; taken++) {
            const uint32_t i = taken;
            if (status[i] != CHIP_FINISHED) err = status[i] < 0 ? status[i] : -ZSTD_E_CORRUPTION;
            else if (out_len[i] > bmax) err = -ZSTD_E_CORRUPTION;
            else if (cur.content_size != CHIP_ZBLOCKS_UNSIZED && cur.out_total + total + out_len[i] > cur.content_size) err = -ZSTD_E_CORRUPTION;
            else if ((recs[i].flags & CHIP_ZBLOCK_LAST) && cur.content_size != CHIP_ZBLOCKS_UNSIZED && cur.out_total + total + out_len[i] != cur.content_size)
                err = -ZSTD_E_CORRUPTION;
            if (err) break;
            if (total + out_len[i] > c.out_cap) {
                room_cut = true;
                need_out = out_len[i];
                break;
            }
            pos[i] = (uint32_t)total;
            total += out_len[i];
            for (uint32_t k = 0; k < 3; k++) rep_in[3 * (size_t)i + k] = rep[k];
            if (recs[i].type == 2) {
                const uint32_t nr[3] = {sym_value(res[8 * (size_t)i], rep), sym_value(res[8 * (size_t)i + 1], rep), sym_value(res[8 * (size_t)i + 2], rep)};
                rep[0] = nr[0];
                rep[1] = nr[1];
                rep[2] = nr[2];
            }
            for (uint32_t k = 0; k < 3; k++) rep_after[3 * (size_t)i + k] = rep[k];
        }
        if (!err && !room_cut && taken == nj) err = tail_err;
        uint32_t rounds = 0;
        if (taken > nc) {
            if ((e = hipMemcpyAsync(base + o_pos, pos.data(), (size_t)nj * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(base + o_rep, rep_in.data(), (size_t)nj * 12, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
            if ((e = sl.grow(1, up16(((size_t)total + 4) * 4))) != hipSuccess) return e;
            uint32_t *const W = (uint32_t *)sl.buf[1];
            // 4. place, with the window in front of position 0
            if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(ZparDev), s)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(&sl.d_sum->bad, 0xFF, 4, s)) != hipSuccess) return e;
            hipLaunchKernelGGL(zpar_place_kernel<true>, dim3(taken), dim3(64), 0, s, (const uint8_t *)stage, tk.blocks, (const uint32_t *)(base + o_pos),
                               (const uint32_t *)a.out_len, tk.seq_base, (const uint32_t *)tk.tok, (const uint32_t *)tk.res, (const uint32_t *)(base + o_rep),
                               a.in_off, (const uint8_t *)a.out_base, a.out_off, window, W, sl.d_sum, cur.hist, (const uint8_t *)ring, cur.ring);
            if ((e = sl.fetch(s)) != hipSuccess) return e;  // (pos and rep_in have left the host by now)
            clock.mark("place");
            if (sl.h_sum->bad != NO_BAD) {  // the blocks in front of the first bad one are whole and checked
                if (sl.h_sum->bad < nc || sl.h_sum->bad >= taken) return hipErrorUnknown;
                taken = sl.h_sum->bad;
                total = pos[taken];
                err = -ZSTD_E_CORRUPTION;
                room_cut = false;
            }
        }
        if (taken > nc) {
            uint32_t *const W = (uint32_t *)sl.buf[1];
            // 5. jump
            const uint32_t n_words = (uint32_t)total, grid = (uint32_t)((total + 1023) / 1024);
            uint32_t left = n_words ? 1u : 0u;
            while (left && rounds < CHIP_ZPAR_ROUNDS_MAX) {
                if ((e = hipMemsetAsync(&sl.d_sum->left, 0, 4, s)) != hipSuccess) return e;
                hipLaunchKernelGGL(zpar_jump_kernel, dim3(grid), dim3(256), 0, s, W, n_words, sl.d_sum);
                if ((e = sl.fetch(s)) != hipSuccess) return e;
                left = sl.h_sum->left;
                rounds++;
                clock.mark("jump", left);
            }
            if (left) return hipErrorUnknown;  // (cannot happen below 2^31 bytes: the reach of every pointer at least doubles per round)
            // 6. deliver, checksum, window, carry
            if (n_words) hipLaunchKernelGGL(zpar_deliver_kernel, dim3(grid), dim3(256), 0, s, (const uint32_t *)W, n_words, c.out);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            clock.mark("deliver");
            if (compare && n_words) {
                if ((e = launch_zstd_xxh_update(c.out, n_words, cur.xxh, &sl.d_sum->state, s)) != hipSuccess) return e;
                if ((e = sl.fetch(s)) != hipSuccess) return e;
                cur.xxh = sl.h_sum->state;
                clock.mark("checksum");
            }
            if (n_words && window) {  // the last min(total, window) bytes, in at most two pieces
                const uint64_t m = total < window ? total : window, at = ring_mod(cur.ring + (total - m), window), one = m < window - at ? m : window - at;
                if ((e = hipMemcpyAsync(ring + at, c.out + (total - m), one, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
                if (m > one && (e = hipMemcpyAsync(ring, c.out + (total - m) + one, m - one, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
            }
            int32_t def[4] = {-1, -1, -1, -1};
            for (uint32_t i = nc; i < taken; i++)
                for (uint32_t k = 0; k < 4; k++)
                    if (defines(recs[i], k)) def[k] = (int32_t)i;
            const uint64_t taken_bytes = recs[taken - 1].offset - CHIP_ZCUR_CARRY_BYTES + 3 + (recs[taken - 1].type == 1 ? 1u : recs[taken - 1].size);
            for (uint32_t k = 0; k < 4; k++) {
                if (def[k] < 0) continue;
                const chip_zstd_block &b = recs[def[k]];
                const uint64_t at = b.offset - CHIP_ZCUR_CARRY_BYTES;
                if ((e = hipMemcpyAsync(c.state + (size_t)k * CHIP_ZCUR_SLOT_BYTES, in + at, 3 + (size_t)b.size, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
                cur.carry_len[k] = 3 + b.size;
                cur.carry_at[k] = cur.in_total + at;
            }
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            clock.mark("window");
            for (uint32_t k = 0; k < 3; k++) cur.rep[k] = rep_after[3 * (size_t)(taken - 1) + k];
            cur.in_total += taken_bytes;
            cur.out_total += total;
            cur.hist = cur.out_total < window ? cur.out_total : window;
            cur.ring = ring_mod(cur.out_total, window);
            q += taken_bytes;
            o.in_used = q;
            o.out_len = total;
            o.n_blocks = taken - nc;
            o.n_sequences = seq_base[taken - 1] + recs[taken - 1].n_seq;
            o.rounds = rounds;
            if (!err && (recs[taken - 1].flags & CHIP_ZBLOCK_LAST)) cur.phase = CHIP_ZCUR_CHECKSUM;
        }
        if (err) return leave(err);
        if (room_cut) {
            o.need_out = need_out;
            return leave(CHIP_NEED_OUTPUT);
        }
        if (cur.phase != CHIP_ZCUR_CHECKSUM) return leave(CHIP_NEED_INPUT);
    }
    // the checksum behind the last block
    if (cur.descriptor & 4u) {
        if (c.len - q < 4) return leave(CHIP_NEED_INPUT);
        uint8_t want[4];
        if ((e = hipMemcpyAsync(want, c.in + q, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        q += 4;
        cur.in_total += 4;
        o.in_used = q;
        if (compare && (uint32_t)xxh_digest_host(cur.xxh) != (uint32_t)le_field(want, 4)) return leave(-ZSTD_E_CHECKSUM_WRONG);
    }
    cur.phase = CHIP_ZCUR_DONE;
    return leave(CHIP_FINISHED);
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_zstd_blocks_host(const uint8_t *in, uint64_t len, uint64_t max_blocks, chip_zstd_block *blocks, chip_zstd_blocks_summary *summary)
{
    if (!summary || (len && !in) || (max_blocks && !blocks)) return CHIP_E_INVALID;
    *summary = walk_blocks(in, len, max_blocks, blocks);
    const uint64_t n = summary->n_blocks < max_blocks ? summary->n_blocks : max_blocks;
    int32_t last[4] = {-1, -1, -1, -1};
    for (uint64_t i = 0; i < n; i++) {
        describe_block(in, blocks[i]);
        for (uint32_t k = 0; k < 4; k++) {
            blocks[i].src[k] = last[k];
            if (defines(blocks[i], k)) last[k] = (int32_t)i;
        }
    }
    return CHIP_OK;
}

int chip_zstd_blocks(const void *in_base, uint64_t len, uint64_t max_blocks, chip_zstd_block *blocks, chip_zstd_blocks_summary *summary,
                     void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_blocks && !blocks) || ((uintptr_t)in_base & 3u) || len > ((uint64_t)1 << 40)) return CHIP_E_INVALID;
    *summary = NO_FRAME;
    if (len < 4) return CHIP_OK;  // (what the walk says of it)
    return with_slot(
        g_zblocks_cache, stream,
        [&](ZblocksSlot &sl, hipStream_t s) {
            hipError_t e = sl.summary();
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(zblocks_hop_kernel, dim3(1), dim3(64), 0, s, (const uint8_t *)in_base, len, max_blocks, blocks, sl.d_sum);
            if ((e = sl.fetch(s)) != hipSuccess) return e;
            const chip_zstd_blocks_summary r = *sl.h_sum;
            const uint32_t n = (uint32_t)(r.n_blocks < max_blocks ? r.n_blocks : max_blocks);  // (at most CHIP_ZPLAN_MAX_BLOCKS)
            if (n) {
                hipLaunchKernelGGL(zblocks_describe_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, (const uint8_t *)in_base, blocks, n);
                hipLaunchKernelGGL(zblocks_sources_kernel, dim3(1), dim3(SRC_THREADS), 0, s, blocks, n);
                if ((e = hipGetLastError()) != hipSuccess) return e;
                if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            }
            *summary = r;
            return hipSuccess;
        },
        [&] { *summary = NO_FRAME; });
}

int chip_zstd_parallel(const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, int window_log_max, uint32_t flags,
                       chip_zstd_parallel_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (out_cap && !out_base) || ((uintptr_t)in_base & 3u) || (flags & ~CHIP_ZPAR_NO_CHECKSUM) || len > 0xFFFFFFFFull ||
        window_log_max < 0)
        return CHIP_E_INVALID;
    const auto blank = [&] { *summary = chip_zstd_parallel_summary{0, 0, 0, 0, 0, 0, CHIP_ZPAR_SERIAL, 0, 0}; };
    blank();
    const ZparCall c{(const uint8_t *)in_base, len, (uint8_t *)out_base, out_cap, window_log_max, flags, summary};
    return with_slot(
        g_zpar_cache, stream,
        [&](ZparSlot &sl, hipStream_t s) {
            bool serial = true;
            uint64_t unit_len = c.len;
            hipError_t e = zpar_parallel(sl, c, s, serial, unit_len);
            if (e == hipSuccess && serial) e = zpar_serial(sl, c, unit_len, s);
            return e;
        },
        blank);
}

int chip_zstd_slab_blocks_host(const uint8_t *in, uint64_t len, uint64_t block_max, uint64_t max_blocks, chip_zstd_block *blocks,
                               chip_zstd_slab_summary *summary)
{
    if (!summary || (len && !in) || (max_blocks && !blocks)) return CHIP_E_INVALID;
    *summary = walk_slab(in, len, block_max, max_blocks, CHIP_ZPLAN_MAX_BLOCKS, blocks);
    const uint64_t n = summary->n_blocks < max_blocks ? summary->n_blocks : max_blocks;
    int32_t last[4] = {-1, -1, -1, -1};
    for (uint64_t i = 0; i < n; i++) {
        describe_block(in, blocks[i]);
        for (uint32_t k = 0; k < 4; k++) {
            blocks[i].src[k] = last[k];
            if (defines(blocks[i], k)) last[k] = (int32_t)i;
        }
    }
    return CHIP_OK;
}

int chip_zstd_cursor_header_host(chip_zstd_cursor *cur, const uint8_t *in, uint64_t len, int window_log_max, uint32_t flags, uint32_t *header_bytes,
                                 uint64_t *need_state)
{
    if (!cur || (len && !in) || !header_bytes || !need_state || (flags & ~CHIP_ZPAR_NO_CHECKSUM) || window_log_max < 0 || window_log_max > 31) return CHIP_E_INVALID;
    if (cur->phase != CHIP_ZCUR_HEADER || !cursor_ok(*cur)) return CHIP_E_INVALID;
    return header_step(*cur, in, len, window_log_max, flags, *header_bytes, *need_state);
}

int chip_xxh64_update_host(chip_xxh64_state *st, const uint8_t *data, uint64_t len)
{
    if (!st || (len && !data) || st->tail_n > 31) return CHIP_E_INVALID;
    xxh_update_host(*st, data, len);
    return CHIP_OK;
}

uint64_t chip_xxh64_digest_host(const chip_xxh64_state *st) { return st && st->tail_n <= 31 ? xxh_digest_host(*st) : 0; }

int chip_zstd_parallel_next(chip_zstd_cursor *cur, void *state, uint64_t state_cap, const void *in_base, uint64_t len, void *out_base, uint64_t out_cap,
                            int window_log_max, uint32_t flags, chip_zstd_next_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || !cur || !state || (!in_base && len) || (!out_base && out_cap) || len > ((uint64_t)1 << 31) || out_cap >= ((uint64_t)1 << 31) ||
        (flags & ~CHIP_ZPAR_NO_CHECKSUM) || window_log_max < 0 || window_log_max > 31)
        return CHIP_E_INVALID;
    if (!cursor_ok(*cur)) return CHIP_E_INVALID;
    if ((cur->phase == CHIP_ZCUR_BLOCKS || cur->phase == CHIP_ZCUR_CHECKSUM) && cur->waived != (flags & CHIP_ZPAR_NO_CHECKSUM)) return CHIP_E_INVALID;
    const chip_zstd_next_summary none{0, 0, 0, 0, 0, 0, CHIP_NEED_INPUT, 0};
    *summary = none;
    const chip_zstd_cursor before = *cur;
    const ZnextCall c{cur, (uint8_t *)state, state_cap, (const uint8_t *)in_base, len, (uint8_t *)out_base, out_cap, window_log_max, flags};
    // (the caller's device stays current: with_slot looks up the slot of the current device and changes none)
    return with_slot(
        g_zpar_cache, stream, [&](ZparSlot &sl, hipStream_t s) { return znext_locked(sl, c, *summary, s); },
        [&] {
            *summary = none;
            *cur = before;  // (the state may hold a later call's bytes: a failed call ends the decode)
        });
}

}  // extern "C"
