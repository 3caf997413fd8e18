// BGZF (the blocked gzip of BAM / BCF / bgzip): the block index of a buffer, on the host (chip_bgzf_plan_host) and on the GPU
// (chip_bgzf_plan), and htslib's EOF marker.  DESIGN.md sec. 4.10.
//
// The plan of a buffer is DEFINED by the serial walk of include/compu_hip.h (chip_bgzf_plan_host below is that walk; describe_block
// is its per-block part, shared by the host walk and the kernel).  The GPU version gives the same answer without chasing BSIZE
// through HBM one block after the other: it is the plan pipeline of plan_common.h ("The container plan") with the format below.
//   candidates  every byte position is tested for the gzip magic with FEXTRA (`1f 8b 08 04`) in 16-byte loads, the rare hits for the
//               other fixed header bytes
//   describe    BSIZE and ISIZE of a candidate: end = position + BSIZE + 1, cap = ISIZE, the verdict (block too short / runs past
//               the end / ISIZE too large).  Every block is a unit of the batch: there is nothing to step over
// What the marking never reaches is a decoy: valid compressed data may hold the header bytes, e.g. inside a stored block.
#include "chip_internal.h"
#include "launch_slots.h"
#include "plan_common.h"

namespace chip {

namespace {

constexpr uint32_t BGZF_HDR = 18;               // bytes of the header this library accepts (XLEN 6: the BC subfield alone)
constexpr uint32_t BGZF_MIN = 28;               // header + empty deflate body (2) + CRC-32 + ISIZE
constexpr uint32_t BGZF_MAGIC = 0x04088b1fu;    // 1f 8b 08 04, little endian

__host__ __device__ __forceinline__ uint32_t le32(const uint8_t *b)
{
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

// room for a header at p in front of `len`
__host__ __device__ __forceinline__ bool header_fits(uint64_t len, uint64_t p) { return len >= BGZF_HDR && p <= len - BGZF_HDR; }

// the fixed header bytes behind the magic: XLEN 6, `B C 02 00`
__host__ __device__ __forceinline__ bool header_rest(const uint8_t *h)
{
    return h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0;
}

__host__ __device__ __forceinline__ bool is_header(const uint8_t *h) { return le32(h) == BGZF_MAGIC && header_rest(h); }

// The per-block part of the walk for the block whose header sits at p (p + 18 <= len).  Reads bytes of [p, len) only.
__host__ __device__ __forceinline__ Described describe_block(const uint8_t *in, uint64_t len, uint64_t p)
{
    Described r{0, 0, 0, KIND_FRAME};
    const uint32_t bs = ((uint32_t)in[p + 16] | ((uint32_t)in[p + 17] << 8)) + 1u;
    if (bs < BGZF_MIN) return r.verdict = CHIP_BGZF_BAD_HEADER, r;
    if (bs > len - p) return r.verdict = CHIP_BGZF_TRUNCATED, r;
    const uint32_t isize = le32(in + p + bs - 4);
    if (isize > 65536u) return r.verdict = CHIP_BGZF_BAD_HEADER, r;
    r.end = p + bs;
    r.cap = isize;
    return r;
}

struct BgzfFormat {
    static constexpr uint32_t MIN_HEADER = BGZF_HDR;

    // bit k: the four bytes at offset k of the chunk are the magic
    static __device__ __forceinline__ uint32_t magic_mask(const uint32_t w[5])
    {
        uint32_t m = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) m |= (chunk_word(w, k) == BGZF_MAGIC ? 1u : 0u) << k;
        return m;
    }

    // candidates of chunk g as a 16-bit mask: the magic, then the rare hits are tested for a whole header in front of `len`
    static __device__ __forceinline__ uint32_t candidates(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t g)
    {
        if (g >= n_chunks) return 0;
        uint32_t w[5];
        load_chunk(base, (len + 3) & ~(uint64_t)3, g, w);
        uint32_t m = magic_mask(w), keep = 0;
        while (m) {
            const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            const uint64_t p = g * 16 + k;
            if (header_fits(len, p) && header_rest(base + p)) keep |= 1u << k;
        }
        return keep;
    }

    static __device__ __forceinline__ Described describe(const uint8_t *base, uint64_t len, uint64_t p, bool &gone)
    {
        gone = !header_fits(len, p) || !is_header(base + p);
        return gone ? Described{} : describe_block(base, len, p);
    }
};

SlotCache<SummarySlot<PlanSummary>> g_bgzf_cache;

const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

const uint8_t *chip_bgzf_eof_block(size_t *len)
{
    if (len) *len = sizeof(EOF_BLOCK);
    return EOF_BLOCK;
}

int chip_bgzf_plan_host(const uint8_t *in, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                        uint32_t *out_cap, chip_bgzf_summary *summary)
{
    if (!summary || (len && !in) || (max_blocks && (!in_off || !in_len || !out_off || !out_cap))) return CHIP_E_INVALID;
    uint64_t p = 0, n = 0, total = 0;
    uint32_t last_isize = 1;
    int32_t status = CHIP_BGZF_OK;
    while (p != len) {
        if (!header_fits(len, p) || !is_header(in + p)) {
            status = stop_status<BgzfFormat>(len, p);
            break;
        }
        const Described r = describe_block(in, len, p);
        if (r.verdict) {
            status = (int32_t)r.verdict;
            break;
        }
        if (n < max_blocks) {
            in_off[n] = p;
            in_len[n] = (uint32_t)(r.end - p);
            out_off[n] = total;
            out_cap[n] = r.cap;
        }
        last_isize = r.cap;
        n++;
        total += r.cap;
        p = r.end;
    }
    summary->n_blocks = n;
    summary->total_out = total;
    summary->in_used = p;
    summary->status = status;
    summary->eof = n && last_isize == 0 ? 1u : 0u;
    return CHIP_OK;
}

int chip_bgzf_plan(const void *in_base, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                   uint32_t *out_cap, chip_bgzf_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_blocks && (!in_off || !in_len || !out_off || !out_cap)) || ((uintptr_t)in_base & 3u) ||
        len > ((uint64_t)1 << 40))
        return CHIP_E_INVALID;
    *summary = chip_bgzf_summary{0, 0, 0, CHIP_BGZF_OK, 0};
    if (len == 0) return CHIP_OK;
    PlanSummary r{};
    bool too_many = false;
    const int rc = with_slot(
        g_bgzf_cache, stream,
        [&](SummarySlot<PlanSummary> &sl, hipStream_t s) {
            return plan_locked<BgzfFormat>(sl, (const uint8_t *)in_base, len, max_blocks, in_off, in_len, out_off, out_cap, s, r, too_many);
        },
        [&] { *summary = chip_bgzf_summary{0, 0, 0, CHIP_BGZF_BAD_HEADER, 0}; });
    if (rc != CHIP_OK) return rc;
    if (too_many) return CHIP_E_NOMEM;
    // eof: the last block of the walk has ISIZE 0
    *summary = chip_bgzf_summary{r.sum.frames, r.sum.bytes, r.in_used, r.status, r.sum.frames && r.last_cap == 0 ? 1u : 0u};
    return CHIP_OK;
}

}  // extern "C"
