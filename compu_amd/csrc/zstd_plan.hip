// The frame index of a buffer of zstd frames (pzstd output, the seekable format, one frame per chunk, `cat a.zst b.zst`): on the
// host (chip_zstd_plan_host) and on the GPU (chip_zstd_plan), and chip_layout_units, the device step from a size pass to a
// decode.  DESIGN.md sec. 4.12.
//
// The plan of a buffer is DEFINED by the serial walk of include/compu_hip.h (walk_frame below is its per-frame part, shared by
// the host walk and the kernel).  The GPU version is the plan pipeline of plan_common.h ("The container plan") with the format below.
//   candidates  every byte position is tested in 16-byte loads for the frame magic (`28 b5 2f fd`) and the skippable range
//               (`5x 2a 4d 18`)
//   describe    walk_frame: the frame header, then one 3-byte block header per block (a skippable frame: one size field); the end
//               position, the verdict, Frame_Content_Size and the kind.  Skippable frames are stepped over and counted
// What the marking never reaches is a decoy: magic bytes inside block data, or a whole frame embedded in a raw block.  No byte
// outside [0, len4) is loaded and none outside [0, len) decides anything.
#include "chip_internal.h"
#include "launch_slots.h"
#include "plan_common.h"

namespace chip {

namespace {

constexpr uint32_t ZSTD_MAGIC = 0xFD2FB528u, SKIP_MAGIC = 0x184D2A50u;  // the skippable range: SKIP_MAGIC | 0..15

__host__ __device__ __forceinline__ uint64_t le_bytes(const uint8_t *b, uint32_t n)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < n; k++) v |= (uint64_t)b[k] << (8 * k);
    return v;
}

// The per-frame part of the walk for the frame or skippable frame whose magic sits at p (p + 4 <= len, m = LE32(p) is one of the
// two kinds).  Reads bytes of [p, len) only.
__host__ __device__ __forceinline__ Described walk_frame(const uint8_t *in, uint64_t len, uint64_t p, uint32_t m)
{
    Described r{0, 0, 0, KIND_FRAME};
    const uint64_t room = len - p;
    if (m != ZSTD_MAGIC) {
        r.kind = KIND_SKIP;
        if (room < 8) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        const uint64_t s = le_bytes(in + p + 4, 4);
        if (s > room - 8) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        r.end = p + 8 + s;
        return r;
    }
    if (room < 5) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
    const uint32_t fhd = in[p + 4], f = fhd >> 6, ss = (fhd >> 5) & 1u, d = fhd & 3u;
    const uint32_t did_bytes = d == 3 ? 4u : d, fcs_bytes = f == 0 ? ss : 1u << f, fcs_at = 5u + (ss ? 0u : 1u) + did_bytes;
    const uint32_t hs = fcs_at + fcs_bytes;
    if (room < hs) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
    const bool sized = fcs_bytes != 0;
    const uint64_t fcs = sized ? le_bytes(in + p + fcs_at, fcs_bytes) + (fcs_bytes == 2 ? 256u : 0u) : 0;
    uint64_t q = p + hs;
    for (uint32_t blocks = 0;;) {
        if (len - q < 3) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        const uint32_t h = (uint32_t)le_bytes(in + q, 3), type = (h >> 1) & 3u;
        if (type == 3) return r.verdict = CHIP_ZPLAN_BAD_HEADER, r;
        if (++blocks > CHIP_ZPLAN_MAX_BLOCKS) return r.verdict = CHIP_ZPLAN_TOO_LARGE, r;
        const uint64_t body = type == 1 ? 1u : h >> 3;
        if (body > len - q - 3) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        q += 3 + body;
        if (h & 1u) break;
    }
    if (fhd & 4u) {
        if (len - q < 4) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        q += 4;
    }
    if (q - p > 0xFFFFFFFFull || (sized && fcs >= 0xFFFFFFFFull)) return r.verdict = CHIP_ZPLAN_TOO_LARGE, r;
    r.end = q;
    r.cap = sized ? (uint32_t)fcs : CHIP_ZPLAN_UNSIZED;
    return r;
}

__host__ __device__ __forceinline__ bool is_magic(uint32_t m) { return m == ZSTD_MAGIC || (m & 0xFFFFFFF0u) == SKIP_MAGIC; }

struct ZstdFormat {
    static constexpr uint32_t MIN_HEADER = 4;

    // candidates of chunk g as a 16-bit mask: the positions whose four bytes, all in front of `len`, are one of the magics
    static __device__ __forceinline__ uint32_t candidates(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t g)
    {
        if (g >= n_chunks) return 0;
        uint32_t w[5];
        load_chunk(base, (len + 3) & ~(uint64_t)3, g, w);
        uint32_t m = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) m |= (is_magic(chunk_word(w, k)) ? 1u : 0u) << k;
        const uint64_t b = g * 16;
        if (b + 20 > len) {  // (the last two chunks) drop what reaches behind len: the padding up to len4 holds anything
#pragma unroll
            for (uint32_t k = 0; k < 16; k++)
                if (b + k + 4 > len) m &= ~(1u << k);
        }
        return m;
    }

    // a position that no longer holds a magic, or lies out of range, is gone
    static __device__ __forceinline__ Described describe(const uint8_t *base, uint64_t len, uint64_t p, bool &gone)
    {
        const uint32_t m = p < len && len - p >= 4 ? (uint32_t)le_bytes(base + p, 4) : 0u;
        gone = !is_magic(m);
        return gone ? Described{} : walk_frame(base, len, p, m);
    }
};

// the plan's summary, and chip_layout_units' behind it
struct DevSummary : PlanSummary {
    uint64_t layout_total, layout_over;
};

// chip_layout_units behind the two scan kernels: out_off[i] gets its workgroup's offset, out_cap[i] the clipped size
__global__ __launch_bounds__(256) void layout_finish_kernel(const uint64_t *out_size, uint64_t *out_off, uint32_t *out_cap, const uint64_t *part,
                                                            uint64_t n, DevSummary *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = out_size[i];
    out_off[i] += part[i / SCAN_THREADS];
    out_cap[i] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
    if (s > 0xFFFFFFFFull) atomicAdd((unsigned long long *)&ds->layout_over, 1ull);  // (rare: a unit above 4 GiB)
}

// the plan's slot; chip_layout_units uses 8 bytes per 1024 units of its buffer 0
using ZplanSlot = SummarySlot<DevSummary>;
SlotCache<ZplanSlot> g_zplan_cache;

hipError_t layout_locked(ZplanSlot &sl, uint64_t n, const uint64_t *out_size, uint64_t *out_off, uint32_t *out_cap, uint64_t *total,
                         uint64_t *n_over, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    if ((e = sl.grow(0, (size_t)scan_parts(n) * 8)) != hipSuccess) return e;
    uint64_t *part = (uint64_t *)sl.buf[0];
    if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(DevSummary), stream)) != hipSuccess) return e;
    enqueue_scan<uint64_t>(out_size, out_off, n, part, &sl.d_sum->layout_total, stream);
    hipLaunchKernelGGL(layout_finish_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, out_size, out_off, out_cap,
                       (const uint64_t *)part, n, sl.d_sum);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    *total = sl.h_sum->layout_total;
    *n_over = sl.h_sum->layout_over;
    return hipSuccess;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_zstd_plan_host(const uint8_t *in, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                        uint32_t *out_cap, chip_zstd_plan_summary *summary)
{
    if (!summary || (len && !in) || (max_frames && (!in_off || !in_len || !out_off || !out_cap))) return CHIP_E_INVALID;
    uint64_t p = 0, n = 0, skipped = 0, unsized = 0, total = 0;
    int32_t status = CHIP_ZPLAN_OK;
    for (;;) {
        const uint32_t m = len - p >= 4 ? (uint32_t)le_bytes(in + p, 4) : 0u;
        if (len - p < 4 || !is_magic(m)) {
            status = stop_status<ZstdFormat>(len, p);
            break;
        }
        const Described r = walk_frame(in, len, p, m);
        if (r.verdict) {
            status = (int32_t)r.verdict;
            break;
        }
        if (r.kind == KIND_SKIP) {
            skipped++;
        } else {
            const bool sized = r.cap != CHIP_ZPLAN_UNSIZED;
            if (n < max_frames) {
                in_off[n] = p;
                in_len[n] = (uint32_t)(r.end - p);
                out_off[n] = total;
                out_cap[n] = r.cap;
            }
            n++;
            unsized += sized ? 0 : 1;
            total += sized ? r.cap : 0;
        }
        p = r.end;
    }
    *summary = chip_zstd_plan_summary{n, skipped, unsized, total, p, status, 0};
    return CHIP_OK;
}

int chip_zstd_plan(const void *in_base, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                   uint32_t *out_cap, chip_zstd_plan_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_frames && (!in_off || !in_len || !out_off || !out_cap)) || ((uintptr_t)in_base & 3u) ||
        len > ((uint64_t)1 << 40))
        return CHIP_E_INVALID;
    *summary = chip_zstd_plan_summary{0, 0, 0, 0, 0, CHIP_ZPLAN_OK, 0};
    if (len == 0) return CHIP_OK;
    PlanSummary r{};
    bool too_many = false;
    const int rc = with_slot(
        g_zplan_cache, stream,
        [&](ZplanSlot &sl, hipStream_t s) {
            return plan_locked<ZstdFormat>(sl, (const uint8_t *)in_base, len, max_frames, in_off, in_len, out_off, out_cap, s, r, too_many);
        },
        [&] { *summary = chip_zstd_plan_summary{0, 0, 0, 0, 0, CHIP_ZPLAN_BAD_HEADER, 0}; });
    if (rc != CHIP_OK) return rc;
    if (too_many) return CHIP_E_NOMEM;
    *summary = chip_zstd_plan_summary{r.sum.frames, r.sum.skips, r.sum.unsized, r.sum.bytes, r.in_used, r.status, 0};
    return CHIP_OK;
}

int chip_layout_units(size_t n, const uint64_t *out_size, uint64_t *out_off, uint32_t *out_cap, uint64_t *total, uint64_t *n_over, void *stream)
{
    if (!total || !n_over || (n && (!out_size || !out_off || !out_cap || (const void *)out_size == (const void *)out_off)) ||
        (uint64_t)n > 0xFFFFFFFFull)
        return CHIP_E_INVALID;
    *total = *n_over = 0;
    if (n == 0) return CHIP_OK;
    return with_slot(
        g_zplan_cache, stream,
        [&](ZplanSlot &sl, hipStream_t s) { return layout_locked(sl, n, out_size, out_off, out_cap, total, n_over, s); },
        [&] { *total = *n_over = 0; });
}

}  // extern "C"
