// Reading ranges: random access on a plan.  Given the four arrays of a plan and many byte ranges of the
// decoded content, chip_select_units[_host] names the units the ranges touch and where each range lies in their decoded image;
// a read decodes exactly those units once and lands the ranges end to end.  The definition is in include/compu_hip.h; the host
// walk and the kernels below implement it.  One driver, read_locked<Source>(), serves three sources of units: the caller's plan
// (chip_read_ranges, PlanSource), the chunks of a checkpoint index (chip_inflate_index_read, sec. 4.16, IndexSource) and a plan
// with a checksum per unit (chip_zstd_seek_read, sec. 4.25, SeekSource).  The phases on the device, in stream order:
//   0. units    Source::carve and units: an index fills the four arrays of its units, arrays of its own in buffer ARRAYS; a plan
//               brings them
//   1. link     one lane per unit: out_off[i] + out_cap[i] == out_off[i + 1], no unsized cap, no wrap; the lowest failing link wins
//               (every later kernel returns at once when there is one: a broken layout writes nothing)
//   2. span     one lane per range: verdict, two binary searches, +1 at first and -1 behind last in a zeroed difference array
//   3. cover    exclusive scan of the differences; a unit is selected when its coverage is not 0 and it has content
//   4. select   exclusive {count, bytes} scan over the selected units, scatter of the sub-batch rows
//   5. ranges   exclusive scan of the lengths that count (dst_off), then per range src_off and the status
//      -- the host reads {n_sel, scratch_bytes, out_len} and compares with the room --
//   6. decode   Source::decode: the sub-batch (a BatchArgs) into the slot's area, buffer AREA of Source::area bytes:
//               chip_decode_batch for a plan, resumed units for an index
//   7. verify   (Source::decode still) one lane per selected unit: a unit that is not "good" as its source defines it gets
//               flag[k] = 1, is counted in ds->n_bad, the lowest one kept in ds->bad_key; a prefix count of the flags tells each
//               range whether its span holds one
//   8. copy     the destination-driven copy of pack_copy.h: src = Source::image, the selected units' content end to end (a source
//               that has to lay it there enqueues that first), src_off, the counted lengths, dst_off
// Order between the phases comes from kernel boundaries on the stream only.  The atomics are integer sums, maxima and counts: the
// result does not depend on their order.
#include <new>
#include <vector>

#include "chip_internal.h"
#include "launch_slots.h"
#include "pack_copy.h"
#include "plan_common.h"
#include "wave_checksums.h"

namespace chip {

namespace {

constexpr uint32_t NO_UNIT = 0xFFFFFFFFu;  // first[r] of a range that touches no unit (n_units <= 2^32 - 1: never an index)

// 32-bit sums for the scans (a class type: the scans find operator+ and shfl_up_t at their instantiation).  Coverage counts are
// sums of +1 / -1 modulo 2^32; the true value is at most n_ranges <= 2^32 - 1, so "not 0" is exact.
struct Cnt32 {
    uint32_t v;
};
__host__ __device__ __forceinline__ Cnt32 operator+(const Cnt32 &a, const Cnt32 &b) { return Cnt32{a.v + b.v}; }
__device__ __forceinline__ Cnt32 shfl_up_t(const Cnt32 &a, uint32_t d) { return Cnt32{(uint32_t)__shfl_up((int)a.v, d, 64)}; }

struct UnitAcc {
    uint64_t count, bytes;  // selected units, and their out_cap
};
__host__ __device__ __forceinline__ UnitAcc operator+(const UnitAcc &a, const UnitAcc &b) { return UnitAcc{a.count + b.count, a.bytes + b.bytes}; }
__device__ __forceinline__ UnitAcc shfl_up_t(const UnitAcc &a, uint32_t d) { return UnitAcc{shfl_up_t(a.count, d), shfl_up_t(a.bytes, d)}; }

// what the kernels hand to the host (device memory, zeroed per call, copied back behind phase 5 and at the end)
struct DevSummary {
    UnitAcc sel;         // total of the selection scan: n_sel, scratch_bytes
    uint64_t out_len;    // total of the range scan
    uint64_t n_outside;
    uint64_t bad_link;   // ~(the lowest i + 1 whose link fails), 0: the chain holds
    uint64_t bad_key;    // ~(the lowest bad unit's index) << 32 | its status, 0: none
    uint64_t n_bad;
    Cnt32 cover_total, flag_total;  // totals of the two 32-bit scans (nobody reads them)
};

// the link i -> i + 1 of the layout check
__host__ __device__ __forceinline__ bool link_fails(const uint64_t *out_off, const uint32_t *out_cap, uint64_t n, uint64_t i)
{
    const uint64_t a = out_off[i], s = a + out_cap[i];
    return out_cap[i] == CHIP_ZPLAN_UNSIZED || s < a || (i + 1 < n && out_off[i + 1] != s);
}

// the last unit that starts at or in front of pos: the one that holds byte pos (empty units at pos sit in front of it), as
// pack_copy_kernel finds it.  out_off[0] <= pos.
__host__ __device__ __forceinline__ uint32_t unit_of(const uint64_t *out_off, uint32_t n, uint64_t pos)
{
    uint32_t u = 0, b = n;  // out_off[u] <= pos, and out_off[b] > pos or b == n
    while (b - u > 1u) {
        const uint32_t mid = u + ((b - u) >> 1);
        if (out_off[mid] <= pos) u = mid;
        else b = mid;
    }
    return u;
}

// the verdict on one range: CHIP_RANGE_OK with len > 0 touches units
__host__ __device__ __forceinline__ int32_t range_verdict(uint64_t begin, uint64_t end, uint64_t lo, uint32_t len)
{
    if (len == 0) return CHIP_RANGE_OK;
    return (lo < begin || lo > end || len > end - lo) ? CHIP_RANGE_OUTSIDE : CHIP_RANGE_OK;  // (lo + len is never formed: no wrap)
}

__global__ __launch_bounds__(256) void rr_link_kernel(const uint64_t *out_off, const uint32_t *out_cap, uint64_t n, DevSummary *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (link_fails(out_off, out_cap, n, i)) atomicMax((unsigned long long *)&ds->bad_link, (unsigned long long)~(i + 1));
}

__global__ __launch_bounds__(256) void rr_span_kernel(const uint64_t *out_off, const uint32_t *out_cap, uint32_t n, const uint64_t *range_lo,
                                                      const uint32_t *range_len, uint64_t m, uint32_t *diff, uint32_t *first, uint32_t *last,
                                                      uint64_t *wide, uint32_t *counted, DevSummary *ds)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= m || ds->bad_link) return;
    const uint64_t begin = n ? out_off[0] : 0, end = n ? out_off[n - 1] + out_cap[n - 1] : 0;
    const uint64_t lo = range_lo[r];
    const uint32_t len = range_len[r];
    const int32_t verdict = range_verdict(begin, end, lo, len);
    uint32_t f = NO_UNIT, l = NO_UNIT, cnt = 0;
    if (verdict == CHIP_RANGE_OUTSIDE) {
        atomicAdd((unsigned long long *)&ds->n_outside, 1ull);
    } else if (len) {
        f = unit_of(out_off, n, lo);
        l = unit_of(out_off, n, lo + (len - 1u));
        atomicAdd(&diff[f], 1u);
        atomicAdd(&diff[(uint64_t)l + 1], ~0u);  // (-1; the array has n + 1 entries)
        cnt = len;
    }
    first[r] = f;
    last[r] = l;
    wide[r] = cnt;
    counted[r] = cnt;
}

// behind the coverage scan: the selected flag and the {1, out_cap} the selection scan sums
__global__ __launch_bounds__(256) void rr_flags_kernel(const uint32_t *diff, const Cnt32 *cover, const Cnt32 *cover_part, const uint32_t *out_cap,
                                                       uint64_t n, UnitAcc *acc, const DevSummary *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n || ds->bad_link) return;
    const uint32_t c = cover[i].v + cover_part[i / SCAN_THREADS].v + diff[i], cap = out_cap[i];
    acc[i] = (c != 0 && cap != 0) ? UnitAcc{1, cap} : UnitAcc{0, 0};
}

// behind the selection scan: acc[i] gets its workgroup's offset ({k, sel_out_off} of a selected unit) and the rows of the
// sub-batch are written (the first max_sel of them).
__global__ __launch_bounds__(256) void rr_scatter_kernel(const uint64_t *in_off, const uint32_t *in_len, const uint32_t *out_cap, UnitAcc *acc,
                                                         const UnitAcc *acc_part, const uint32_t *diff, const Cnt32 *cover, const Cnt32 *cover_part,
                                                         uint64_t n, uint64_t max_sel, uint32_t *sel_unit, uint64_t *sel_in_off, uint32_t *sel_in_len,
                                                         uint64_t *sel_out_off, uint32_t *sel_out_cap, const DevSummary *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n || ds->bad_link) return;
    const UnitAcc e = acc[i] + acc_part[i / SCAN_THREADS];
    acc[i] = e;
    const uint32_t c = cover[i].v + cover_part[i / SCAN_THREADS].v + diff[i], cap = out_cap[i];
    if (c == 0 || cap == 0 || e.count >= max_sel) return;
    sel_unit[e.count] = (uint32_t)i;
    sel_in_off[e.count] = in_off[i];
    sel_in_len[e.count] = in_len[i];
    sel_out_off[e.count] = e.bytes;
    sel_out_cap[e.count] = cap;
}

// behind the range scan: wide[r] becomes dst_off[r]; src_off and the status per range.  The caller's arrays may be null.
__global__ __launch_bounds__(256) void rr_ranges_kernel(const uint64_t *range_lo, const uint32_t *range_len, const uint64_t *out_off,
                                                        const uint32_t *first, const UnitAcc *acc, uint64_t *wide, const uint64_t *wide_part, uint64_t m,
                                                        uint64_t *src, uint64_t *user_src, uint64_t *user_dst, int32_t *user_status,
                                                        const DevSummary *ds)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= m || ds->bad_link) return;
    const uint64_t d = wide[r] + wide_part[r / SCAN_THREADS];
    const uint32_t f = first[r];
    const uint64_t s = f == NO_UNIT ? 0 : acc[f].bytes + (range_lo[r] - out_off[f]);
    wide[r] = d;
    src[r] = s;
    if (user_src) user_src[r] = s;
    if (user_dst) user_dst[r] = d;
    if (user_status) user_status[r] = (f == NO_UNIT && range_len[r]) ? CHIP_RANGE_OUTSIDE : CHIP_RANGE_OK;
}

// behind the decode: the selected units that did not decode to their size
__global__ __launch_bounds__(256) void rr_verify_kernel(const uint32_t *sel_unit, const uint32_t *sel_cap, const uint32_t *out_len,
                                                        const int32_t *status, uint64_t n_sel, Cnt32 *flag, DevSummary *ds)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_sel) return;
    const int32_t st = status[k];
    const bool bad = st != CHIP_FINISHED || out_len[k] != sel_cap[k];
    flag[k] = Cnt32{bad ? 1u : 0u};
    if (!bad) return;
    atomicAdd((unsigned long long *)&ds->n_bad, 1ull);
    atomicMax((unsigned long long *)&ds->bad_key, ((unsigned long long)(uint32_t)~sel_unit[k] << 32) | (uint32_t)st);
}

// behind the scan of the bad flags: a range whose span [k(first), k(last)] holds a bad unit
__global__ __launch_bounds__(256) void rr_bad_ranges_kernel(const uint32_t *first, const uint32_t *last, const UnitAcc *acc, const Cnt32 *flag,
                                                            const Cnt32 *excl, const Cnt32 *excl_part, uint64_t m, int32_t *user_status)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= m || first[r] == NO_UNIT) return;
    const uint64_t kf = acc[first[r]].count, kl = acc[last[r]].count;
    const uint32_t before = excl[kf].v + excl_part[kf / SCAN_THREADS].v, upto = excl[kl].v + excl_part[kl / SCAN_THREADS].v + flag[kl].v;
    if (upto != before) user_status[r] = CHIP_RANGE_BAD_UNIT;
}

// The scratch of one (device, stream): buffer 0 the per-unit and per-range arrays, buffer 1 the decoded image of the selected
// units.  A launch slot.
using ReadSlot = SummarySlot<DevSummary>;
constexpr uint32_t ARRAYS = 0, AREA = 1;
SlotCache<ReadSlot> g_read_cache;

// what a call hands to select_locked: the plan, the ranges and the caller's outputs (any of them may be null)
struct SelectArgs {
    uint64_t n, m;
    const uint64_t *in_off;
    const uint32_t *in_len;
    const uint64_t *out_off;
    const uint32_t *out_cap;
    const uint64_t *range_lo;
    const uint32_t *range_len;
    uint64_t max_sel;
    uint32_t *sel_unit;
    uint64_t *sel_in_off;
    uint32_t *sel_in_len;
    uint64_t *sel_out_off;
    uint32_t *sel_out_cap;
    uint64_t *src_off, *dst_off;
    int32_t *range_status;
};

// where the arrays lie in buffer 0 (byte offsets, each a multiple of 16)
struct Carve {
    size_t at = 0;
    size_t take(uint64_t count, size_t each)
    {
        const size_t o = at;
        at = up16(at + (size_t)count * each);
        return o;
    }
};
struct Arrays {
    // selection: 24 bytes per unit and 28 per range, and the scans' partials
    size_t acc, acc_part, wide, wide_part, src, diff, cover, cover_part, first, last, counted;
    // chip_read_ranges: the sub-batch and what the decode answers, 48 bytes per unit (the selection may be all of them)
    size_t s_in_off, s_out_off, s_unit, s_in_len, s_cap, d_out_len, d_in_used, d_status, flag, flag_excl, flag_part;
    size_t bytes;
};
Arrays carve_arrays(uint64_t n, uint64_t m, bool read)
{
    Carve c;
    Arrays a{};
    a.acc = c.take(n, sizeof(UnitAcc)), a.acc_part = c.take(scan_parts(n), sizeof(UnitAcc));
    a.wide = c.take(m, 8), a.wide_part = c.take(scan_parts(m), 8), a.src = c.take(m, 8);
    a.diff = c.take(n + 1, 4), a.cover = c.take(n, 4), a.cover_part = c.take(scan_parts(n), 4);
    a.first = c.take(m, 4), a.last = c.take(m, 4), a.counted = c.take(m, 4);
    if (read) {
        a.s_in_off = c.take(n, 8), a.s_out_off = c.take(n, 8), a.s_unit = c.take(n, 4), a.s_in_len = c.take(n, 4), a.s_cap = c.take(n, 4);
        a.d_out_len = c.take(n, 4), a.d_in_used = c.take(n, 4), a.d_status = c.take(n, 4);
        a.flag = c.take(n, 4), a.flag_excl = c.take(n, 4), a.flag_part = c.take(scan_parts(n), 4);
    }
    a.bytes = c.at;
    return a;
}

inline dim3 grid256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// Phases 1 to 5: enqueues everything and waits for the summary (in sl.h_sum).  m > 0; buffer 0 holds `a`.
hipError_t select_locked(ReadSlot &sl, const Arrays &a, const SelectArgs &g, hipStream_t stream)
{
    uint8_t *b = sl.buf[ARRAYS];
    DevSummary *ds = sl.d_sum;
    UnitAcc *acc = (UnitAcc *)(b + a.acc), *acc_part = (UnitAcc *)(b + a.acc_part);
    uint64_t *wide = (uint64_t *)(b + a.wide), *wide_part = (uint64_t *)(b + a.wide_part), *src = (uint64_t *)(b + a.src);
    uint32_t *diff = (uint32_t *)(b + a.diff), *first = (uint32_t *)(b + a.first), *last = (uint32_t *)(b + a.last);
    uint32_t *counted = (uint32_t *)(b + a.counted);
    Cnt32 *cover = (Cnt32 *)(b + a.cover), *cover_part = (Cnt32 *)(b + a.cover_part);
    const uint64_t n = g.n, m = g.m;
    hipError_t e = hipMemsetAsync(ds, 0, sizeof(DevSummary), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(diff, 0, (size_t)(n + 1) * 4, stream)) != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(rr_link_kernel, grid256(n), dim3(256), 0, stream, g.out_off, g.out_cap, n, ds);
    hipLaunchKernelGGL(rr_span_kernel, grid256(m), dim3(256), 0, stream, g.out_off, g.out_cap, (uint32_t)n, g.range_lo, g.range_len, m, diff, first, last,
                       wide, counted, ds);
    if (n) {
        enqueue_scan<Cnt32>((const Cnt32 *)diff, cover, n, cover_part, &ds->cover_total, stream);
        hipLaunchKernelGGL(rr_flags_kernel, grid256(n), dim3(256), 0, stream, (const uint32_t *)diff, (const Cnt32 *)cover, (const Cnt32 *)cover_part,
                           g.out_cap, n, acc, (const DevSummary *)ds);
        enqueue_scan<UnitAcc>(acc, acc, n, acc_part, &ds->sel, stream);
        hipLaunchKernelGGL(rr_scatter_kernel, grid256(n), dim3(256), 0, stream, g.in_off, g.in_len, g.out_cap, acc, (const UnitAcc *)acc_part,
                           (const uint32_t *)diff, (const Cnt32 *)cover, (const Cnt32 *)cover_part, n, g.max_sel, g.sel_unit, g.sel_in_off, g.sel_in_len,
                           g.sel_out_off, g.sel_out_cap, (const DevSummary *)ds);
    }
    enqueue_scan<uint64_t>(wide, wide, m, wide_part, &ds->out_len, stream);
    hipLaunchKernelGGL(rr_ranges_kernel, grid256(m), dim3(256), 0, stream, g.range_lo, g.range_len, g.out_off, (const uint32_t *)first,
                       (const UnitAcc *)acc, wide, (const uint64_t *)wide_part, m, src, g.src_off, g.dst_off, g.range_status, (const DevSummary *)ds);
    return sl.fetch(stream);
}

chip_select_summary select_summary(const DevSummary &h)
{
    if (h.bad_link) return chip_select_summary{0, 0, 0, 0, ~h.bad_link, CHIP_READ_BAD_LAYOUT, 0};
    return chip_select_summary{h.sel.count, h.sel.bytes, h.out_len, h.n_outside, 0, CHIP_READ_OK, 0};
}

hipError_t select_units_locked(ReadSlot &sl, const SelectArgs &g, chip_select_summary *summary, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    const Arrays a = carve_arrays(g.n, g.m, false);
    if ((e = sl.grow(ARRAYS, a.bytes)) != hipSuccess) return e;
    if ((e = select_locked(sl, a, g, stream)) != hipSuccess) return e;
    *summary = select_summary(*sl.h_sum);
    return hipSuccess;
}

bool range_args_ok(size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len)
{
    return (uint64_t)n_ranges <= 0xFFFFFFFFull && !(n_ranges && (!range_lo || !range_len));
}

bool plan_args_ok(size_t n_units, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap, size_t n_ranges,
                  const uint64_t *range_lo, const uint32_t *range_len)
{
    if ((uint64_t)n_units > 0xFFFFFFFFull || (n_units && (!in_off || !in_len || !out_off || !out_cap))) return false;
    return range_args_ok(n_ranges, range_lo, range_len);
}

bool select_args_ok(size_t n_units, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap, size_t n_ranges,
                    const uint64_t *range_lo, const uint32_t *range_len, uint64_t max_sel, const uint32_t *sel_unit, const uint64_t *sel_in_off,
                    const uint32_t *sel_in_len, const uint64_t *sel_out_off, const uint32_t *sel_out_cap, const chip_select_summary *summary)
{
    if (!summary || !plan_args_ok(n_units, in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len)) return false;
    return !(max_sel && (!sel_unit || !sel_in_off || !sel_in_len || !sel_out_off || !sel_out_cap));
}

bool decode_format_ok(int format)
{
    return format == CHIP_FMT_DEFLATE || format == CHIP_FMT_ZLIB || format == CHIP_FMT_GZIP || format == CHIP_FMT_AUTO || format == CHIP_FMT_ZSTD ||
           format == CHIP_FMT_BROTLI || format == CHIP_FMT_DETECT;
}

// ---- reading through the checkpoint index of one large stream --------------------------------------------
// The units are the chunks of an index.  What IndexSource (further down) puts into the source's phases of the walk above:
//   0. units    one lane per chunk: in_off, in_len, out_cap by index_chunk(), out_off = pt_out; a chunk that offends the layout gets
//               the cap CHIP_ZPLAN_UNSIZED, so that phase 1 fails at exactly that link (an honest chunk's link to its successor
//               holds by construction) and nothing else is written
//   6a. stage   one lane per selected chunk: its slot [window | chunk] in the area, the resume words, where its content starts
//   6b. window  four waves per selected chunk: the window slot of the index goes to the front of the chunk's slot
//   6c. decode  launch_inflate() with BatchArgs::resume: the chunks are resumed units of inflate_kernel
//   7. verify   one lane per selected chunk: the link to the next point (or the end of the stream) as the header defines "good"
//   8. copy     once more pack_copy.h's copy, in front of the driver's: the chunks' content goes end to end into an image behind
//               the slots (the windows between them are gone); the ranges are gathered from that image
constexpr uint32_t IX_WINDOW = 32768;
constexpr uint64_t IX_CAP_MAX = 0xFFFFFFF0ull - IX_WINDOW;

struct IxChunk {
    uint64_t in_off;
    uint32_t in_len, out_cap, wl, r0;
    bool bad;
};
// chunk k of the index: the arithmetic of include/compu_hip.h (8 * len does not wrap: len <= 2^61)
__host__ __device__ __forceinline__ IxChunk index_chunk(const uint64_t *pt_bit, const uint64_t *pt_out, uint64_t n, uint64_t len, uint64_t total_out,
                                                        uint64_t k)
{
    const uint64_t bit = pt_bit[k], o = pt_out[k];
    const bool more = k + 1 < n;
    const uint64_t next_bit = more ? pt_bit[k + 1] : 0;
    const uint64_t end_out = more ? pt_out[k + 1] : total_out, end_in = more ? (next_bit >> 3) + ((next_bit & 7u) ? 1u : 0u) : len;
    IxChunk c{};
    c.in_off = (bit >> 3) - (((bit & 7u) == 0 && bit != 0) ? 1u : 0u);
    c.bad = (k == 0 && o != 0) || bit >= 8 * len || (more && next_bit <= bit) || end_out < o || end_out - o > IX_CAP_MAX || end_in < c.in_off ||
            end_in - c.in_off > CHIP_GZPLAN_WINDOW;
    if (c.bad) return c;
    c.in_len = (uint32_t)(end_in - c.in_off);
    c.out_cap = (uint32_t)(end_out - o);
    c.wl = o < IX_WINDOW ? (uint32_t)o : IX_WINDOW;
    c.r0 = (uint32_t)(bit - 8 * c.in_off);
    return c;
}
__host__ __device__ __forceinline__ void index_resume_words(const IxChunk &c, uint32_t wrap, uint32_t check, uint64_t o, uint32_t *rs)
{
    rs[0] = c.r0, rs[1] = c.wl, rs[2] = wrap, rs[3] = check, rs[4] = (uint32_t)o, rs[5] = (uint32_t)(o - c.wl);
}

__global__ __launch_bounds__(256) void ix_units_kernel(const uint64_t *pt_bit, const uint64_t *pt_out, uint64_t n, uint64_t len, uint64_t total_out,
                                                       uint64_t *in_off, uint32_t *in_len, uint32_t *out_cap)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const IxChunk c = index_chunk(pt_bit, pt_out, n, len, total_out, k);
    in_off[k] = c.bad ? 0 : c.in_off;
    in_len[k] = c.in_len;
    out_cap[k] = c.bad ? CHIP_ZPLAN_UNSIZED : c.out_cap;
}

// selected chunk j's slot is area[sel_out_off[j] + 32768 j, + 32768 + cap): the content starts 32 KiB in, the window ends there
__global__ __launch_bounds__(256) void ix_stage_kernel(const uint64_t *pt_bit, const uint64_t *pt_out, const uint32_t *pt_check, uint64_t n, uint64_t len,
                                                       uint64_t total_out, uint32_t wrap, const uint32_t *sel_unit, const uint64_t *sel_out_off,
                                                       uint64_t n_sel, uint64_t *slot_off, uint32_t *slot_cap, uint64_t *content_off, uint32_t *resume)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    const uint64_t k = sel_unit[j];
    const IxChunk c = index_chunk(pt_bit, pt_out, n, len, total_out, k);
    const uint64_t at = sel_out_off[j] + (uint64_t)IX_WINDOW * (j + 1);
    content_off[j] = at;
    slot_off[j] = at - c.wl;
    slot_cap[j] = c.wl + c.out_cap;
    index_resume_words(c, wrap, pt_check[k], pt_out[k], resume + RESUME_WORDS * j);
}

__global__ __launch_bounds__(256) void ix_window_kernel(const uint8_t *windows, const uint32_t *sel_unit, const uint64_t *slot_off,
                                                        const uint64_t *content_off, uint8_t *area)
{
    const uint32_t lane = lane_id(), wave = rdfirst(threadIdx.x >> 6);
    const uint64_t at = rdfirst64(slot_off[blockIdx.x]);
    const uint32_t wl = (uint32_t)(rdfirst64(content_off[blockIdx.x]) - at);
    const uint8_t *src = windows + (uint64_t)IX_WINDOW * rdfirst(sel_unit[blockIdx.x]);
    uint8_t *dst = area + at;
    for (uint32_t p = wave * PACK_TILE; p < wl; p += 4 * PACK_TILE) copy_span(src + p, dst + p, wl - p < PACK_TILE ? wl - p : PACK_TILE, lane);
}

// behind the decode: the chunks whose link to the next point (or to the end of the stream) does not hold
__global__ __launch_bounds__(256) void ix_verify_kernel(const uint64_t *pt_bit, const uint32_t *pt_check, uint64_t n, const uint32_t *sel_unit,
                                                        const uint64_t *sel_in_off, const uint32_t *slot_cap, const uint32_t *resume,
                                                        const uint32_t *out_len, const int32_t *status, uint64_t n_sel, Cnt32 *flag, DevSummary *ds)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    const uint64_t k = sel_unit[j];
    const int32_t st = status[j];
    const uint32_t *rs = resume + RESUME_WORDS * j;
    bool good = out_len[j] == slot_cap[j];
    if (k + 1 < n)
        good = good && (st == CHIP_NEED_INPUT || st == CHIP_NEED_OUTPUT) && rs[0] == (uint32_t)(pt_bit[k + 1] - 8 * sel_in_off[j]) &&
               rs[1] == slot_cap[j] && rs[3] == pt_check[k + 1];
    else good = good && st == CHIP_FINISHED;
    flag[j] = Cnt32{good ? 0u : 1u};
    if (good) return;
    atomicAdd((unsigned long long *)&ds->n_bad, 1ull);
    atomicMax((unsigned long long *)&ds->bad_key, ((unsigned long long)(uint32_t)~sel_unit[j] << 32) | (uint32_t)st);
}

bool index_format_ok(int format) { return format == CHIP_FMT_DEFLATE || format == CHIP_FMT_ZLIB || format == CHIP_FMT_GZIP; }
uint32_t index_wrap(int format) { return format == CHIP_FMT_DEFLATE ? 0u : format == CHIP_FMT_ZLIB ? 1u : 2u; }

// ---- the read driver and its two sources ---------------------------------------------------------------------------------------
// A source is the template parameter of read_locked(), as D is plan_locked()'s: the hooks the phase list at the top names, none of
// which waits for the stream, and LINK_BACK, how far the failing link that select_summary() names is ahead of the bad_index that
// the source's header promises.
struct PlanSource {
    void carve(Carve &) {}
    void units(uint8_t *, SelectArgs &, hipStream_t) {}
    static constexpr uint64_t LINK_BACK = 0;
    static size_t area(const chip_select_summary &s) { return (size_t)s.scratch_bytes + 64; }  // the units end to end, 64 bytes of slack
    static hipError_t decode(const BatchArgs &ba, const uint32_t *unit, Cnt32 *flag, DevSummary *ds, hipStream_t stream)
    {
        const int rc = chip_decode_batch(ba.format, ba.n, ba.in_base, ba.in_off, ba.in_len, ba.out_base, ba.out_off, ba.out_cap, ba.out_len, ba.in_used,
                                         ba.status, stream);
        if (rc != CHIP_OK) return rc == CHIP_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;  // (CHIP_E_LAUNCH)
        hipLaunchKernelGGL(rr_verify_kernel, grid256(ba.n), dim3(256), 0, stream, unit, ba.out_cap, (const uint32_t *)ba.out_len,
                           (const int32_t *)ba.status, (uint64_t)ba.n, flag, ds);
        return hipSuccess;
    }
    static const uint8_t *image(const BatchArgs &ba, uint64_t, hipStream_t) { return ba.out_base; }
};

struct IndexSource {
    uint64_t len, n, total_out;
    const uint64_t *pt_bit, *pt_out;
    const uint32_t *pt_check;
    const uint8_t *windows;
    // in buffer ARRAYS: the chunks as units (16 bytes per chunk), the slots (20), the resume words (24)
    size_t o_in_off = 0, o_in_len = 0, o_cap = 0, o_slot_off = 0, o_content = 0, o_slot_cap = 0, o_resume = 0;
    uint64_t *slot_off = nullptr, *content_off = nullptr;
    uint32_t *slot_cap = nullptr, *resume = nullptr;

    void carve(Carve &c)
    {
        o_in_off = c.take(n, 8), o_in_len = c.take(n, 4), o_cap = c.take(n, 4), o_slot_off = c.take(n, 8), o_content = c.take(n, 8);
        o_slot_cap = c.take(n, 4), o_resume = c.take(n, 4 * RESUME_WORDS);
    }
    void units(uint8_t *b, SelectArgs &g, hipStream_t stream)
    {
        uint64_t *u_in_off = (uint64_t *)(b + o_in_off);
        uint32_t *u_in_len = (uint32_t *)(b + o_in_len), *u_cap = (uint32_t *)(b + o_cap);
        slot_off = (uint64_t *)(b + o_slot_off), content_off = (uint64_t *)(b + o_content);
        slot_cap = (uint32_t *)(b + o_slot_cap), resume = (uint32_t *)(b + o_resume);
        if (n) hipLaunchKernelGGL(ix_units_kernel, grid256(n), dim3(256), 0, stream, pt_bit, pt_out, n, len, total_out, u_in_off, u_in_len, u_cap);
        g.in_off = u_in_off, g.in_len = u_in_len, g.out_off = pt_out, g.out_cap = u_cap;
    }
    static constexpr uint64_t LINK_BACK = 1;  // (the failing link i is the lowest offending chunk: select_summary() says i + 1)
    // the slots [window | chunk] of the selected chunks, then the image of their content end to end (64 bytes of slack behind each)
    static size_t image_at(uint64_t n_sel, uint64_t scratch_bytes) { return up16((size_t)scratch_bytes + (size_t)IX_WINDOW * n_sel + 64); }
    static size_t area(const chip_select_summary &s) { return image_at(s.n_sel, s.scratch_bytes) + (size_t)s.scratch_bytes + 64; }
    hipError_t decode(const BatchArgs &ba, const uint32_t *unit, Cnt32 *flag, DevSummary *ds, hipStream_t stream) const
    {
        const uint64_t n_sel = ba.n;
        hipLaunchKernelGGL(ix_stage_kernel, grid256(n_sel), dim3(256), 0, stream, pt_bit, pt_out, pt_check, n, len, total_out, index_wrap(ba.format), unit,
                           ba.out_off, n_sel, slot_off, slot_cap, content_off, resume);
        hipLaunchKernelGGL(ix_window_kernel, dim3(ba.n), dim3(256), 0, stream, windows, unit, (const uint64_t *)slot_off,
                           (const uint64_t *)content_off, ba.out_base);
        BatchArgs r = ba;  // the chunks as resumed units, each into its slot
        r.out_off = slot_off, r.out_cap = slot_cap, r.resume = resume;
        const hipError_t e = launch_inflate(r, nullptr, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(ix_verify_kernel, grid256(n_sel), dim3(256), 0, stream, pt_bit, pt_check, n, unit, ba.in_off, (const uint32_t *)slot_cap,
                           (const uint32_t *)resume, (const uint32_t *)ba.out_len, (const int32_t *)ba.status, n_sel, flag, ds);
        return hipSuccess;
    }
    const uint8_t *image(const BatchArgs &ba, uint64_t scratch_bytes, hipStream_t stream) const
    {
        uint8_t *image = ba.out_base + image_at(ba.n, scratch_bytes);
        enqueue_copy(ba.n, ba.out_base, (const uint64_t *)content_off, ba.out_cap, image, ba.out_off, scratch_bytes, stream);
        return image;
    }
};

// ---- reading through a seek table with per-frame checksums ------------------------------------------------
// The units are a plan's, decoded and verified as PlanSource does it.  Behind that, phase 7 goes on: one wave per selected unit that
// is not bad already hashes the unit's image (XXH64, wave_checksums.h); a unit whose low 32 bits differ from the table's entry is a
// bad unit with the decoder's own status for a wrong content checksum.
__global__ __launch_bounds__(64) void rr_hash_kernel(const uint8_t *image, const uint64_t *sel_out_off, const uint32_t *sel_cap, const uint32_t *sel_unit,
                                                     const uint32_t *checksum, Cnt32 *flag, DevSummary *ds)
{
    __shared__ uint64_t stage[512];
    const uint32_t k = blockIdx.x;
    if (flag[k].v) return;  // (uniform) counted by rr_verify_kernel
    const uint32_t unit = sel_unit[k];
    const uint32_t got = wave_xxh64_low32(stage, image + sel_out_off[k], sel_cap[k]);
    if (lane_id() != 0 || got == checksum[unit]) return;
    flag[k] = Cnt32{1u};
    atomicAdd((unsigned long long *)&ds->n_bad, 1ull);
    atomicMax((unsigned long long *)&ds->bad_key, ((unsigned long long)(uint32_t)~unit << 32) | (uint32_t)-ZSTD_E_CHECKSUM_WRONG);
}

struct SeekSource {
    const uint32_t *checksum;  // per unit of the plan

    void carve(Carve &) {}
    void units(uint8_t *, SelectArgs &, hipStream_t) {}
    static constexpr uint64_t LINK_BACK = PlanSource::LINK_BACK;
    static size_t area(const chip_select_summary &s) { return PlanSource::area(s); }
    hipError_t decode(const BatchArgs &ba, const uint32_t *unit, Cnt32 *flag, DevSummary *ds, hipStream_t stream) const
    {
        const hipError_t e = PlanSource::decode(ba, unit, flag, ds, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(rr_hash_kernel, dim3(ba.n), dim3(64), 0, stream, (const uint8_t *)ba.out_base, ba.out_off, ba.out_cap, unit, checksum, flag, ds);
        return hipSuccess;
    }
    static const uint8_t *image(const BatchArgs &ba, uint64_t scratch_bytes, hipStream_t stream) { return PlanSource::image(ba, scratch_bytes, stream); }
};

SlotCache<ReadSlot> g_index_read_cache;

constexpr chip_select_summary SELECT_NOTHING{0, 0, 0, 0, 0, CHIP_READ_OK, 0};
constexpr chip_read_summary READ_NOTHING{0, 0, 0, 0, 0, 0, CHIP_READ_OK, 0};

// One read: enqueues everything, waits twice (the sizes, the end).  g brings the ranges and the caller's outputs, with a plan its
// four arrays.  The caller holds the cache's lock.
template <class Source>
hipError_t read_locked(ReadSlot &sl, Source src, int format, const uint8_t *in_base, SelectArgs g, uint8_t *dst_base, uint64_t dst_cap,
                       chip_read_summary *summary, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    const uint64_t n = g.n, m = g.m;
    const Arrays a = carve_arrays(n, m, true);
    Carve c{a.bytes};
    src.carve(c);
    if ((e = sl.grow(ARRAYS, c.at)) != hipSuccess) return e;
    uint8_t *b = sl.buf[ARRAYS];
    g.max_sel = n;
    g.sel_unit = (uint32_t *)(b + a.s_unit), g.sel_in_off = (uint64_t *)(b + a.s_in_off), g.sel_in_len = (uint32_t *)(b + a.s_in_len);
    g.sel_out_off = (uint64_t *)(b + a.s_out_off), g.sel_out_cap = (uint32_t *)(b + a.s_cap);
    src.units(b, g, stream);
    if ((e = select_locked(sl, a, g, stream)) != hipSuccess) return e;
    const chip_select_summary s = select_summary(*sl.h_sum);
    *summary = chip_read_summary{0, s.out_len, s.n_outside, 0, 0, s.status == CHIP_READ_OK ? 0 : s.bad_index - Source::LINK_BACK, s.status, 0};
    if (s.status == CHIP_READ_OK && s.out_len > dst_cap) summary->status = CHIP_READ_NEED_OUTPUT;
    if (summary->status != CHIP_READ_OK || s.n_sel == 0) return hipSuccess;  // (no unit: no byte either, a range that counts touches one)
    if (s.n_sel > 0x7fffffffull) return hipErrorUnknown;  // (more units than a batch counts)
    if ((e = sl.grow(AREA, Source::area(s))) != hipSuccess) return e;
    BatchArgs ba{};  // the sub-batch: the selected units decode into the area
    ba.format = format, ba.in_base = in_base, ba.n = (uint32_t)s.n_sel;
    ba.in_off = g.sel_in_off, ba.in_len = g.sel_in_len, ba.out_base = sl.buf[AREA], ba.out_off = g.sel_out_off, ba.out_cap = g.sel_out_cap;
    ba.out_len = (uint32_t *)(b + a.d_out_len), ba.in_used = (uint32_t *)(b + a.d_in_used), ba.status = (int32_t *)(b + a.d_status);
    Cnt32 *flag = (Cnt32 *)(b + a.flag), *flag_excl = (Cnt32 *)(b + a.flag_excl), *flag_part = (Cnt32 *)(b + a.flag_part);
    if ((e = src.decode(ba, (const uint32_t *)g.sel_unit, flag, sl.d_sum, stream)) != hipSuccess) return e;
    if (g.range_status) {
        enqueue_scan<Cnt32>(flag, flag_excl, s.n_sel, flag_part, &sl.d_sum->flag_total, stream);
        hipLaunchKernelGGL(rr_bad_ranges_kernel, grid256(m), dim3(256), 0, stream, (const uint32_t *)(b + a.first), (const uint32_t *)(b + a.last),
                           (const UnitAcc *)(b + a.acc), (const Cnt32 *)flag, (const Cnt32 *)flag_excl, (const Cnt32 *)flag_part, m, g.range_status);
    }
    enqueue_copy(m, src.image(ba, s.scratch_bytes, stream), (const uint64_t *)(b + a.src), (const uint32_t *)(b + a.counted), dst_base,
                 (const uint64_t *)(b + a.wide), s.out_len, stream);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;  // the slot is handed on only with nothing in flight
    const DevSummary &h = *sl.h_sum;
    summary->n_units = s.n_sel, summary->n_bad = h.n_bad;
    if (h.n_bad) {
        summary->first_bad = (uint32_t)~(uint32_t)(h.bad_key >> 32);
        summary->bad_status = (int32_t)(uint32_t)h.bad_key;
    }
    return hipSuccess;
}

// What both read entry points do once their arguments are in order.
template <class Source>
int read_with_slot(SlotCache<ReadSlot> &cache, const Source &src, int format, const void *in_base, const SelectArgs &g, void *dst_base, uint64_t dst_cap,
                   chip_read_summary *summary, void *stream)
{
    *summary = READ_NOTHING;
    if (g.m == 0) return CHIP_OK;
    return with_slot(
        cache, stream,
        [&](ReadSlot &sl, hipStream_t s) { return read_locked(sl, src, format, (const uint8_t *)in_base, g, (uint8_t *)dst_base, dst_cap, summary, s); },
        [&] { *summary = READ_NOTHING; });
}
}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_select_units_host(size_t n_units, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap,
                           size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, uint64_t max_sel, uint32_t *sel_unit,
                           uint64_t *sel_in_off, uint32_t *sel_in_len, uint64_t *sel_out_off, uint32_t *sel_out_cap, uint64_t *src_off,
                           uint64_t *dst_off, int32_t *range_status, chip_select_summary *summary)
{
    if (!select_args_ok(n_units, in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len, max_sel, sel_unit, sel_in_off, sel_in_len,
                        sel_out_off, sel_out_cap, summary))
        return CHIP_E_INVALID;
    *summary = SELECT_NOTHING;
    if (n_ranges == 0) return CHIP_OK;
    const uint64_t n = n_units, m = n_ranges;
    for (uint64_t i = 0; i < n; i++) {
        if (!link_fails(out_off, out_cap, n, i)) continue;
        summary->status = CHIP_READ_BAD_LAYOUT;
        summary->bad_index = i + 1;
        return CHIP_OK;
    }
    const uint64_t begin = n ? out_off[0] : 0, end = n ? out_off[n - 1] + out_cap[n - 1] : 0;
    std::vector<uint32_t> diff, first;   // coverage differences; first[r]
    std::vector<uint64_t> image;         // per unit: the selected bytes in front of it
    try {
        diff.assign((size_t)n + 1, 0u);
        first.assign((size_t)m, NO_UNIT);
        image.assign((size_t)n, 0);
    } catch (const std::bad_alloc &) {
        return CHIP_E_NOMEM;
    }
    uint64_t out_len = 0, n_outside = 0;
    for (uint64_t r = 0; r < m; r++) {
        const int32_t verdict = range_verdict(begin, end, range_lo[r], range_len[r]);
        uint32_t cnt = 0;
        if (verdict == CHIP_RANGE_OUTSIDE) {
            n_outside++;
        } else if (range_len[r]) {
            first[r] = unit_of(out_off, (uint32_t)n, range_lo[r]);
            diff[first[r]]++;
            diff[(size_t)unit_of(out_off, (uint32_t)n, range_lo[r] + (range_len[r] - 1u)) + 1]--;
            cnt = range_len[r];
        }
        if (dst_off) dst_off[r] = out_len;
        if (range_status) range_status[r] = verdict;
        out_len += cnt;
    }
    uint64_t n_sel = 0, bytes = 0;
    uint32_t cover = 0;
    for (uint64_t i = 0; i < n; i++) {
        cover += diff[i];
        image[i] = bytes;
        if (cover == 0 || out_cap[i] == 0) continue;
        if (n_sel < max_sel) {
            sel_unit[n_sel] = (uint32_t)i;
            sel_in_off[n_sel] = in_off[i];
            sel_in_len[n_sel] = in_len[i];
            sel_out_off[n_sel] = bytes;
            sel_out_cap[n_sel] = out_cap[i];
        }
        n_sel++;
        bytes += out_cap[i];
    }
    if (src_off)
        for (uint64_t r = 0; r < m; r++) src_off[r] = first[r] == NO_UNIT ? 0 : image[first[r]] + (range_lo[r] - out_off[first[r]]);
    *summary = chip_select_summary{n_sel, bytes, out_len, n_outside, 0, CHIP_READ_OK, 0};
    return CHIP_OK;
}

int chip_select_units(size_t n_units, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap,
                      size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, uint64_t max_sel, uint32_t *sel_unit,
                      uint64_t *sel_in_off, uint32_t *sel_in_len, uint64_t *sel_out_off, uint32_t *sel_out_cap, uint64_t *src_off, uint64_t *dst_off,
                      int32_t *range_status, chip_select_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!select_args_ok(n_units, in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len, max_sel, sel_unit, sel_in_off, sel_in_len,
                        sel_out_off, sel_out_cap, summary))
        return CHIP_E_INVALID;
    *summary = SELECT_NOTHING;
    if (n_ranges == 0) return CHIP_OK;
    const SelectArgs g{n_units, n_ranges, in_off, in_len, out_off, out_cap, range_lo, range_len, max_sel, sel_unit, sel_in_off, sel_in_len,
                       sel_out_off, sel_out_cap, src_off, dst_off, range_status};
    return with_slot(
        g_read_cache, stream, [&](ReadSlot &sl, hipStream_t s) { return select_units_locked(sl, g, summary, s); },
        [&] { *summary = SELECT_NOTHING; });
}

int chip_read_ranges(int format, size_t n_units, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off,
                     const uint32_t *out_cap, size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, void *dst_base, uint64_t dst_cap,
                     uint64_t *dst_off, int32_t *range_status, chip_read_summary *summary, void *stream)
{
    if (!summary || !plan_args_ok(n_units, in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len) || (n_units && !in_base) ||
        ((uintptr_t)in_base & 3u) || (dst_cap && !dst_base) || !decode_format_ok(format))
        return CHIP_E_INVALID;
    const SelectArgs g{n_units, n_ranges, in_off,  in_len,  out_off, out_cap, range_lo, range_len,   0,
                       nullptr, nullptr,  nullptr, nullptr, nullptr, nullptr, dst_off,  range_status};
    return read_with_slot(g_read_cache, PlanSource{}, format, in_base, g, dst_base, dst_cap, summary, stream);
}

int chip_zstd_seek_read(size_t n_units, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off,
                        const uint32_t *out_cap, const uint32_t *checksum, size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len,
                        void *dst_base, uint64_t dst_cap, uint64_t *dst_off, int32_t *range_status, chip_read_summary *summary, void *stream)
{
    if (!checksum)
        return chip_read_ranges(CHIP_FMT_ZSTD, n_units, in_base, in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len, dst_base, dst_cap,
                                dst_off, range_status, summary, stream);
    if (!summary || !plan_args_ok(n_units, in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len) || (n_units && !in_base) ||
        ((uintptr_t)in_base & 3u) || (dst_cap && !dst_base))
        return CHIP_E_INVALID;
    const SelectArgs g{n_units, n_ranges, in_off,  in_len,  out_off, out_cap, range_lo, range_len,   0,
                       nullptr, nullptr,  nullptr, nullptr, nullptr, nullptr, dst_off,  range_status};
    return read_with_slot(g_read_cache, SeekSource{checksum}, CHIP_FMT_ZSTD, in_base, g, dst_base, dst_cap, summary, stream);
}

int chip_inflate_index_units_host(int format, uint64_t len, uint64_t n_points, const uint64_t *pt_bit, const uint64_t *pt_out,
                                  const uint32_t *pt_check, uint64_t total_out, uint64_t *in_off, uint32_t *in_len, uint32_t *out_cap,
                                  uint32_t *win_len, uint32_t *resume, int32_t *status, uint64_t *bad_index)
{
    if (!status || !bad_index || !index_format_ok(format) || n_points > 0xFFFFFFFFull || len > (1ull << 61) ||
        (n_points && (!pt_bit || !pt_out || !pt_check)))
        return CHIP_E_INVALID;
    *status = CHIP_READ_OK;
    *bad_index = 0;
    for (uint64_t k = 0; k < n_points; k++) {
        if (!index_chunk(pt_bit, pt_out, n_points, len, total_out, k).bad) continue;
        *status = CHIP_READ_BAD_LAYOUT;
        *bad_index = k;
        return CHIP_OK;
    }
    for (uint64_t k = 0; k < n_points; k++) {
        const IxChunk c = index_chunk(pt_bit, pt_out, n_points, len, total_out, k);
        if (in_off) in_off[k] = c.in_off;
        if (in_len) in_len[k] = c.in_len;
        if (out_cap) out_cap[k] = c.out_cap;
        if (win_len) win_len[k] = c.wl;
        if (resume) index_resume_words(c, index_wrap(format), pt_check[k], pt_out[k], resume + RESUME_WORDS * k);
    }
    return CHIP_OK;
}

int chip_inflate_index_read(int format, const void *in_base, uint64_t len, uint64_t n_points, const uint64_t *pt_bit, const uint64_t *pt_out,
                            const uint32_t *pt_check, const void *windows, uint64_t total_out, size_t n_ranges, const uint64_t *range_lo,
                            const uint32_t *range_len, void *dst_base, uint64_t dst_cap, uint64_t *dst_off, int32_t *range_status,
                            chip_read_summary *summary, void *stream)
{
    if (!summary || !index_format_ok(format) || !in_base || ((uintptr_t)in_base & 3u) || len > (1ull << 61) || n_points > 0xFFFFFFFFull ||
        (n_points && (!pt_bit || !pt_out || !pt_check || !windows)) || !range_args_ok(n_ranges, range_lo, range_len) || (dst_cap && !dst_base))
        return CHIP_E_INVALID;
    const IndexSource x{len, n_points, total_out, pt_bit, pt_out, pt_check, (const uint8_t *)windows};
    const SelectArgs g{n_points, n_ranges, nullptr, nullptr, nullptr, nullptr, range_lo, range_len,    0,
                       nullptr,  nullptr,  nullptr, nullptr, nullptr, nullptr, dst_off,  range_status};
    return read_with_slot(g_index_read_cache, x, format, in_base, g, dst_base, dst_cap, summary, stream);
}

}  // extern "C"
