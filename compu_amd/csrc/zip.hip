// ZIP archives: chip_zip_plan[_host], chip_crc32_batch, chip_zip_decode.  The definitions are in
// include/compu_hip.h; the host walk and the per-record code that host and device share are in zip_plan_core.h.
//
// The plan.  The end record is searched by one workgroup over the last 64 KiB (zip_end_kernel; its thread 0 reads the ZIP64 records).
// The directory's records are a chain of variable-length records, walked with the phases of plan_common.h ("The container plan")
// over the directory's byte range [cd_off, cd_off + cd_size), which starts at any alignment: the tiles are laid over the range from
// cd_off rounded down to 16, so positions are relative to that base and the chain starts at the candidate at cd_off - base.
//   count, scan, emit   plan_count_kernel / plan_emit_kernel<ZipFormat>: candidates are the positions whose bytes are 50 4b 01 02
//   describe            zip_describe_kernel: one lane per candidate reads the record (zip::read_record): its end, or "no record"
//   succ, double, mark  zip_succ_kernel, plan_double_kernel, plan_mark_kernel: what the marking never reaches is a decoy (a signature
//                       inside a name, an extra field, a comment)
//   output              this format's own: an exclusive scan of the marked whole records gives each its entry index
//                       (zip_map_kernel: entry -> candidate), then zip_entry_kernel, one lane per entry, reads the record again and
//                       the local header (zip::make_entry), writes the record and sums n_ok / total_size
// The sums are integer atomics: the result does not depend on their order.
//
// The CRC.  crc_count_kernel / scan / crc_first_kernel: pieces per range and the first piece of each; crc_piece_kernel: one wave per
// piece of CHIP_CRC_PIECE bytes (binary search over the firsts, wave_crc32); crc_fold_kernel: one wave per range folds its pieces.
//
// The decode.  zd_select_kernel validates every selected record and keeps what it validated (later kernels never read the caller's
// records again), a {bytes, deflated} scan lays the output out and numbers the deflate sub-batch, zd_rows_kernel writes out_off and the
// sub-batch; then chip_decode_batch(CHIP_FMT_DEFLATE), zip_copy_kernel (pack_copy.h's kernel with 64-bit lengths) for the stored
// entries, the CRC pass, zd_verdict_kernel.
// Locks: a cache of this file first, then the inflate slot's (chip_decode_batch takes it itself), the order read_ranges.hip has.
#include <new>

#include "chip_internal.h"
#include "launch_slots.h"
#include "pack_copy.h"
#include "plan_common.h"
#include "wave_checksums.h"
#include "zip_plan_core.h"

namespace chip {

namespace {

static_assert(sizeof(chip_zip_entry) == 56 && alignof(chip_zip_entry) == 8, "chip_zip_entry: 56 bytes, no padding");
static_assert(zip::UNIT_IN_MAX == CHIP_GZPLAN_WINDOW, "the limit of a unit's input");

inline dim3 grid256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// ---- the plan -------------------------------------------------------------------------------------------------------------------

struct ZipFormat {
    // candidates of chunk g as a 16-bit mask: the positions whose four bytes, all in front of `len`, are 50 4b 01 02
    static __device__ __forceinline__ uint32_t candidates(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t g)
    {
        if (g >= n_chunks) return 0;
        uint32_t w[5];
        load_chunk(base, (len + 3) & ~(uint64_t)3, g, w);
        uint32_t m = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) m |= (chunk_word(w, k) == zip::SIG_CENTRAL ? 1u : 0u) << k;
        const uint64_t b = g * 16;
        if (b + 20 > len) {  // (the last two chunks) drop what reaches behind len
#pragma unroll
            for (uint32_t k = 0; k < 16; k++)
                if (b + k + 4 > len) m &= ~(1u << k);
        }
        return m;
    }
};

// what the plan's kernels hand to the host (device memory, zeroed per call, copied back three times).  It starts with a PlanSummary:
// plan_emit_kernel reports a fault there.
struct PlanDev : PlanSummary {
    uint64_t chain;  // total of the output scan: the whole records on the chain from cd_off
    uint64_t n_ok, total_size;
    zip::End end;
    uint32_t found, pad2;
};

__global__ __launch_bounds__(1024) void zip_end_kernel(const uint8_t *b, uint64_t len, PlanDev *ds)
{
    __shared__ uint32_t s_best;
    if (threadIdx.x == 0) s_best = 0;
    __syncthreads();
    const uint64_t from = zip::end_search_from(len), last = len - zip::END_BYTES;  // len >= 22
    for (uint64_t p = from + threadIdx.x; p <= last; p += 1024)
        if (zip::end_record_at(b, len, p)) atomicMax(&s_best, (uint32_t)(p - from) + 1u);
    __syncthreads();
    if (threadIdx.x == 0 && s_best) {
        ds->found = 1;
        ds->end = zip::read_end(b, from + (s_best - 1u));
    }
}

// per candidate: the end of its record (relative, as pos is) and info = 0 a whole record, 1 where the walk stops.  A position that
// is no candidate (the data changed under the kernels) is a fault.
__global__ __launch_bounds__(256) void zip_describe_kernel(const uint8_t *b, uint64_t abase, uint64_t cd_off, uint64_t cd_end, const uint64_t *pos,
                                                           uint32_t n_cand, uint64_t *end, uint32_t *info, PlanDev *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    const uint64_t rel = pos[i], q = abase + rel;
    zip::Record r;
    bool whole = false;
    if (rel > cd_end - abase || cd_end - q < 4 || zip::le32(b, q) != zip::SIG_CENTRAL) ds->fault = 1;
    else whole = zip::read_record(b, cd_off, cd_end, q, r);
    end[i] = whole ? rel + r.rec_len : 0;
    info[i] = whole ? 0u : 1u;
}

__global__ __launch_bounds__(256) void zip_succ_kernel(const uint64_t *pos, const uint64_t *end, const uint32_t *info, uint32_t n_cand, uint64_t start,
                                                       uint32_t *jump, uint32_t *marked)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    jump[i] = info[i] == 0 ? candidate_at(pos, i + 1u, n_cand, end[i]) : n_cand;
    marked[i] = pos[i] == start ? 1u : 0u;
}

__global__ __launch_bounds__(256) void zip_flags_kernel(const uint32_t *info, const uint32_t *marked, uint32_t n_cand, uint64_t *acc)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_cand) acc[i] = (marked[i] && info[i] == 0) ? 1u : 0u;
}

// behind the scan: ent[k] = the candidate that is entry k, for the first n entries
__global__ __launch_bounds__(256) void zip_map_kernel(const uint32_t *info, const uint32_t *marked, const uint64_t *acc, const uint64_t *acc_part,
                                                      uint32_t n_cand, uint64_t n, uint32_t *ent)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand || !marked[i] || info[i] != 0) return;
    const uint64_t k = acc[i] + acc_part[i / SCAN_THREADS];
    if (k < n && k < n_cand) ent[k] = i;
}

// one lane per entry: the record once more, the local header, the output row, the sums
__global__ __launch_bounds__(256) void zip_entry_kernel(const uint8_t *b, uint64_t abase, uint64_t cd_off, uint64_t cd_end, const uint64_t *pos,
                                                        const uint32_t *ent, uint32_t n_cand, uint64_t n, uint64_t max_entries, chip_zip_entry *entries,
                                                        PlanDev *ds)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t chain = ds->chain;
    uint64_t size = 0;
    bool ok = false;
    if (k < n && k < chain) {
        const uint32_t c = ent[k];
        zip::Record r;
        if (c >= n_cand || !zip::read_record(b, cd_off, cd_end, abase + pos[c], r)) {
            ds->fault = 1;
        } else {
            const chip_zip_entry e = zip::make_entry(b, cd_off, abase + pos[c], r);
            if (k < max_entries) entries[k] = e;
            ok = e.status == CHIP_ZIPENT_OK;
            size = ok ? e.size : 0;
        }
    }
    const uint64_t wave_size = wave_incl_scan_t(size);
    const uint32_t wave_ok = (uint32_t)__popcll(__ballot(ok));
    if (lane_id() == 63 && wave_ok) {
        atomicAdd((unsigned long long *)&ds->n_ok, (unsigned long long)wave_ok);
        atomicAdd((unsigned long long *)&ds->total_size, (unsigned long long)wave_size);
    }
}

using ZipPlanSlot = SummarySlot<PlanDev>;
SlotCache<ZipPlanSlot> g_zip_plan_cache;

// The plan of base[0 .. len), len >= 22: enqueues everything, waits three times (end record, candidate count, summary).  The caller
// holds the cache's lock.  Buffer 0 holds the tile counts and their scan, buffer 1 the candidate tables.
hipError_t zip_plan_locked(ZipPlanSlot &sl, const uint8_t *base, uint64_t len, uint64_t max_entries, chip_zip_entry *entries, hipStream_t stream,
                           chip_zip_plan_summary &out, bool &too_many)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    PlanDev *ds = sl.d_sum;
    if ((e = hipMemsetAsync(ds, 0, sizeof(PlanDev), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(zip_end_kernel, dim3(1), dim3(1024), 0, stream, base, len, ds);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    if (!sl.h_sum->found) return hipSuccess;  // (out says CHIP_ZIP_NO_EOCD)
    const zip::End end = sl.h_sum->end;
    if (end.eocd_off > len - zip::END_BYTES) return hipErrorUnknown;
    out = chip_zip_plan_summary{0, 0, 0, end.cd_off, end.cd_size, end.eocd_off, 0, end.status, end.zip64};
    if (end.status != CHIP_ZIP_OK || end.n == 0) return hipSuccess;
    if (end.cd_off > end.eocd_off || end.cd_size > end.eocd_off - end.cd_off) return hipErrorUnknown;  // (read_end checked it: the data changed)
    out.status = CHIP_ZIP_BAD_DIRECTORY;  // until the chain holds n records
    if (end.cd_size < zip::CENTRAL_BYTES) return hipSuccess;
    const uint64_t cd_end = end.cd_off + end.cd_size, abase = end.cd_off & ~(uint64_t)15, dlen = cd_end - abase;
    const uint8_t *dbase = base + abase;
    const uint64_t n_chunks = (dlen + 15) / 16, n_tiles = (n_chunks + TILE_CHUNKS - 1) / TILE_CHUNKS;
    if ((e = sl.grow(0, (size_t)(2 * n_tiles + scan_parts(n_tiles)) * 8)) != hipSuccess) return e;
    uint64_t *tile_cnt = (uint64_t *)sl.buf[0], *tile_excl = tile_cnt + n_tiles, *tile_part = tile_excl + n_tiles;
    hipLaunchKernelGGL(plan_count_kernel<ZipFormat>, dim3((uint32_t)n_tiles), dim3(TILE_THREADS), 0, stream, dbase, dlen, n_chunks, tile_cnt);
    enqueue_scan<uint64_t>(tile_cnt, tile_excl, n_tiles, tile_part, &ds->cand, stream);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const uint64_t cand64 = sl.h_sum->cand;
    if (cand64 == 0) return hipSuccess;  // no record at all: the walk stops at entry 0
    if (cand64 > 0x7fffffffull) {
        too_many = true;
        return hipSuccess;
    }
    const uint32_t n_cand = (uint32_t)cand64, levels = jump_levels(n_cand);
    const size_t o_acc = 0, o_part = o_acc + (size_t)n_cand * 8, o_pos = o_part + (size_t)scan_parts(n_cand) * 8, o_end = o_pos + (size_t)n_cand * 8;
    const size_t o_info = up16(o_end + (size_t)n_cand * 8), o_mark = up16(o_info + (size_t)n_cand * 4), o_ent = up16(o_mark + (size_t)n_cand * 4);
    const size_t o_jump = up16(o_ent + (size_t)n_cand * 4), jump_stride = up16((size_t)n_cand * 4);
    if ((e = sl.grow(1, o_jump + jump_stride * levels)) != hipSuccess) return e;
    uint8_t *c = sl.buf[1];
    uint64_t *acc = (uint64_t *)(c + o_acc), *acc_part = (uint64_t *)(c + o_part), *pos = (uint64_t *)(c + o_pos), *rec_end = (uint64_t *)(c + o_end);
    uint32_t *info = (uint32_t *)(c + o_info), *marked = (uint32_t *)(c + o_mark), *ent = (uint32_t *)(c + o_ent);
    auto jump = [&](uint32_t k) { return (uint32_t *)(c + o_jump + jump_stride * k); };
    const dim3 cgrid((n_cand + 255u) / 256u);

    hipLaunchKernelGGL(plan_emit_kernel<ZipFormat>, dim3((uint32_t)n_tiles), dim3(TILE_THREADS), 0, stream, dbase, dlen, n_chunks,
                       (const uint64_t *)tile_cnt, (const uint64_t *)tile_excl, (const uint64_t *)tile_part, pos, n_cand, static_cast<PlanSummary *>(ds));
    hipLaunchKernelGGL(zip_describe_kernel, cgrid, dim3(256), 0, stream, base, abase, end.cd_off, cd_end, (const uint64_t *)pos, n_cand, rec_end, info, ds);
    hipLaunchKernelGGL(zip_succ_kernel, cgrid, dim3(256), 0, stream, (const uint64_t *)pos, (const uint64_t *)rec_end, (const uint32_t *)info, n_cand,
                       end.cd_off - abase, jump(0), marked);
    for (uint32_t k = 0; k + 1 < levels; k++)
        hipLaunchKernelGGL(plan_double_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), jump(k + 1), n_cand);
    for (uint32_t k = levels; k-- > 0;) hipLaunchKernelGGL(plan_mark_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), marked, n_cand);
    hipLaunchKernelGGL(zip_flags_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)info, (const uint32_t *)marked, n_cand, acc);
    enqueue_scan<uint64_t>(acc, acc, n_cand, acc_part, &ds->chain, stream);
    hipLaunchKernelGGL(zip_map_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)info, (const uint32_t *)marked, (const uint64_t *)acc,
                       (const uint64_t *)acc_part, n_cand, end.n, ent);
    const uint64_t lanes = end.n < n_cand ? end.n : n_cand;
    hipLaunchKernelGGL(zip_entry_kernel, grid256(lanes), dim3(256), 0, stream, base, abase, end.cd_off, cd_end, (const uint64_t *)pos,
                       (const uint32_t *)ent, n_cand, end.n, max_entries, entries, ds);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const PlanDev &h = *sl.h_sum;
    if (h.fault || h.chain > n_cand) return hipErrorUnknown;  // the input changed between two passes
    out.n_entries = h.chain < end.n ? h.chain : end.n;
    out.n_ok = h.n_ok, out.total_size = h.total_size;
    if (h.chain >= end.n) out.status = CHIP_ZIP_OK;
    else out.bad_index = h.chain;
    return hipSuccess;
}

// ---- CRC-32 of many ranges ------------------------------------------------------------------------------------------------------

constexpr uint32_t CRC_PIECE_LOG2 = 16;
static_assert((1u << CRC_PIECE_LOG2) == CHIP_CRC_PIECE, "CHIP_CRC_PIECE");
constexpr uint32_t CRC_FOLD_WAVES = 4;

__host__ __device__ __forceinline__ uint64_t crc_pieces(uint64_t len) { return (len >> CRC_PIECE_LOG2) + ((len & (CHIP_CRC_PIECE - 1u)) ? 1u : 0u); }

__global__ __launch_bounds__(256) void crc_count_kernel(const uint64_t *len, uint64_t n, uint64_t *cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) cnt[i] = crc_pieces(len[i]);
}

// behind the scan: first[i] gets its workgroup's offset
__global__ __launch_bounds__(256) void crc_first_kernel(uint64_t *first, const uint64_t *part, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) first[i] += part[i / SCAN_THREADS];
}

// One wave per piece t: the range that holds it is the last one whose first piece is at or in front of t (ranges without pieces at
// t sit in front of it).  A range of one piece is answered here.  Lengths that no longer fit the scan (they changed under the
// kernels) read nothing.
__global__ __launch_bounds__(64) void crc_piece_kernel(const uint8_t *base, const uint64_t *off, const uint64_t *len, const uint64_t *first, uint32_t n,
                                                       const uint64_t *total, uint32_t *pc, uint32_t *crc)
{
    __shared__ uint32_t tab[2048];
    const uint64_t t = blockIdx.x;
    if (t >= rdfirst64(*total)) return;  // (uniform)
    uint32_t u = 0, b = n;  // first[u] <= t, and first[b] > t or b == n
    while (b - u > 1u) {
        const uint32_t mid = u + ((b - u) >> 1);
        if (rdfirst64(first[mid]) <= t) u = mid;
        else b = mid;
    }
    const uint64_t L = rdfirst64(len[u]), np = crc_pieces(L), j = t - rdfirst64(first[u]);
    if (j >= np) return;
    const uint64_t head = L - ((np - 1) << CRC_PIECE_LOG2);  // the first piece's length, 1 .. CHIP_CRC_PIECE
    const uint64_t beg = j ? head + ((j - 1) << CRC_PIECE_LOG2) : 0;
    const uint32_t cnt = j ? CHIP_CRC_PIECE : (uint32_t)head;
    const uint32_t v = wave_crc32((LDS_AS uint32_t *)tab, base + rdfirst64(off[u]) + beg, cnt);
    if (lane_id() == 0) {
        pc[t] = v;
        if (np == 1) crc[u] = v;
    }
}

// One wave per range of more than one piece: crc(A || B) = crc(A) * x^(8 |B|) + crc(B), every piece but the first CHIP_CRC_PIECE
// bytes long.  Lane l folds a run of consecutive pieces, its value is moved over the pieces behind the run and the lanes' values
// are summed.
__global__ __launch_bounds__(64 * CRC_FOLD_WAVES) void crc_fold_kernel(const uint64_t *len, const uint64_t *first, uint64_t n, const uint64_t *total,
                                                                      const uint32_t *pc, uint32_t *crc)
{
    const uint32_t lane = lane_id();
    const uint64_t i = (uint64_t)blockIdx.x * CRC_FOLD_WAVES + rdfirst(threadIdx.x >> 6);
    if (i >= n) return;
    const uint64_t np = crc_pieces(rdfirst64(len[i]));
    if (np == 1) return;  // (uniform) answered by its piece
    if (np == 0) {
        if (lane == 0) crc[i] = 0;
        return;
    }
    const uint64_t f0 = rdfirst64(first[i]), all = rdfirst64(*total);
    if (f0 > all || np > all - f0) return;  // (the lengths changed under the kernels)
    const uint64_t per = (np + 63) >> 6;
    const uint64_t a = lane * per < np ? lane * per : np, b = a + per < np ? a + per : np;
    const uint32_t x_piece = X2N[(3 + CRC_PIECE_LOG2) & 31];  // x^(8 * CHIP_CRC_PIECE)
    uint32_t r = 0;
    for (uint64_t j = a; j < b; j++) r = multmodp(x_piece, r) ^ pc[f0 + j];
    uint32_t shift = 0x80000000u;  // x^0
    uint32_t bit = 3 + CRC_PIECE_LOG2;
    for (uint64_t m = np - b; m; m >>= 1, bit++)
        if (m & 1u) shift = multmodp(X2N[bit & 31], shift);
    r = multmodp(shift, r);
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) r ^= (uint32_t)__shfl_xor((int)r, (int)d, 64);
    if (lane == 0) crc[i] = r;
}

// scratch of n ranges in front of the piece values: first[n], part[scan_parts(n)]
inline size_t crc_range_bytes(uint64_t n) { return up16((size_t)(n + scan_parts(n)) * 8); }

// enqueues the piece counts and their scan: first[i] = the pieces in front of range i, *total (device memory) their number
void crc_enqueue_count(uint64_t n, const uint64_t *len, uint64_t *first, uint64_t *part, uint64_t *total, hipStream_t stream)
{
    hipLaunchKernelGGL(crc_count_kernel, grid256(n), dim3(256), 0, stream, len, n, first);
    enqueue_scan<uint64_t>(first, first, n, part, total, stream);
    hipLaunchKernelGGL(crc_first_kernel, grid256(n), dim3(256), 0, stream, first, (const uint64_t *)part, n);
}

// enqueues the pieces and the fold; `pieces` >= *total, pc has room for that many values
void crc_enqueue_pieces(uint64_t n, const uint8_t *base, const uint64_t *off, const uint64_t *len, const uint64_t *first, const uint64_t *total,
                        uint64_t pieces, uint32_t *pc, uint32_t *crc, hipStream_t stream)
{
    if (pieces) hipLaunchKernelGGL(crc_piece_kernel, dim3((uint32_t)pieces), dim3(64), 0, stream, base, off, len, first, (uint32_t)n, total, pc, crc);
    hipLaunchKernelGGL(crc_fold_kernel, dim3((uint32_t)((n + CRC_FOLD_WAVES - 1) / CRC_FOLD_WAVES)), dim3(64 * CRC_FOLD_WAVES), 0, stream, len, first, n,
                       total, (const uint32_t *)pc, crc);
}

struct CrcDev {
    uint64_t pieces;
};
using CrcSlot = SummarySlot<CrcDev>;
SlotCache<CrcSlot> g_crc_cache;

// a buffer that work still in flight on the stream may read (chip_crc32_batch does not wait at its end) grows behind a wait
hipError_t grow_drained(CrcSlot &sl, uint32_t k, size_t want, hipStream_t stream)
{
    if (sl.cap[k] >= want) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(stream);
    return e != hipSuccess ? e : sl.grow(k, want);
}

hipError_t crc_locked(CrcSlot &sl, uint64_t n, const uint8_t *base, const uint64_t *off, const uint64_t *len, uint32_t *crc, hipStream_t stream,
                      bool &too_many)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    if ((e = grow_drained(sl, 0, crc_range_bytes(n), stream)) != hipSuccess) return e;
    uint64_t *first = (uint64_t *)sl.buf[0], *part = first + n;
    crc_enqueue_count(n, len, first, part, &sl.d_sum->pieces, stream);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const uint64_t pieces = sl.h_sum->pieces;
    if (pieces > 0x7fffffffull) {
        too_many = true;
        return hipSuccess;
    }
    if ((e = grow_drained(sl, 1, (size_t)pieces * 4 + 16, stream)) != hipSuccess) return e;
    crc_enqueue_pieces(n, base, off, len, first, &sl.d_sum->pieces, pieces, (uint32_t *)sl.buf[1], crc, stream);
    return hipGetLastError();
}

// ---- the decode -----------------------------------------------------------------------------------------------------------------

struct SelAcc {
    uint64_t bytes, defl;  // decoded sizes of the entries that take part, and how many of them are deflated
};
__host__ __device__ __forceinline__ SelAcc operator+(const SelAcc &a, const SelAcc &b) { return SelAcc{a.bytes + b.bytes, a.defl + b.defl}; }
__device__ __forceinline__ SelAcc shfl_up_t(const SelAcc &a, uint32_t d) { return SelAcc{shfl_up_t(a.bytes, d), shfl_up_t(a.defl, d)}; }

constexpr uint32_t KIND_NONE = 0, KIND_STORED = 1, KIND_DEFLATE = 2;

// what the decode's kernels hand to the host (device memory, zeroed per call, copied back twice)
struct DecDev {
    SelAcc sel;           // total of the selection scan: total_out, deflated entries
    uint64_t crc_pieces;  // total of the CRC pass's scan
    uint64_t n_ok, n_bad;
    uint64_t bad_key;  // ~(the lowest k that is not CHIP_FINISHED), 0: none
};

// the per-entry arrays in buffer 0 (what zd_select_kernel validated, the layout, the sub-batch, the CRC pass)
struct DecArrays {
    SelAcc *acc, *acc_part;
    uint64_t *size, *src_off, *stored_len, *dst_off, *crc_first, *crc_part, *d_in_off, *d_out_off;
    uint32_t *comp, *want_crc, *got_crc, *kind, *d_in_len, *d_out_cap, *d_out_len, *d_in_used;
    int32_t *pre, *d_status;
    size_t bytes;
};
DecArrays carve_decode(uint8_t *b, uint64_t n)
{
    size_t at = 0;
    auto take = [&](uint64_t count, size_t each) {
        uint8_t *p = b + at;
        at = up16(at + (size_t)count * each);
        return p;
    };
    DecArrays a{};
    a.acc = (SelAcc *)take(n, sizeof(SelAcc)), a.acc_part = (SelAcc *)take(scan_parts(n), sizeof(SelAcc));
    a.size = (uint64_t *)take(n, 8), a.src_off = (uint64_t *)take(n, 8), a.stored_len = (uint64_t *)take(n, 8), a.dst_off = (uint64_t *)take(n, 8);
    a.crc_first = (uint64_t *)take(n, 8), a.crc_part = (uint64_t *)take(scan_parts(n), 8);
    a.d_in_off = (uint64_t *)take(n, 8), a.d_out_off = (uint64_t *)take(n, 8);
    a.comp = (uint32_t *)take(n, 4), a.want_crc = (uint32_t *)take(n, 4), a.got_crc = (uint32_t *)take(n, 4), a.kind = (uint32_t *)take(n, 4);
    a.d_in_len = (uint32_t *)take(n, 4), a.d_out_cap = (uint32_t *)take(n, 4), a.d_out_len = (uint32_t *)take(n, 4);
    a.d_in_used = (uint32_t *)take(n, 4);
    a.pre = (int32_t *)take(n, 4), a.d_status = (int32_t *)take(n, 4);
    a.bytes = at;
    return a;
}

// one lane per selected entry: the record is read once, checked against `len`, and what passed is kept
__global__ __launch_bounds__(256) void zd_select_kernel(const chip_zip_entry *entries, uint64_t n_entries, const uint32_t *sel, uint64_t n_sel,
                                                        uint64_t len, DecArrays a)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_sel) return;
    const uint64_t idx = sel ? sel[k] : k;
    int32_t st = CHIP_ZIPENT_BAD_INDEX;
    uint64_t size = 0, data = 0, comp = 0;
    uint32_t kind = KIND_NONE, crc = 0;
    if (idx < n_entries) {
        const chip_zip_entry e = entries[idx];
        st = e.status;
        if (st == CHIP_ZIPENT_OK) {
            const bool in_range = e.data_off <= len && e.comp_size <= len - e.data_off;
            if (in_range && e.method == 0 && e.comp_size == e.size) kind = KIND_STORED;
            else if (in_range && e.method == 8 && e.comp_size <= zip::UNIT_IN_MAX && e.size <= zip::UNIT_OUT_MAX) kind = KIND_DEFLATE;
            else st = CHIP_ZIPENT_BAD_LOCAL;
            if (kind != KIND_NONE) size = e.size, data = e.data_off, comp = e.comp_size, crc = e.crc32;
        }
    }
    a.pre[k] = st;
    a.kind[k] = kind;
    a.size[k] = size;
    a.src_off[k] = data;
    a.comp[k] = (uint32_t)comp;  // (a deflated entry's: at most 2^29 - 64)
    a.stored_len[k] = kind == KIND_STORED ? size : 0;
    a.want_crc[k] = crc;
    a.acc[k] = SelAcc{size, kind == KIND_DEFLATE ? 1u : 0u};
}

// behind the scan: the layout, the caller's out_off, the verdict so far, the rows of the deflate sub-batch
__global__ __launch_bounds__(256) void zd_rows_kernel(uint64_t n_sel, DecArrays a, uint64_t *out_off, int32_t *status)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_sel) return;
    const SelAcc e = a.acc[k] + a.acc_part[k / SCAN_THREADS];
    a.acc[k] = e;
    a.dst_off[k] = e.bytes;
    out_off[k] = e.bytes;
    status[k] = a.kind[k] != KIND_NONE ? (int32_t)CHIP_NEED_OUTPUT : a.pre[k];  // (zd_verdict_kernel answers those that take part)
    if (a.kind[k] != KIND_DEFLATE || e.defl >= n_sel) return;
    a.d_in_off[e.defl] = a.src_off[k];
    a.d_in_len[e.defl] = a.comp[k];
    a.d_out_off[e.defl] = e.bytes;
    a.d_out_cap[e.defl] = (uint32_t)a.size[k];
}

// pack_copy_kernel (pack_copy.h) with 64-bit lengths: a stored entry may be longer than 2^32.  The units are all selected
// entries in order, dst_off ascending; those that are not stored have the length 0, so their bytes are nobody's here.
__global__ __launch_bounds__(64 * PACK_WAVES) void zip_copy_kernel(const uint8_t *src_base, uint64_t src_len_all, const uint64_t *src_off,
                                                                   const uint64_t *src_len, uint8_t *dst_base, const uint64_t *__restrict__ dst_off,
                                                                   uint32_t n, uint64_t total)
{
    const uint32_t lane = lane_id();
    const uint64_t t = (uint64_t)blockIdx.x * PACK_WAVES + rdfirst(threadIdx.x >> 6);
    const uint32_t mis = (uint32_t)((uintptr_t)dst_base & 15u);
    const uint64_t lo = t ? t * PACK_TILE - mis : 0;
    uint64_t hi = (t + 1) * PACK_TILE - mis;
    hi = hi < total ? hi : total;
    if (lo >= total) return;  // (uniform) the last workgroup's spare waves
    uint32_t u = 0, b = n;    // dst_off[u] <= lo, and dst_off[b] > lo or b == n
    while (b - u > 1u) {
        const uint32_t mid = u + ((b - u) >> 1);
        if (rdfirst64(dst_off[mid]) <= lo) u = mid;
        else b = mid;
    }
    for (uint64_t first = u;; first += 64u) {
        const uint64_t uj = first + lane;
        uint64_t d_v = ~0ull, so_v = 0, len_v = 0;
        if (uj < n) d_v = dst_off[uj], so_v = src_off[uj], len_v = src_len[uj];
        const uint32_t here = (uint32_t)__popcll(__ballot(d_v < hi));  // (the offsets ascend: a prefix of the lanes)
        for (uint32_t j = 0; j < here; j++) {
            const uint64_t d = ((uint64_t)rdlane((uint32_t)(d_v >> 32), j) << 32) | rdlane((uint32_t)d_v, j);
            const uint64_t so = ((uint64_t)rdlane((uint32_t)(so_v >> 32), j) << 32) | rdlane((uint32_t)so_v, j);
            const uint64_t ln = ((uint64_t)rdlane((uint32_t)(len_v >> 32), j) << 32) | rdlane((uint32_t)len_v, j);
            const uint64_t s = d > lo ? d : lo, end = d + ln, e = end < hi ? end : hi;
            // (so + ln <= src_len_all: zd_select_kernel checked it; once more, the scratch is all this kernel trusts)
            if (e > s && so <= src_len_all && ln <= src_len_all - so) copy_span(src_base + so + (s - d), dst_base + s, (uint32_t)(e - s), lane);
        }
        if (here < 64u) break;
    }
}

// behind the decode and the CRC pass: the verdict of every entry that took part, and the counts
__global__ __launch_bounds__(256) void zd_verdict_kernel(uint64_t n_sel, DecArrays a, uint64_t n_defl, int32_t *status, DecDev *ds)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool good = false, bad = false;
    if (k < n_sel) {
        int32_t st = a.pre[k];
        const uint32_t kind = a.kind[k];
        if (kind != KIND_NONE) {
            st = CHIP_FINISHED;
            if (kind == KIND_DEFLATE) {
                const uint64_t j = a.acc[k].defl;
                if (j >= n_defl) st = CHIP_ZIPENT_BAD_SIZE;  // (cannot be: the scan numbered them)
                else if (a.d_status[j] != CHIP_FINISHED) st = a.d_status[j];
                else if (a.d_out_len[j] != (uint32_t)a.size[k]) st = CHIP_ZIPENT_BAD_SIZE;
            }
            if (st == CHIP_FINISHED && a.got_crc[k] != a.want_crc[k]) st = CHIP_ZIPENT_BAD_CRC;
            status[k] = st;
        }
        good = st == CHIP_FINISHED && kind != KIND_NONE;
        bad = !good;
        if (bad) atomicMax((unsigned long long *)&ds->bad_key, (unsigned long long)~k);
    }
    const uint32_t n_good = (uint32_t)__popcll(__ballot(good)), n_badw = (uint32_t)__popcll(__ballot(bad));
    if (lane_id() == 0) {
        if (n_good) atomicAdd((unsigned long long *)&ds->n_ok, (unsigned long long)n_good);
        if (n_badw) atomicAdd((unsigned long long *)&ds->n_bad, (unsigned long long)n_badw);
    }
}

using ZipDecSlot = SummarySlot<DecDev>;
SlotCache<ZipDecSlot> g_zip_dec_cache;

// One decode: enqueues everything, waits twice (the sizes, the end).  The caller holds the cache's lock.  Buffer 0 holds the
// per-entry arrays, buffer 1 the CRC pass's piece values.
hipError_t zip_decode_locked(ZipDecSlot &sl, const uint8_t *in_base, uint64_t len, const chip_zip_entry *entries, uint64_t n_entries, uint64_t n_sel,
                             const uint32_t *sel, uint8_t *out_base, uint64_t out_cap, uint64_t *out_off, int32_t *status,
                             chip_zip_decode_summary *summary, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    if ((e = sl.grow(0, carve_decode(nullptr, n_sel).bytes)) != hipSuccess) return e;
    const DecArrays a = carve_decode(sl.buf[0], n_sel);
    DecDev *ds = sl.d_sum;
    if ((e = hipMemsetAsync(ds, 0, sizeof(DecDev), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(zd_select_kernel, grid256(n_sel), dim3(256), 0, stream, entries, n_entries, sel, n_sel, len, a);
    enqueue_scan<SelAcc>(a.acc, a.acc, n_sel, a.acc_part, &ds->sel, stream);
    hipLaunchKernelGGL(zd_rows_kernel, grid256(n_sel), dim3(256), 0, stream, n_sel, a, out_off, status);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const uint64_t total = sl.h_sum->sel.bytes, n_defl = sl.h_sum->sel.defl;
    summary->total_out = total;
    if (total > out_cap) {
        summary->status = CHIP_READ_NEED_OUTPUT;
        return hipSuccess;
    }
    if (n_defl > n_sel) return hipErrorUnknown;
    const uint64_t pieces = (total >> CRC_PIECE_LOG2) + n_sel;  // every entry's pieces, rounded up per entry
    if (pieces > 0x7fffffffull) return hipErrorOutOfMemory;
    if ((e = sl.grow(1, (size_t)pieces * 4 + 16)) != hipSuccess) return e;
    if (n_defl) {
        const int rc = chip_decode_batch(CHIP_FMT_DEFLATE, (size_t)n_defl, in_base, a.d_in_off, a.d_in_len, out_base, a.d_out_off, a.d_out_cap,
                                         a.d_out_len, a.d_in_used, a.d_status, stream);
        if (rc != CHIP_OK) return rc == CHIP_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;
    }
    if (total) {
        const uint64_t tiles = (total + ((uintptr_t)out_base & 15u) + PACK_TILE - 1) / PACK_TILE;
        hipLaunchKernelGGL(zip_copy_kernel, dim3((uint32_t)((tiles + PACK_WAVES - 1) / PACK_WAVES)), dim3(64 * PACK_WAVES), 0, stream, in_base, len,
                           (const uint64_t *)a.src_off, (const uint64_t *)a.stored_len, out_base, (const uint64_t *)a.dst_off, (uint32_t)n_sel, total);
    }
    crc_enqueue_count(n_sel, a.size, a.crc_first, a.crc_part, &ds->crc_pieces, stream);
    crc_enqueue_pieces(n_sel, out_base, a.dst_off, a.size, a.crc_first, &ds->crc_pieces, total ? pieces : 0, (uint32_t *)sl.buf[1], a.got_crc, stream);
    hipLaunchKernelGGL(zd_verdict_kernel, grid256(n_sel), dim3(256), 0, stream, n_sel, a, n_defl, status, ds);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const DecDev &h = *sl.h_sum;
    summary->n_ok = h.n_ok, summary->n_bad = h.n_bad;
    summary->first_bad = h.n_bad ? ~h.bad_key : 0;
    return hipSuccess;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_zip_plan_host(const uint8_t *in, uint64_t len, uint64_t max_entries, chip_zip_entry *entries, chip_zip_plan_summary *summary)
{
    if (!summary || (len && !in) || (max_entries && !entries) || len > ((uint64_t)1 << 40)) return CHIP_E_INVALID;
    zip::plan_host(in, len, max_entries, entries, summary);
    return CHIP_OK;
}

int chip_zip_plan(const void *in_base, uint64_t len, uint64_t max_entries, chip_zip_entry *entries, chip_zip_plan_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_entries && !entries) || ((uintptr_t)in_base & 3u) || len > ((uint64_t)1 << 40)) return CHIP_E_INVALID;
    constexpr chip_zip_plan_summary NOTHING{0, 0, 0, 0, 0, 0, 0, CHIP_ZIP_NO_EOCD, 0};
    *summary = NOTHING;
    if (len < zip::END_BYTES) return CHIP_OK;
    chip_zip_plan_summary r = NOTHING;
    bool too_many = false;
    const int rc = with_slot(
        g_zip_plan_cache, stream,
        [&](ZipPlanSlot &sl, hipStream_t s) { return zip_plan_locked(sl, (const uint8_t *)in_base, len, max_entries, entries, s, r, too_many); },
        [&] { *summary = NOTHING; });
    if (rc != CHIP_OK) return rc;
    if (too_many) return CHIP_E_NOMEM;
    *summary = r;
    return CHIP_OK;
}

int chip_crc32_batch(size_t n, const void *base, const uint64_t *off, const uint64_t *len, uint32_t *crc, void *stream)
{
    if ((uint64_t)n > 0xFFFFFFFFull || (n && (!base || !off || !len || !crc))) return CHIP_E_INVALID;
    if (n == 0) return CHIP_OK;
    bool too_many = false;
    const int rc = with_slot(
        g_crc_cache, stream, [&](CrcSlot &sl, hipStream_t s) { return crc_locked(sl, n, (const uint8_t *)base, off, len, crc, s, too_many); }, [] {});
    if (rc != CHIP_OK) return rc;
    return too_many ? CHIP_E_NOMEM : CHIP_OK;
}

int chip_zip_decode(const void *in_base, uint64_t len, const chip_zip_entry *entries, uint64_t n_entries, uint64_t n_sel, const uint32_t *sel,
                    void *out_base, uint64_t out_cap, uint64_t *out_off, int32_t *status, chip_zip_decode_summary *summary, void *stream)
{
    if (!summary || (len && !in_base) || ((uintptr_t)in_base & 3u) || len > ((uint64_t)1 << 40) || (n_entries && !entries) ||
        (n_sel && (!out_off || !status)) || (out_cap && !out_base) || n_entries > 0x7fffffffull || n_sel > 0x7fffffffull)
        return CHIP_E_INVALID;
    *summary = chip_zip_decode_summary{0, 0, 0, 0, 0, CHIP_READ_OK, 0};
    if (n_sel == 0) return CHIP_OK;
    chip_zip_decode_summary r{n_sel, 0, 0, 0, 0, CHIP_READ_OK, 0};
    const int rc = with_slot(
        g_zip_dec_cache, stream,
        [&](ZipDecSlot &sl, hipStream_t s) {
            return zip_decode_locked(sl, (const uint8_t *)in_base, len, entries, n_entries, n_sel, sel, (uint8_t *)out_base, out_cap, out_off, status, &r,
                                     s);
        },
        [] {});
    if (rc != CHIP_OK) return rc;
    *summary = r;
    return CHIP_OK;
}

}  // extern "C"
