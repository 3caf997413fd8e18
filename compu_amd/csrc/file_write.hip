// The write side of the container formats: chip_pack_units lays ranges of device memory end to end, chip_encode_file cuts a buffer
// into units, encodes them with the batch encoder, packs the results and appends the format's trailer (htslib's EOF block, the
// seek table of zstd's seekable format).  DESIGN.md sec. 4.13.  CHIP_FMT_LZ4 is ONE frame with a block per unit and has passes of
// its own, further down.
//
//   1. widen    the 32-bit lengths become 64-bit sums-to-be (chip_encode_file: a unit that is not CHIP_ENC_FINISHED is counted)
//   2. scan     exclusive 64-bit scan (plan_common.h), the total goes to the summary
//      -- the host reads the total and compares it with the room --
//   3. copy     destination-driven, one wave per PACK_TILE bytes of destination: pack_copy.h, shared with read_ranges.hip
//   4. trailer  (chip_encode_file) 28 bytes of EOF block, or 17 + 8n bytes of seek table from the device arrays
// Order between the phases comes from kernel boundaries on the stream only.  The copy writes dst[0 .. total) only, whatever the
// arrays hold by then: every store is clipped to its tile, and the tiles end at the total the host compared with the room.
#include <string.h>

#include "chip_internal.h"
#include "launch_slots.h"
#include "lz4_enc_core.h"
#include "pack_copy.h"
#include "plan_common.h"

namespace chip {

namespace {

// what the kernels hand to the host (device memory, copied back once the scan is done)
struct DevSummary {
    uint64_t total;  // sum of all lengths
    uint32_t bad;    // chip_encode_file: units whose status is not CHIP_ENC_FINISHED
    uint32_t pad;
};

__global__ __launch_bounds__(256) void pack_widen_kernel(const uint32_t *len, const int32_t *status, uint64_t n, uint64_t *wide, DevSummary *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    wide[i] = len[i];
    if (status && status[i] != CHIP_ENC_FINISHED) atomicAdd(&ds->bad, 1u);  // (never, with slots of chip_encode_bound bytes)
}

// behind the two scan kernels: off[i] gets its workgroup's offset; the caller's array, if there is one, a copy
__global__ __launch_bounds__(256) void pack_offsets_kernel(uint64_t *off, const uint64_t *part, uint64_t n, uint64_t *user_off)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = off[i] + part[i / SCAN_THREADS];
    off[i] = o;
    if (user_off) user_off[i] = o;
}

// chip_encode_file: the arrays of the encode batch, unit i = [i * unit, min(len, (i + 1) * unit)) into slot i
__global__ __launch_bounds__(256) void file_units_kernel(uint64_t *in_off, uint32_t *in_len, uint64_t *out_off, uint32_t *out_cap, uint32_t n,
                                                         uint32_t unit, uint64_t len, uint32_t slot)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = (uint64_t)i * unit, left = len - at;  // (len == 0: the one unit of empty content)
    in_off[i] = at;
    in_len[i] = left < unit ? (uint32_t)left : unit;
    out_off[i] = (uint64_t)i * slot;
    out_cap[i] = slot;
}

struct EofWords {
    uint32_t w[7];  // htslib's EOF block
};

__global__ __launch_bounds__(64) void file_eof_kernel(uint8_t *at, EofWords eof)
{
    const uint32_t lane = threadIdx.x;
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 7; k++) w = (lane >> 2) == k ? eof.w[k] : w;
    if (lane < 28) at[lane] = (uint8_t)(w >> (8 * (lane & 3u)));
}

__device__ __forceinline__ void put_le32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

// the seek table of zstd's seekable format (contrib/seekable_format, no per-frame checksums) at `at`, any alignment: 17 + 8n bytes
__global__ __launch_bounds__(256) void file_seek_table_kernel(uint8_t *at, const uint32_t *c_len, const uint32_t *d_len, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (i == 0) {
        put_le32(at, 0x184D2A5Eu);
        put_le32(at + 4, 8u * n + 9u);
    }
    uint8_t *e = at + 8 + 8ull * i;
    put_le32(e, c_len[i]);
    put_le32(e + 4, d_len[i]);
    if (i == n - 1u) {
        put_le32(e + 8, n);
        e[12] = 0;  // Seek_Table_Descriptor: no checksums
        put_le32(e + 13, 0x8F92EAB1u);
    }
}

// The scratch of one (device, stream): buffer 0 the per-unit arrays with the scan's partials behind them, buffer 1
// chip_encode_file's slot area.  A launch slot.
using FileSlot = SummarySlot<DevSummary>;
constexpr uint32_t ARRAYS = 0, AREA = 1;
SlotCache<FileSlot> g_file_cache;

// lengths -> offsets in `off` (n entries, `part` behind them) and the caller's array; waits for the total
hipError_t offsets_locked(FileSlot &sl, uint64_t n, const uint32_t *len, const int32_t *status, uint64_t *off, uint64_t *part, uint64_t *user_off,
                          hipStream_t stream)
{
    const dim3 grid((uint32_t)((n + 255) / 256));
    const hipError_t e = hipMemsetAsync(sl.d_sum, 0, sizeof(DevSummary), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pack_widen_kernel, grid, dim3(256), 0, stream, len, status, n, off, sl.d_sum);
    enqueue_scan<uint64_t>(off, off, n, part, &sl.d_sum->total, stream);
    hipLaunchKernelGGL(pack_offsets_kernel, grid, dim3(256), 0, stream, off, (const uint64_t *)part, n, user_off);
    return sl.fetch(stream);
}

hipError_t pack_locked(FileSlot &sl, uint64_t n, const uint8_t *src_base, const uint64_t *src_off, const uint32_t *src_len, uint8_t *dst_base,
                       uint64_t dst_cap, uint64_t *dst_off, uint64_t *total, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    if ((e = sl.grow(ARRAYS, (size_t)(n + scan_parts(n)) * 8)) != hipSuccess) return e;
    uint64_t *off = (uint64_t *)sl.buf[ARRAYS], *part = off + n;
    if ((e = offsets_locked(sl, n, src_len, nullptr, off, part, dst_off, stream)) != hipSuccess) return e;
    *total = sl.h_sum->total;
    if (*total == 0 || *total > dst_cap) return hipSuccess;
    enqueue_copy(n, src_base, src_off, src_len, dst_base, off, *total, stream);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipStreamSynchronize(stream);  // the slot's offsets are read until the copy is done
}

// What chip_encode_file makes of its arguments (all but the level and the pointers): false = CHIP_E_INVALID.
struct FileShape {
    uint32_t unit;     // bytes per unit
    uint64_t n;        // units encoded: ceil(len / unit), one unit of empty content for an empty gzip / zstd input
    uint64_t trailer;  // bytes behind the last unit
};
constexpr uint32_t LZ4_W_FLAGS = CHIP_W_LZ4_CONTENT_CHECKSUM | CHIP_W_LZ4_BLOCK_CHECKSUM;
bool file_shape(int format, uint32_t unit_bytes, uint32_t flags, uint64_t len, FileShape &s)
{
    if (format == CHIP_FMT_LZ4) {  // ONE frame: a block per unit; unit_bytes is one of the format's block maxima
        s.unit = unit_bytes ? unit_bytes : 65536u;
        if (s.unit != 65536u && s.unit != 262144u && s.unit != 1048576u && s.unit != 4194304u) return false;
        if ((flags & ~LZ4_W_FLAGS) || len > ((uint64_t)1 << 40)) return false;
        s.n = (len + s.unit - 1) / s.unit;  // (at most 2^24)
        s.trailer = 4u + ((flags & CHIP_W_LZ4_CONTENT_CHECKSUM) ? 4u : 0u);
        return true;
    }
    if (format != CHIP_FMT_BGZF && format != CHIP_FMT_GZIP && format != CHIP_FMT_ZSTD) return false;
    if ((flags & ~(uint32_t)CHIP_W_SEEK_TABLE) || (flags && format != CHIP_FMT_ZSTD)) return false;
    const bool bgzf = format == CHIP_FMT_BGZF;
    s.unit = unit_bytes ? unit_bytes : bgzf ? 65280u : 262144u;
    if (s.unit > (bgzf ? 65280u : 0x40000000u) || len > ((uint64_t)1 << 40)) return false;
    s.n = (len + s.unit - 1) / s.unit;
    if (s.n == 0 && !bgzf) s.n = 1;
    if (s.n > 0x7fffffffull || (flags && s.n > 0x8000000ull)) return false;
    s.trailer = bgzf ? 28 : flags ? 17 + 8 * s.n : 0;
    return true;
}

bool level_ok(int format, int level)
{
    if (format == CHIP_FMT_LZ4) return level >= -1 && level <= 12;
    return format == CHIP_FMT_ZSTD ? level >= -131072 && level <= 131072 : level >= -1 && level <= 9;
}

// Enqueues everything, waits twice (total, end).  The caller holds the cache's lock.
hipError_t encode_file_locked(FileSlot &sl, int format, int level, const FileShape &s, uint32_t flags, const uint8_t *in_base, uint64_t len,
                              uint8_t *out_base, uint64_t out_cap, chip_file_summary *summary, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    const uint32_t n = (uint32_t)s.n;
    const size_t slot = up16(chip_encode_bound(format, s.unit));
    uint64_t total = 0;
    // in_off (the packed offsets once the encode is done) | out_off | in_len | out_cap | out_len | status | partials
    if ((e = sl.grow(ARRAYS, (size_t)n * 32 + (size_t)scan_parts(n) * 8)) != hipSuccess) return e;
    if ((e = sl.grow(AREA, (size_t)n * slot)) != hipSuccess) return e;
    uint8_t *area = sl.buf[AREA];
    uint64_t *in_off = (uint64_t *)sl.buf[ARRAYS], *out_off = in_off + n;
    uint32_t *in_len = (uint32_t *)(out_off + n), *cap = in_len + n, *out_len = cap + n;
    int32_t *status = (int32_t *)(out_len + n);
    uint64_t *part = (uint64_t *)(status + n);
    if (n) {  // (an empty BGZF file has no unit)
        hipLaunchKernelGGL(file_units_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, in_off, in_len, out_off, cap, n, s.unit, len, (uint32_t)slot);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // (an empty input has no buffer: the one unit of length 0 reads nothing, the batch call wants a pointer)
        if (chip_encode_batch(format, level, n, in_base ? in_base : area, in_off, in_len, area, out_off, cap, out_len, status, stream) != CHIP_OK)
            return hipErrorUnknown;  // (the encoder failed: CHIP_E_LAUNCH)
        if ((e = offsets_locked(sl, n, out_len, status, in_off, part, nullptr, stream)) != hipSuccess) return e;
        if (sl.h_sum->bad) return hipErrorUnknown;  // (a unit did not end CHIP_ENC_FINISHED: CHIP_E_LAUNCH)
        total = sl.h_sum->total;
    }
    summary->n_units = n;
    summary->table_off = flags ? total : total + s.trailer;
    summary->out_len = total + s.trailer;
    summary->status = summary->out_len > out_cap ? CHIP_FILE_NEED_OUTPUT : CHIP_FILE_OK;
    if (summary->status != CHIP_FILE_OK) return hipSuccess;
    if (total) enqueue_copy(n, area, out_off, out_len, out_base, in_off, total, stream);
    if (format == CHIP_FMT_BGZF) {
        EofWords eof;
        memcpy(eof.w, chip_bgzf_eof_block(nullptr), sizeof(eof.w));
        hipLaunchKernelGGL(file_eof_kernel, dim3(1), dim3(64), 0, stream, out_base + total, eof);
    } else if (flags) {
        hipLaunchKernelGGL(file_seek_table_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, out_base + total, (const uint32_t *)out_len,
                           (const uint32_t *)in_len, n);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipStreamSynchronize(stream);  // the slot is handed on only with nothing in flight
}

// ---- chip_encode_file(CHIP_FMT_LZ4): ONE frame, a block per unit ------------------------------------------------------------------
//   1. units    file_units_kernel, 2. encode: a CHIP_FMT_LZ4_BLOCK batch into the slots
//   3. decide   out_len >= in_len: the block is stored; its bytes in the file, its piece (header + bytes + checksum) to the scan
//   4. scan     the layout; the host reads the total and compares it with the room
//   5. copy     destination-driven as pack_copy.h's, each block from its slot or from the input (a selector per unit)
//   6. hash     chip_xxh32_batch over every block's bytes as they lie in the file (block checksums only)
//   7. marks    block headers and checksums, the frame header, the end mark, the content checksum (one wave over the input:
//               XXH32 is one serial chain, which is why CHIP_W_LZ4_CONTENT_CHECKSUM is off by default)
struct Lz4FileArrays {
    uint64_t *in_off, *out_off, *foff, *part;
    uint32_t *in_len, *cap, *out_len, *dlen, *stored, *digest, *check;
    int32_t *status;
    static size_t bytes(uint64_t n) { return (size_t)n * 52 + (size_t)scan_parts(n) * 8 + 64; }
    Lz4FileArrays(uint8_t *b, uint64_t n)
    {
        in_off = (uint64_t *)b;
        out_off = in_off + n;
        foff = out_off + n;
        part = foff + n;
        in_len = (uint32_t *)(part + scan_parts(n));
        cap = in_len + n;
        out_len = cap + n;
        dlen = out_len + n;
        stored = dlen + n;
        digest = stored + n;
        status = (int32_t *)(digest + n);
        check = (uint32_t *)(status + n);
    }
};

__global__ __launch_bounds__(256) void lz4w_decide_kernel(Lz4FileArrays a, uint32_t n, uint32_t extra, DevSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (a.status[i] != CHIP_ENC_FINISHED) atomicAdd(&ds->bad, 1u);  // (never, with slots of chip_encode_bound bytes)
    const uint32_t st = a.out_len[i] >= a.in_len[i] ? 1u : 0u;
    a.stored[i] = st;
    a.dlen[i] = st ? a.in_len[i] : a.out_len[i];
    a.foff[i] = 4ull + a.dlen[i] + extra;
}

// behind the scan: foff[i] becomes the file offset of block i's bytes (behind the frame header and the block's own header)
__global__ __launch_bounds__(256) void lz4w_offsets_kernel(uint64_t *foff, const uint64_t *part, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    foff[i] += part[i / SCAN_THREADS] + lz4enc::FRAME_HEADER + 4u;
}

// pack_copy_kernel with a source per unit: stored[u] picks the input, else the unit's slot.  The offsets ascend; the bytes between
// two blocks (headers, checksums) belong to the marks kernel.
__global__ __launch_bounds__(64 * PACK_WAVES) void lz4w_copy_kernel(const uint8_t *slots, const uint8_t *input, Lz4FileArrays a, uint8_t *dst_base, uint32_t n,
                                                                    uint64_t total)
{
    const uint32_t lane = lane_id();
    const uint64_t t = (uint64_t)blockIdx.x * PACK_WAVES + rdfirst(threadIdx.x >> 6);
    const uint32_t mis = (uint32_t)((uintptr_t)dst_base & 15u);
    const uint64_t lo = t ? t * PACK_TILE - mis : 0;
    uint64_t hi = (t + 1) * PACK_TILE - mis;
    hi = hi < total ? hi : total;
    if (lo >= total) return;  // (uniform) the last workgroup's spare waves
    const uint64_t *__restrict__ dst_off = a.foff;
    uint32_t u = 0, b = n;  // dst_off[u] <= lo (or u == 0), and dst_off[b] > lo or b == n
    while (b - u > 1u) {
        const uint32_t mid = u + ((b - u) >> 1);
        if (rdfirst64(dst_off[mid]) <= lo) u = mid;
        else b = mid;
    }
    for (uint64_t first = u;; first += 64u) {
        const uint64_t uj = first + lane;
        uint64_t d_v = ~0ull, so_v = 0;
        uint32_t len_v = 0, sel_v = 0;
        if (uj < n) {
            d_v = dst_off[uj], len_v = a.dlen[uj], sel_v = a.stored[uj];
            so_v = sel_v ? a.in_off[uj] : a.out_off[uj];
        }
        const uint32_t here = (uint32_t)__popcll(__ballot(d_v < hi));  // (the offsets ascend: a prefix of the lanes)
        for (uint32_t j = 0; j < here; j++) {
            const uint64_t d = ((uint64_t)rdlane((uint32_t)(d_v >> 32), j) << 32) | rdlane((uint32_t)d_v, j);
            const uint64_t so = ((uint64_t)rdlane((uint32_t)(so_v >> 32), j) << 32) | rdlane((uint32_t)so_v, j);
            const uint8_t *base = rdlane(sel_v, j) ? input : slots;
            const uint64_t s = d > lo ? d : lo, end = d + rdlane(len_v, j), e = end < hi ? end : hi;
            if (e > s) copy_span(base + so + (s - d), dst_base + s, (uint32_t)(e - s), lane);
        }
        if (here < 64u) break;
    }
}

struct Lz4FrameHead {
    uint8_t b[lz4enc::FRAME_HEADER];
};

// thread i: block i's header and checksum; thread 0 also the frame header, the end mark at `end` and the content checksum
__global__ __launch_bounds__(256) void lz4w_marks_kernel(uint8_t *out, Lz4FileArrays a, uint32_t n, uint32_t bchk, uint32_t cchk, Lz4FrameHead head, uint64_t end)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) {
        for (uint32_t k = 0; k < lz4enc::FRAME_HEADER; k++) out[k] = head.b[k];
        put_le32(out + end, 0u);
        if (cchk) put_le32(out + end + 4, *a.check);
    }
    if (i >= n) return;
    uint8_t *p = out + a.foff[i];
    put_le32(p - 4, a.dlen[i] | (a.stored[i] << 31));
    if (bchk) put_le32(p + a.dlen[i], a.digest[i]);
}

hipError_t encode_lz4_file_locked(FileSlot &sl, int level, const FileShape &s, uint32_t flags, const uint8_t *in_base, uint64_t len, uint8_t *out_base,
                                  uint64_t out_cap, chip_file_summary *summary, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    const uint32_t n = (uint32_t)s.n;
    const uint32_t bchk = (flags & CHIP_W_LZ4_BLOCK_CHECKSUM) ? 1u : 0u, cchk = (flags & CHIP_W_LZ4_CONTENT_CHECKSUM) ? 1u : 0u;
    const size_t slot = up16(chip_encode_bound(CHIP_FMT_LZ4_BLOCK, s.unit));
    if ((e = sl.grow(ARRAYS, Lz4FileArrays::bytes(n))) != hipSuccess) return e;
    if ((e = sl.grow(AREA, (size_t)n * slot + 16)) != hipSuccess) return e;
    uint8_t *area = sl.buf[AREA];
    const Lz4FileArrays a(sl.buf[ARRAYS], n);
    const dim3 grid((n + 255u) / 256u);
    uint64_t blocks_total = 0;
    if (n) {
        hipLaunchKernelGGL(file_units_kernel, grid, dim3(256), 0, stream, a.in_off, a.in_len, a.out_off, a.cap, n, s.unit, len, (uint32_t)slot);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (chip_encode_batch(CHIP_FMT_LZ4_BLOCK, level, n, in_base, a.in_off, a.in_len, area, a.out_off, a.cap, a.out_len, a.status, stream) != CHIP_OK)
            return hipErrorUnknown;  // (the encoder failed: CHIP_E_LAUNCH)
        if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(DevSummary), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(lz4w_decide_kernel, grid, dim3(256), 0, stream, a, n, 4u * bchk, sl.d_sum);
        enqueue_scan<uint64_t>(a.foff, a.foff, n, a.part, &sl.d_sum->total, stream);
        hipLaunchKernelGGL(lz4w_offsets_kernel, grid, dim3(256), 0, stream, a.foff, (const uint64_t *)a.part, n);
        if ((e = sl.fetch(stream)) != hipSuccess) return e;
        if (sl.h_sum->bad) return hipErrorUnknown;  // (a unit did not end CHIP_ENC_FINISHED: CHIP_E_LAUNCH)
        blocks_total = sl.h_sum->total;
    }
    const uint64_t end = lz4enc::FRAME_HEADER + blocks_total;  // of the last block: where the end mark goes
    summary->n_units = n;
    summary->out_len = end + s.trailer;
    summary->table_off = summary->out_len;
    summary->status = summary->out_len > out_cap ? CHIP_FILE_NEED_OUTPUT : CHIP_FILE_OK;
    if (summary->status != CHIP_FILE_OK) return hipSuccess;
    if (n) {
        const uint64_t tiles = (end + ((uintptr_t)out_base & 15u) + PACK_TILE - 1) / PACK_TILE;
        hipLaunchKernelGGL(lz4w_copy_kernel, dim3((uint32_t)((tiles + PACK_WAVES - 1) / PACK_WAVES)), dim3(64 * PACK_WAVES), 0, stream, (const uint8_t *)area,
                           in_base, a, out_base, n, end);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (bchk && chip_xxh32_batch(n, out_base, a.foff, a.dlen, 0, a.digest, stream) != CHIP_OK) return hipErrorUnknown;
    }
    if (cchk && (e = launch_lz4_xxh(in_base, len, a.check, stream)) != hipSuccess) return e;
    Lz4FrameHead head;
    const uint32_t id = s.unit == 65536u ? 4u : s.unit == 262144u ? 5u : s.unit == 1048576u ? 6u : 7u;
    lz4enc::frame_header(head.b, (id << CHIP_LZ4_S_BLOCK_ID_SHIFT) | (bchk ? CHIP_LZ4_S_BLOCK_CHECKSUM : 0) | (cchk ? 0 : CHIP_LZ4_S_NO_CONTENT_CHECKSUM), len);
    hipLaunchKernelGGL(lz4w_marks_kernel, dim3(n ? grid.x : 1u), dim3(256), 0, stream, out_base, a, n, bchk, cchk, head, end);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipStreamSynchronize(stream);  // the slot is handed on only with nothing in flight
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_pack_units(size_t n, const void *src_base, const uint64_t *src_off, const uint32_t *src_len, void *dst_base, uint64_t dst_cap,
                    uint64_t *dst_off, uint64_t *total, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!total || (n && (!src_base || !src_off || !src_len)) || (dst_cap && !dst_base) || (uint64_t)n > 0xFFFFFFFFull) return CHIP_E_INVALID;
    *total = 0;
    if (n == 0) return CHIP_OK;
    return with_slot(
        g_file_cache, stream,
        [&](FileSlot &sl, hipStream_t s) {
            return pack_locked(sl, n, (const uint8_t *)src_base, src_off, src_len, (uint8_t *)dst_base, dst_cap, dst_off, total, s);
        },
        [&] { *total = 0; });
}

uint64_t chip_encode_file_bound(int format, uint32_t unit_bytes, uint32_t flags, uint64_t len)
{
    FileShape s;
    if (!file_shape(format, unit_bytes, flags, len, s)) return 0;
    // one LZ4 frame: the header, every block stored at worst (a header, its bytes, its checksum), end mark and content checksum
    if (format == CHIP_FMT_LZ4) return lz4enc::FRAME_HEADER + len + s.n * (4u + ((flags & CHIP_W_LZ4_BLOCK_CHECKSUM) ? 4u : 0u)) + s.trailer;
    if (s.n == 0) return s.trailer;
    return (s.n - 1) * chip_encode_bound(format, s.unit) + chip_encode_bound(format, (size_t)(len - (s.n - 1) * s.unit)) + s.trailer;
}

int chip_encode_file(int format, int level, uint32_t unit_bytes, uint32_t flags, const void *in_base, uint64_t len, void *out_base,
                     uint64_t out_cap, chip_file_summary *summary, void *stream)
{
    FileShape s;
    if (!summary || (len && !in_base) || ((uintptr_t)in_base & 3u) || (out_cap && !out_base) || !file_shape(format, unit_bytes, flags, len, s) ||
        !level_ok(format, level))
        return CHIP_E_INVALID;
    *summary = chip_file_summary{0, 0, 0, CHIP_FILE_OK, 0};
    return with_slot(
        g_file_cache, stream,
        [&](FileSlot &sl, hipStream_t st) {
            if (format == CHIP_FMT_LZ4)
                return encode_lz4_file_locked(sl, level, s, flags, (const uint8_t *)in_base, len, (uint8_t *)out_base, out_cap, summary, st);
            return encode_file_locked(sl, format, level, s, flags, (const uint8_t *)in_base, len, (uint8_t *)out_base, out_cap, summary, st);
        },
        [&] { *summary = chip_file_summary{0, 0, 0, CHIP_FILE_OK, 0}; });
}

}  // extern "C"
