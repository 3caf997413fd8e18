// ZIP archives, the write side: chip_zip_assemble[_host], chip_zip_write, chip_zip_write_bound.  The definitions
// are in include/compu_hip.h; the check of a record, the lengths and the bytes of every generated record, which host and device
// share, and the host assembly are in zip_write_core.h.
//
// The assembly, in stream order:
//   1. check    zw_check_kernel, one lane per entry: the record is read once, checked, the method chosen, and what passed is kept
//               (zipw::Kept: later kernels never read the caller's records again); {local part's length, deflated} goes to the scan,
//               a bad record to a 64-bit atomicMax of ~i (the lowest i wins)
//   2. scan     exclusive scan (plan_common.h): header_off of every entry, cd_off and n_deflated as the total
//   3. sizes    zw_sizes_kernel: header_off is final, so zl_i is known and with it the central record's length; second scan: where
//               every record lies in the directory, cd_size as the total
//      -- the host reads both totals and the lowest bad index, adds the end records and compares with the room --
//   4. records  zw_records_kernel, one lane per entry: the 30 + (20) bytes of the local header and the 46 + (0..28) bytes of the
//               central record through zipw::format_*, byte by byte with byte stores (a record starts at any address; a byte store
//               covers its own byte only), entries[i], and the copy's units; zw_end_kernel writes the end records the host formatted
//   5. copies   zw_copy_kernel: zip.hip's destination-driven copy (one wave per PACK_TILE bytes of destination, 64-bit lengths, gaps
//               between the units belong to nobody) with a source selector per unit -- names, content or the encoded streams.  The
//               local area is 2n units (name_i, data_i), the directory n units (name_i).
// With too little room step 4 fills entries[] only and nothing else follows.
// chip_zip_write runs in front of that: zw_prep_kernel (the CRC ranges, the slot of every deflate-eligible entry), a scan,
// zw_units_kernel (the encode batch), chip_crc32_batch, chip_encode_batch, zw_gather_kernel (comp_len per entry).
// Locks: this file's cache first, then the CRC slot's and the encoder's (those calls take them themselves), the order zip.hip has.
#include <stdlib.h>
#include <string.h>

#include "chip_internal.h"
#include "launch_slots.h"
#include "pack_copy.h"
#include "plan_common.h"
#include "zip_write_core.h"

namespace chip {

namespace {

static_assert(sizeof(chip_zip_source) == 32 && alignof(chip_zip_source) == 8, "chip_zip_source: 32 bytes, no padding");
static_assert(sizeof(chip_zip_write_summary) == 64, "chip_zip_write_summary: 64 bytes");
static_assert(sizeof(zipw::Kept) == 48, "zipw::Kept");

inline dim3 grid256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

struct LayAcc {
    uint64_t bytes, defl;  // lengths, and how many of the entries in front are deflated (deflate-eligible, in chip_zip_write's scan)
};
__host__ __device__ __forceinline__ LayAcc operator+(const LayAcc &a, const LayAcc &b) { return LayAcc{a.bytes + b.bytes, a.defl + b.defl}; }
__device__ __forceinline__ LayAcc shfl_up_t(const LayAcc &a, uint32_t d) { return LayAcc{shfl_up_t(a.bytes, d), shfl_up_t(a.defl, d)}; }

// what the kernels hand to the host (device memory, zeroed per call)
struct WriteDev {
    LayAcc lay;        // total of the first scan: cd_off, n_deflated
    uint64_t cd_size;  // total of the second scan
    uint64_t bad_key;  // ~(the lowest bad index), 0: none
    LayAcc slots;      // chip_zip_write: bytes of the slot area, deflate-eligible entries
    uint32_t enc_bad;  // chip_zip_write: units that did not end CHIP_ENC_FINISHED
    uint32_t pad;
};

constexpr uint32_t SRC_NAMES = 0, SRC_CONTENT = 1, SRC_COMP = 2;
struct Sources {
    const uint8_t *base[3];
    uint64_t len[3];
};

// the per-entry arrays in buffer 0
struct Arrays {
    // the assembly
    zipw::Kept *kept;
    LayAcc *acc, *acc_part;
    uint64_t *hoff, *cacc, *cacc_part;
    uint64_t *u_dst, *u_src, *u_len, *c_dst, *c_src, *c_len;  // u_*: 2n units of the local area; c_*: n units of the directory
    uint32_t *u_sel;
    // chip_zip_write
    LayAcc *sacc, *sacc_part;
    uint64_t *crc_off, *crc_len, *comp_off, *e_in_off, *e_out_off;
    uint32_t *crc, *comp_len, *slot, *e_in_len, *e_cap, *e_out_len;
    int32_t *e_status;
    size_t bytes;
};
Arrays carve(uint8_t *b, uint64_t n, bool write)
{
    size_t at = 0;
    auto take = [&](uint64_t count, size_t each) {
        uint8_t *p = b + at;
        at = up16(at + (size_t)count * each);
        return p;
    };
    Arrays a{};
    a.kept = (zipw::Kept *)take(n, sizeof(zipw::Kept));
    a.acc = (LayAcc *)take(n, sizeof(LayAcc)), a.acc_part = (LayAcc *)take(scan_parts(n), sizeof(LayAcc));
    a.hoff = (uint64_t *)take(n, 8), a.cacc = (uint64_t *)take(n, 8), a.cacc_part = (uint64_t *)take(scan_parts(n), 8);
    a.u_dst = (uint64_t *)take(2 * n, 8), a.u_src = (uint64_t *)take(2 * n, 8), a.u_len = (uint64_t *)take(2 * n, 8);
    a.c_dst = (uint64_t *)take(n, 8), a.c_src = (uint64_t *)take(n, 8), a.c_len = (uint64_t *)take(n, 8);
    a.u_sel = (uint32_t *)take(2 * n, 4);
    if (write) {
        a.sacc = (LayAcc *)take(n, sizeof(LayAcc)), a.sacc_part = (LayAcc *)take(scan_parts(n), sizeof(LayAcc));
        a.crc_off = (uint64_t *)take(n, 8), a.crc_len = (uint64_t *)take(n, 8), a.comp_off = (uint64_t *)take(n, 8);
        a.e_in_off = (uint64_t *)take(n, 8), a.e_out_off = (uint64_t *)take(n, 8);
        a.crc = (uint32_t *)take(n, 4), a.comp_len = (uint32_t *)take(n, 4), a.slot = (uint32_t *)take(n, 4);
        a.e_in_len = (uint32_t *)take(n, 4), a.e_cap = (uint32_t *)take(n, 4), a.e_out_len = (uint32_t *)take(n, 4);
        a.e_status = (int32_t *)take(n, 4);
    }
    a.bytes = at;
    return a;
}

// what the assembly is made from (device pointers)
struct Inputs {
    uint64_t n;
    const chip_zip_source *src;
    uint64_t names_len, content_len, comp_all;
    const uint64_t *comp_off;  // all three NULL: every entry is stored
    const uint32_t *comp_len, *crc;
    uint32_t flags;
};

// ---- the assembly ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void zw_check_kernel(Inputs in, Arrays a, WriteDev *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= in.n) return;
    const chip_zip_source s = in.src[i];
    const bool have = in.comp_len != nullptr;
    zipw::Kept k{};
    const bool ok = zipw::keep(s, in.names_len, in.content_len, have, have ? in.comp_off[i] : 0, have ? in.comp_len[i] : 0, in.comp_all, in.crc[i], in.flags, k);
    if (!ok) {
        k = zipw::Kept{};  // (an entry of nothing: the layout stays in range, the host reads bad_key first)
        atomicMax((unsigned long long *)&ds->bad_key, (unsigned long long)~i);
    }
    a.kept[i] = k;
    a.acc[i] = LayAcc{zipw::local_len(k), k.method == CHIP_ZIP_DEFLATE ? 1u : 0u};
}

// behind the first scan: header_off, and the central record's length for the second
__global__ __launch_bounds__(256) void zw_sizes_kernel(uint64_t n, uint32_t flags, Arrays a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = a.acc[i].bytes + a.acc_part[i / SCAN_THREADS].bytes;
    a.hoff[i] = h;
    a.cacc[i] = zipw::central_len(a.kept[i], zipw::lho_in_extra(h, flags));
}

struct OutPut {  // a byte of a record, at any address; nothing behind `room` (the length the host compared)
    uint8_t *p;
    uint64_t room;
    __device__ __forceinline__ void operator()(uint32_t k, uint8_t v) const
    {
        if (k < room) p[k] = v;
    }
};

// behind the second scan, one lane per entry: the generated bytes, entries[i], the copy's units.  `out` NULL: entries[] only.
__global__ __launch_bounds__(256) void zw_records_kernel(uint64_t n, uint32_t flags, Arrays a, uint64_t cd_off, uint64_t out_len, uint8_t *out,
                                                         chip_zip_entry *entries)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const zipw::Kept k = a.kept[i];
    const uint64_t h = a.hoff[i], rel = a.cacc[i] + a.cacc_part[i / SCAN_THREADS], r = cd_off + rel;
    const bool zl = zipw::lho_in_extra(h, flags);
    if (entries) entries[i] = zipw::entry_of(k, h, r, flags);
    if (!out) return;
    const uint64_t name_at = h + zip::LOCAL_BYTES, extra_at = name_at + k.name_len, data_at = extra_at + zipw::local_extra(k);
    const uint64_t cname_at = r + zip::CENTRAL_BYTES, cextra_at = cname_at + k.name_len;
    // (the offsets are sums of what the check kept: inside out_len unless the scratch changed, which `room` guards)
    auto put_at = [&](uint64_t at) { return OutPut{out + at, at < out_len ? out_len - at : 0}; };
    OutPut lp = put_at(h), lx = put_at(extra_at), cp = put_at(r), cx = put_at(cextra_at);
    zipw::format_local(lp, k, zl, flags);
    if (k.zs) zipw::format_local_extra(lx, k);
    zipw::format_central(cp, k, h, zl, flags);
    zipw::format_central_extra(cx, k, h, zl);
    a.u_dst[2 * i] = name_at, a.u_src[2 * i] = k.name_off, a.u_len[2 * i] = k.name_len, a.u_sel[2 * i] = SRC_NAMES;
    a.u_dst[2 * i + 1] = data_at, a.u_src[2 * i + 1] = k.data_src, a.u_len[2 * i + 1] = k.c;
    a.u_sel[2 * i + 1] = k.method == CHIP_ZIP_DEFLATE ? SRC_COMP : SRC_CONTENT;
    a.c_dst[i] = rel + zip::CENTRAL_BYTES, a.c_src[i] = k.name_off, a.c_len[i] = k.name_len;
}

struct EndBytes {
    uint8_t b[zipw::END_ALL];
};
__global__ __launch_bounds__(128) void zw_end_kernel(uint8_t *at, EndBytes e, uint32_t len)
{
    if (threadIdx.x < len) at[threadIdx.x] = e.b[threadIdx.x];
}

// zip.hip's zip_copy_kernel with a source per unit: sel[u] (NULL: all SRC_NAMES) picks the buffer unit u is read from.  only < 3:
// units of another buffer count as empty, which is how one launch per source buffer is made of the same arrays.  The units'
// offsets ascend; the bytes between two units are nobody's here.
__global__ __launch_bounds__(64 * PACK_WAVES) void zw_copy_kernel(Sources srcs, const uint64_t *src_off, const uint64_t *src_len, const uint32_t *sel,
                                                                  uint32_t only, uint8_t *dst_base, const uint64_t *__restrict__ dst_off, uint32_t n,
                                                                  uint64_t total)
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
        uint32_t sel_v = SRC_NAMES;
        if (uj < n) {
            d_v = dst_off[uj], so_v = src_off[uj], len_v = src_len[uj];
            if (sel) sel_v = sel[uj];
        }
        const uint32_t here = (uint32_t)__popcll(__ballot(d_v < hi));  // (the offsets ascend: a prefix of the lanes)
        for (uint32_t j = 0; j < here; j++) {
            const uint64_t d = ((uint64_t)rdlane((uint32_t)(d_v >> 32), j) << 32) | rdlane((uint32_t)d_v, j);
            const uint64_t so = ((uint64_t)rdlane((uint32_t)(so_v >> 32), j) << 32) | rdlane((uint32_t)so_v, j);
            const uint64_t ln = ((uint64_t)rdlane((uint32_t)(len_v >> 32), j) << 32) | rdlane((uint32_t)len_v, j);
            const uint32_t k = rdlane(sel_v, j);
            if (k > SRC_COMP || (only <= SRC_COMP && k != only)) continue;  // (uniform)
            const uint8_t *base = k == SRC_NAMES ? srcs.base[0] : k == SRC_CONTENT ? srcs.base[1] : srcs.base[2];
            const uint64_t all = k == SRC_NAMES ? srcs.len[0] : k == SRC_CONTENT ? srcs.len[1] : srcs.len[2];
            const uint64_t s = d > lo ? d : lo, end = d + ln, e = end < hi ? end : hi;
            // (so + ln <= all: the check kept nothing else; once more, the scratch is all this kernel trusts)
            if (e > s && d <= hi && so <= all && ln <= all - so) copy_span(base + so + (s - d), dst_base + s, (uint32_t)(e - s), lane);
        }
        if (here < 64u) break;
    }
}

void enqueue_zw_copy(const Sources &srcs, const uint64_t *src_off, const uint64_t *src_len, const uint32_t *sel, uint32_t only, uint8_t *dst_base,
                     const uint64_t *dst_off, uint64_t n, uint64_t total, hipStream_t stream)
{
    if (n == 0 || total == 0) return;
    const uint64_t tiles = (total + ((uintptr_t)dst_base & 15u) + PACK_TILE - 1) / PACK_TILE;
    hipLaunchKernelGGL(zw_copy_kernel, dim3((uint32_t)((tiles + PACK_WAVES - 1) / PACK_WAVES)), dim3(64 * PACK_WAVES), 0, stream, srcs, src_off, src_len,
                       sel, only, dst_base, dst_off, (uint32_t)n, total);
}

// The copy's shape.  One launch over the local area with the selector is the default; CHIP_ZIPW_COPY=launches in the environment
// makes it one launch per source buffer, each taking the other buffers' units as empty (what chip_zip_decode does): the switch
// tools/time_zip_write.py measures the two with.
bool copy_per_source()
{
    const char *v = getenv("CHIP_ZIPW_COPY");
    return v && strcmp(v, "launches") == 0;
}

using ZipWriteSlot = SummarySlot<WriteDev>;
SlotCache<ZipWriteSlot> g_zip_write_cache;

// The assembly: enqueues everything, waits twice (out_len, the end).  The caller holds the cache's lock, has carved `a` out of
// buffer 0 and zeroed the slot's summary on the stream.
hipError_t assemble_enqueued(ZipWriteSlot &sl, const Arrays &a, const Inputs &in, const uint8_t *names, const uint8_t *content, const uint8_t *comp,
                             uint8_t *out, uint64_t out_cap, chip_zip_entry *entries, chip_zip_write_summary *summary, hipStream_t stream)
{
    const uint64_t n = in.n;
    WriteDev *ds = sl.d_sum;
    hipLaunchKernelGGL(zw_check_kernel, grid256(n), dim3(256), 0, stream, in, a, ds);
    enqueue_scan<LayAcc>(a.acc, a.acc, n, a.acc_part, &ds->lay, stream);
    hipLaunchKernelGGL(zw_sizes_kernel, grid256(n), dim3(256), 0, stream, n, in.flags, a);
    enqueue_scan<uint64_t>(a.cacc, a.cacc, n, a.cacc_part, &ds->cd_size, stream);
    hipError_t e = sl.fetch(stream);
    if (e != hipSuccess) return e;
    const WriteDev h = *sl.h_sum;
    if (h.enc_bad) return hipErrorUnknown;  // (a unit did not end CHIP_ENC_FINISHED)
    if (h.bad_key) {
        *summary = zipw::no_archive(n, CHIP_ZIPW_BAD_SOURCE, ~h.bad_key);
        return hipSuccess;
    }
    const uint64_t cd_off = h.lay.bytes, cd_size = h.cd_size;
    if (h.lay.defl > n || cd_off >= ((uint64_t)1 << 63) || cd_size >= ((uint64_t)1 << 63)) return hipErrorUnknown;  // (the inputs changed)
    const bool z = zipw::end_zip64(n, cd_off, cd_size, in.flags);
    const uint64_t end_at = cd_off + cd_size, out_len = end_at + zipw::end_len(z);
    chip_zip_write_summary s{n, h.lay.defl, out_len, cd_off, cd_size, out_len - zip::END_BYTES, 0, CHIP_ZIPW_OK, z ? 1 : 0};
    const bool room = out_len <= out_cap;
    if (!room) s.status = CHIP_ZIPW_NEED_OUTPUT;
    if (room || entries) hipLaunchKernelGGL(zw_records_kernel, grid256(n), dim3(256), 0, stream, n, in.flags, a, cd_off, out_len, room ? out : nullptr, entries);
    if (room) {
        EndBytes eb;
        zipw::BytePut put{eb.b};
        zipw::format_end(put, n, cd_off, cd_size, z);
        hipLaunchKernelGGL(zw_end_kernel, dim3(1), dim3(128), 0, stream, out + end_at, eb, (uint32_t)zipw::end_len(z));
        const Sources srcs{{names, content, comp}, {in.names_len, in.content_len, comp ? in.comp_all : 0}};
        if (copy_per_source()) {
            for (uint32_t k = SRC_NAMES; k <= SRC_COMP; k++)
                if (srcs.len[k]) enqueue_zw_copy(srcs, a.u_src, a.u_len, a.u_sel, k, out, a.u_dst, 2 * n, cd_off, stream);
        } else {
            enqueue_zw_copy(srcs, a.u_src, a.u_len, a.u_sel, 3u, out, a.u_dst, 2 * n, cd_off, stream);
        }
        if (in.names_len) enqueue_zw_copy(srcs, a.c_src, a.c_len, nullptr, SRC_NAMES, out + cd_off, a.c_dst, n, cd_size, stream);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;  // the slot is handed on only with nothing in flight
    *summary = s;
    return hipSuccess;
}

hipError_t assemble_locked(ZipWriteSlot &sl, const Inputs &in, const uint8_t *names, const uint8_t *content, const uint8_t *comp, uint8_t *out,
                           uint64_t out_cap, chip_zip_entry *entries, chip_zip_write_summary *summary, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    if ((e = sl.grow(0, carve(nullptr, in.n, false).bytes)) != hipSuccess) return e;
    const Arrays a = carve(sl.buf[0], in.n, false);
    if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(WriteDev), stream)) != hipSuccess) return e;
    return assemble_enqueued(sl, a, in, names, content, comp, out, out_cap, entries, summary, stream);
}

// ---- chip_zip_write: the CRC ranges and the encode batch ------------------------------------------------------------------------

// one lane per entry: the range the CRC pass reads (nothing, for a record whose content is out of range: the check refuses it
// later), and the slot of a deflate-eligible entry
__global__ __launch_bounds__(256) void zw_prep_kernel(uint64_t n, const chip_zip_source *src, uint64_t in_len, Arrays a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const chip_zip_source s = src[i];
    const bool in_range = s.data_off <= in_len && s.size <= in_len - s.data_off;
    const bool eligible = in_range && s.method == CHIP_ZIP_DEFLATE && s.size > 0 && s.size <= CHIP_ZIPW_DEFLATE_MAX;
    const uint64_t slot = eligible ? (zipw::deflate_bound(s.size) + 15) & ~(uint64_t)15 : 0;
    a.crc_off[i] = in_range ? s.data_off : 0;
    a.crc_len[i] = in_range ? s.size : 0;
    a.slot[i] = (uint32_t)slot;
    a.sacc[i] = LayAcc{slot, eligible ? 1u : 0u};
}

// behind the scan: the rows of the encode batch, comp_off of every entry
__global__ __launch_bounds__(256) void zw_units_kernel(uint64_t n, Arrays a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const LayAcc e = a.sacc[i] + a.sacc_part[i / SCAN_THREADS];
    a.sacc[i] = e;
    const uint32_t slot = a.slot[i];
    a.comp_off[i] = slot ? e.bytes : 0;
    a.comp_len[i] = 0;
    if (!slot || e.defl >= n) return;
    a.e_in_off[e.defl] = a.crc_off[i];
    a.e_in_len[e.defl] = (uint32_t)a.crc_len[i];
    a.e_out_off[e.defl] = e.bytes;
    a.e_cap[e.defl] = slot;
}

// behind the encode: comp_len of every entry from its unit
__global__ __launch_bounds__(256) void zw_gather_kernel(uint64_t n, uint64_t n_units, Arrays a, WriteDev *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !a.slot[i]) return;
    const uint64_t j = a.sacc[i].defl;
    if (j >= n_units || a.e_status[j] != CHIP_ENC_FINISHED || a.e_out_len[j] > a.slot[i]) {
        atomicAdd(&ds->enc_bad, 1u);
        return;
    }
    a.comp_len[i] = a.e_out_len[j];
}

// Enqueues everything, waits for the scratch sizes, then as the assembly does.  The caller holds the cache's lock.  Buffer 0 holds
// the arrays, buffer 1 the slot area.
hipError_t write_locked(ZipWriteSlot &sl, int level, uint32_t flags, uint64_t n, const chip_zip_source *src, const uint8_t *names, uint64_t names_len,
                        const uint8_t *in_base, uint64_t in_len, uint8_t *out, uint64_t out_cap, chip_zip_entry *entries,
                        chip_zip_write_summary *summary, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    if ((e = sl.grow(0, carve(nullptr, n, true).bytes)) != hipSuccess) return e;
    const Arrays a = carve(sl.buf[0], n, true);
    WriteDev *ds = sl.d_sum;
    if ((e = hipMemsetAsync(ds, 0, sizeof(WriteDev), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(zw_prep_kernel, grid256(n), dim3(256), 0, stream, n, src, in_len, a);
    enqueue_scan<LayAcc>(a.sacc, a.sacc, n, a.sacc_part, &ds->slots, stream);
    hipLaunchKernelGGL(zw_units_kernel, grid256(n), dim3(256), 0, stream, n, a);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const uint64_t area_bytes = sl.h_sum->slots.bytes, n_units = sl.h_sum->slots.defl;
    if (n_units > n) return hipErrorUnknown;
    if ((e = sl.grow(1, (size_t)area_bytes + 16)) != hipSuccess) return e;
    uint8_t *area = sl.buf[1];
    // (an archive of empty entries has no buffer: ranges of length 0 read nothing, the batch calls want a pointer)
    const uint8_t *base = in_base ? in_base : area;
    int rc = chip_crc32_batch((size_t)n, base, a.crc_off, a.crc_len, a.crc, stream);
    if (rc != CHIP_OK) return rc == CHIP_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;
    if (n_units) {
        rc = chip_encode_batch(CHIP_FMT_DEFLATE, level, (size_t)n_units, base, a.e_in_off, a.e_in_len, area, a.e_out_off, a.e_cap, a.e_out_len, a.e_status,
                               stream);
        if (rc != CHIP_OK) return hipErrorUnknown;
        hipLaunchKernelGGL(zw_gather_kernel, grid256(n), dim3(256), 0, stream, n, n_units, a, ds);
    }
    const Inputs in{n, src, names_len, in_len, area_bytes, a.comp_off, a.comp_len, a.crc, flags};
    return assemble_enqueued(sl, a, in, names, in_base, area, out, out_cap, entries, summary, stream);
}

// the refusals the three calls share; false = CHIP_E_INVALID
bool args_ok(uint64_t n, const void *src, const void *names, uint64_t names_len, const void *content, uint64_t content_len, const void *crc,
             bool need_crc, uint32_t flags, const void *out, uint64_t out_cap, const void *summary)
{
    if (!summary || (n && !src) || (names_len && !names) || (content_len && !content) || (need_crc && n && !crc) || (out_cap && !out)) return false;
    return n <= zipw::N_MAX && !(flags & ~zipw::FLAGS_KNOWN) && zipw::fits_63_bits(n, content_len);
}

// the archive of no entries: the end records alone
chip_zip_write_summary empty_archive(uint32_t flags, uint64_t out_cap, EndBytes &eb)
{
    const bool z = zipw::end_zip64(0, 0, 0, flags);
    const uint64_t len = zipw::end_len(z);
    zipw::BytePut put{eb.b};
    zipw::format_end(put, 0, 0, 0, z);
    return chip_zip_write_summary{0, 0, len, 0, 0, len - zip::END_BYTES, 0, len > out_cap ? CHIP_ZIPW_NEED_OUTPUT : CHIP_ZIPW_OK, z ? 1 : 0};
}

int empty_on_device(uint32_t flags, void *out, uint64_t out_cap, chip_zip_write_summary *summary, void *stream)
{
    EndBytes eb;
    const chip_zip_write_summary s = empty_archive(flags, out_cap, eb);
    if (s.status == CHIP_ZIPW_OK) {
        int devices = 0;
        if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) return CHIP_E_NO_DEVICE;
        if (hipMemcpyAsync(out, eb.b, (size_t)s.out_len, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
            return CHIP_E_LAUNCH;
    }
    *summary = s;
    return CHIP_OK;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

uint64_t chip_zip_write_bound(uint64_t n, uint64_t names_total, uint64_t content_total) { return zipw::write_bound(n, names_total, content_total); }

int chip_zip_assemble_host(uint64_t n, const chip_zip_source *src, const uint8_t *names, uint64_t names_len, const uint8_t *content,
                           uint64_t content_len, const uint8_t *comp, uint64_t comp_all, const uint64_t *comp_off, const uint32_t *comp_len,
                           const uint32_t *crc, uint32_t flags, uint8_t *out, uint64_t out_cap, chip_zip_entry *entries, chip_zip_write_summary *summary)
{
    const int given = (comp != nullptr) + (comp_off != nullptr) + (comp_len != nullptr);
    if (!args_ok(n, src, names, names_len, content, content_len, crc, true, flags, out, out_cap, summary) || (given != 0 && given != 3))
        return CHIP_E_INVALID;
    zipw::assemble_host(n, src, names, names_len, content, content_len, comp, comp_all, comp_off, comp_len, crc, flags, out, out_cap, entries, summary);
    return CHIP_OK;
}

int chip_zip_assemble(uint64_t n, const chip_zip_source *src, const void *names, uint64_t names_len, const void *content, uint64_t content_len,
                      const void *comp, uint64_t comp_all, const uint64_t *comp_off, const uint32_t *comp_len, const uint32_t *crc, uint32_t flags,
                      void *out, uint64_t out_cap, chip_zip_entry *entries, chip_zip_write_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    const int given = (comp != nullptr) + (comp_off != nullptr) + (comp_len != nullptr);
    if (!args_ok(n, src, names, names_len, content, content_len, crc, true, flags, out, out_cap, summary) || (given != 0 && given != 3))
        return CHIP_E_INVALID;
    if (n == 0) return empty_on_device(flags, out, out_cap, summary, stream);
    *summary = zipw::no_archive(n, CHIP_ZIPW_OK, 0);
    const Inputs in{n, src, names_len, content_len, given ? comp_all : 0, comp_off, comp_len, crc, flags};
    return with_slot(
        g_zip_write_cache, stream,
        [&](ZipWriteSlot &sl, hipStream_t s) {
            return assemble_locked(sl, in, (const uint8_t *)names, (const uint8_t *)content, (const uint8_t *)comp, (uint8_t *)out, out_cap, entries,
                                   summary, s);
        },
        [&] { *summary = zipw::no_archive(n, CHIP_ZIPW_OK, 0); });
}

int chip_zip_write(int level, uint32_t flags, uint64_t n, const chip_zip_source *src, const void *names, uint64_t names_len, const void *in_base,
                   uint64_t in_len, void *out_base, uint64_t out_cap, chip_zip_entry *entries, chip_zip_write_summary *summary, void *stream)
{
    if (!args_ok(n, src, names, names_len, in_base, in_len, nullptr, false, flags, out_base, out_cap, summary) || level < -1 || level > 9 ||
        ((uintptr_t)in_base & 3u))
        return CHIP_E_INVALID;
    if (n == 0) return empty_on_device(flags, out_base, out_cap, summary, stream);
    // the slots are laid out on the device with zipw::deflate_bound: it has to be the encoder's own bound
    for (uint64_t v : {(uint64_t)1, (uint64_t)65535, (uint64_t)65536, (uint64_t)1000003, (uint64_t)CHIP_ZIPW_DEFLATE_MAX})
        if (chip_encode_bound(CHIP_FMT_DEFLATE, (size_t)v) != zipw::deflate_bound(v)) return CHIP_E_LAUNCH;
    *summary = zipw::no_archive(n, CHIP_ZIPW_OK, 0);
    return with_slot(
        g_zip_write_cache, stream,
        [&](ZipWriteSlot &sl, hipStream_t s) {
            return write_locked(sl, level, flags, n, src, (const uint8_t *)names, names_len, (const uint8_t *)in_base, in_len, (uint8_t *)out_base, out_cap,
                                entries, summary, s);
        },
        [&] { *summary = zipw::no_archive(n, CHIP_ZIPW_OK, 0); });
}

}  // extern "C"
