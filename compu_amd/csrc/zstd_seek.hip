// The seek table of zstd's seekable format: chip_zstd_seek_plan[_host] reads one as a plan,
// chip_zstd_seek_table_write[_host] writes one, chip_xxh64_batch makes the checksums its entries hold.  The definitions are in
// include/compu_hip.h; the walk and the writer's bytes that host and device share are in zstd_seek_core.h.  The verified read of
// such a plan, chip_zstd_seek_read, is a source of the range reader (read_ranges.hip).
//
// The plan on the device, in stream order, with the scan and the slot of plan_common.h:
//   head      zseek_head_kernel: one lane runs zseek::head() over the footer and the skippable header
//      -- the host reads n, T and the verdict so far and sizes the grid --
//   entries   zseek_entries_kernel: one lane per entry reads its 8 or 12 bytes: in_len, out_cap, checksum of the first max_frames,
//             {c_i, d_i} for the scan, the lowest entry whose d_i is 0xFFFFFFFF
//   scan      exclusive scan of the pairs {c_i, d_i}: the two 64-bit sums in one pass
//   offsets   zseek_offsets_kernel: in_off, out_off of the first max_frames
//      -- the host reads the sums and judges them (zseek::sums_summary) --
// Every byte of the tail is read once, and the entries' positions follow from the n the host holds: input that changes during the
// call changes the answer, never where anything is read or written.
#include "chip_internal.h"
#include "launch_slots.h"
#include "plan_common.h"
#include "wave_checksums.h"
#include "zstd_seek_core.h"

namespace chip {

namespace {

static_assert(sizeof(chip_zstd_seek_summary) == 48, "chip_zstd_seek_summary");

struct SeekAcc {
    uint64_t c, d;  // compressed and decoded bytes
};
__host__ __device__ __forceinline__ SeekAcc operator+(const SeekAcc &a, const SeekAcc &b) { return SeekAcc{a.c + b.c, a.d + b.d}; }
__device__ __forceinline__ SeekAcc shfl_up_t(const SeekAcc &v, uint32_t d) { return SeekAcc{shfl_up_t(v.c, d), shfl_up_t(v.d, d)}; }

// what the kernels hand to the host (device memory, zeroed per call, copied back twice)
struct SeekDev {
    zseek::Head head;
    SeekAcc sum;        // total of the scan
    uint64_t unsized;   // ~(the lowest i with d_i == 0xFFFFFFFF), 0: none
};

__global__ void zseek_head_kernel(const uint8_t *tail, uint64_t tail_len, uint64_t file_len, SeekDev *ds)
{
    if (threadIdx.x || blockIdx.x) return;
    ds->head = zseek::head(tail, tail_len, file_len);
}

__global__ __launch_bounds__(256) void zseek_entries_kernel(const uint8_t *tail, uint64_t tail_len, zseek::Head h, uint64_t max_frames, uint32_t *in_len,
                                                            uint32_t *out_cap, uint32_t *checksum, SeekAcc *acc, SeekDev *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= h.n) return;
    const zseek::Entry e = zseek::entry(tail, tail_len, h, i);
    acc[i] = SeekAcc{e.c, e.d};
    if (e.d == zseek::UNSIZED) atomicMax((unsigned long long *)&ds->unsized, (unsigned long long)~i);
    if (i >= max_frames) return;
    in_len[i] = e.c;
    out_cap[i] = e.d;
    if (checksum) checksum[i] = e.x;
}

// behind the scan: the offsets of the first `count` entries
__global__ __launch_bounds__(256) void zseek_offsets_kernel(const SeekAcc *acc, const SeekAcc *part, uint64_t count, uint64_t *in_off, uint64_t *out_off)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const SeekAcc a = acc[i] + part[i / SCAN_THREADS];
    in_off[i] = a.c;
    out_off[i] = a.d;
}

using SeekSlot = SummarySlot<SeekDev>;
SlotCache<SeekSlot> g_seek_cache;

inline dim3 grid256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// tail_len >= 17: enqueues everything, waits twice (the head, the sums).  The caller holds the cache's lock.  Buffer 0 holds the
// pairs and the scan's partials: 16 bytes per entry.
hipError_t seek_plan_locked(SeekSlot &sl, const uint8_t *tail, uint64_t tail_len, uint64_t file_len, uint64_t max_frames, uint64_t *in_off,
                            uint32_t *in_len, uint64_t *out_off, uint32_t *out_cap, uint32_t *checksum, chip_zstd_seek_summary &out, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    SeekDev *ds = sl.d_sum;
    if ((e = hipMemsetAsync(ds, 0, sizeof(SeekDev), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(zseek_head_kernel, dim3(1), dim3(64), 0, stream, tail, tail_len, file_len, ds);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const zseek::Head h = sl.h_sum->head;
    // (what the kernel answered is checked like any input: the entries must lie in the tail)
    if (h.status == CHIP_ZSEEK_OK && (h.n > zseek::MAX_FRAMES || h.es != 8u + 4u * h.cs || h.cs > 1u || h.T != zseek::FIXED + h.es * h.n || h.T > tail_len))
        return hipErrorUnknown;
    if (h.status != CHIP_ZSEEK_OK || h.n == 0) {
        out = h.status == CHIP_ZSEEK_OK ? zseek::sums_summary(h, file_len, 0, 0, 0) : zseek::head_summary(h);
        return hipSuccess;
    }
    const uint64_t n = h.n, count = n < max_frames ? n : max_frames;
    if ((e = sl.grow(0, (size_t)(n + scan_parts(n)) * sizeof(SeekAcc))) != hipSuccess) return e;
    SeekAcc *acc = (SeekAcc *)sl.buf[0], *part = acc + n;
    hipLaunchKernelGGL(zseek_entries_kernel, grid256(n), dim3(256), 0, stream, tail, tail_len, h, max_frames, in_len, out_cap, checksum, acc, ds);
    enqueue_scan<SeekAcc>(acc, acc, n, part, &ds->sum, stream);
    if (count)
        hipLaunchKernelGGL(zseek_offsets_kernel, grid256(count), dim3(256), 0, stream, (const SeekAcc *)acc, (const SeekAcc *)part, count, in_off, out_off);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const SeekDev &r = *sl.h_sum;
    const uint64_t lowest = r.unsized ? ~r.unsized : n;
    if (lowest > n) return hipErrorUnknown;
    out = zseek::sums_summary(h, file_len, lowest, r.sum.c, r.sum.d);
    return hipSuccess;
}

__global__ __launch_bounds__(256) void zseek_table_kernel(uint8_t *dst, uint64_t n, const uint32_t *c_len, const uint32_t *d_len, const uint32_t *checksum)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < (n ? n : 1)) zseek::write_part(dst, n, c_len, d_len, checksum, i);
}

// one wave per range
__global__ __launch_bounds__(64) void xxh64_batch_kernel(const uint8_t *base, const uint64_t *off, const uint32_t *len, uint64_t *digest)
{
    __shared__ uint64_t stage[512];
    const uint64_t h = wave_xxh64(stage, base + off[blockIdx.x], len[blockIdx.x]);
    if (lane_id() == 0) digest[blockIdx.x] = h;
}

bool have_device()
{
    int devices = 0;
    return hipGetDeviceCount(&devices) == hipSuccess && devices > 0;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_xxh64_batch(size_t n, const void *base, const uint64_t *off, const uint32_t *len, uint64_t *digest, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if ((uint64_t)n > 0x7fffffffull || (n && (!base || !off || !len || !digest))) return CHIP_E_INVALID;
    if (n == 0) return CHIP_OK;
    if (!have_device()) return CHIP_E_NO_DEVICE;
    hipLaunchKernelGGL(xxh64_batch_kernel, dim3((uint32_t)n), dim3(64), 0, (hipStream_t)stream, (const uint8_t *)base, off, len, digest);
    return hipGetLastError() == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}

int chip_zstd_seek_plan_host(const uint8_t *tail, uint64_t tail_len, uint64_t file_len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len,
                             uint64_t *out_off, uint32_t *out_cap, uint32_t *checksum, chip_zstd_seek_summary *summary)
{
    if (!zseek::plan_args_ok(tail, tail_len, file_len, max_frames, in_off, in_len, out_off, out_cap, summary)) return CHIP_E_INVALID;
    zseek::plan_host(tail, tail_len, file_len, max_frames, in_off, in_len, out_off, out_cap, checksum, summary);
    return CHIP_OK;
}

int chip_zstd_seek_plan(const void *tail, uint64_t tail_len, uint64_t file_len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len,
                        uint64_t *out_off, uint32_t *out_cap, uint32_t *checksum, chip_zstd_seek_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!zseek::plan_args_ok((const uint8_t *)tail, tail_len, file_len, max_frames, in_off, in_len, out_off, out_cap, summary)) return CHIP_E_INVALID;
    if (file_len < zseek::FIXED || tail_len < zseek::FIXED) {  // (no byte is looked at: the host's answer)
        *summary = zseek::head_summary(zseek::head(nullptr, tail_len, file_len));
        return CHIP_OK;
    }
    const chip_zstd_seek_summary NOTHING{};
    *summary = NOTHING;
    chip_zstd_seek_summary r = NOTHING;
    const int rc = with_slot(
        g_seek_cache, stream,
        [&](SeekSlot &sl, hipStream_t s) {
            return seek_plan_locked(sl, (const uint8_t *)tail, tail_len, file_len, max_frames, in_off, in_len, out_off, out_cap, checksum, r, s);
        },
        [&] { *summary = NOTHING; });
    if (rc == CHIP_OK) *summary = r;
    return rc;
}

int chip_zstd_seek_table_write_host(uint64_t n, const uint32_t *c_len, const uint32_t *d_len, const uint32_t *checksum, void *dst, uint64_t dst_cap,
                                    uint64_t *table_bytes)
{
    if (!zseek::write_args_ok(n, c_len, d_len, dst, dst_cap, table_bytes)) return CHIP_E_INVALID;
    zseek::write_host(n, c_len, d_len, checksum, (uint8_t *)dst, dst_cap, table_bytes);
    return CHIP_OK;
}

int chip_zstd_seek_table_write(uint64_t n, const uint32_t *c_len, const uint32_t *d_len, const uint32_t *checksum, void *dst, uint64_t dst_cap,
                               uint64_t *table_bytes, void *stream)
{
    if (!zseek::write_args_ok(n, c_len, d_len, dst, dst_cap, table_bytes)) return CHIP_E_INVALID;
    *table_bytes = zseek::table_bytes(n, checksum != nullptr);
    if (*table_bytes > dst_cap) return CHIP_OK;
    if (!have_device()) return CHIP_E_NO_DEVICE;
    hipLaunchKernelGGL(zseek_table_kernel, grid256(n ? n : 1), dim3(256), 0, (hipStream_t)stream, (uint8_t *)dst, n, c_len, d_len, checksum);
    return hipGetLastError() == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}

}  // extern "C"
