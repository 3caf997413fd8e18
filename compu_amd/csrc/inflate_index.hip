// The checkpoint index of ONE large deflate stream, its build: chip_inflate_index_build.
//
// The build is a decode that takes notes.  inflate_index_kernel is inflate_unit.h's unit loop compiled with the recording
// (CHIP_INFLATE_INDEX, see inflate_unit there): one wave decodes the unit as inflate_kernel would and stores the (bit, out) of every
// block boundary that is a point.  This translation unit keeps the recording out of the batch kernels.  Behind it, in stream order:
//   windows   index_windows_kernel: per stored point the up to 32 KiB of content in front of it, out of the decoded output
//   checks    index_checks_kernel: one wave runs the stream's check (CRC-32 / Adler-32) from point to point over the decoded output,
//             every step wave-parallel (wave_crc32 / wave_adler32 with the previous point's value as seed), and to the end of a
//             finished stream.  The build kernel cannot do this at a boundary without giving up its LDS (the CRC tables take all of
//             it); a pass of its own reads the output once more at a few percent of what the one-wave decode costs.
// The read side (chip_inflate_index_read, chip_inflate_index_units_host) is in read_ranges.hip.
#define CHIP_INFLATE_INDEX 1
#include "inflate_unit.h"

#include "pack_copy.h"
#include "plan_common.h"

namespace chip {

// ONE wave decodes the one unit and records its points
__global__ __launch_bounds__(64, CHIP_WAVES_PER_SIMD) void inflate_index_kernel(BatchArgs a, IndexRec ix, uint32_t *scratch)
{
    __shared__ WaveLds L;
    inflate_unit<false>(a, 0, L, scratch, nullptr, ix);
}

namespace {

constexpr uint32_t WINDOW = 32768;

// the unit of the build in device memory (the kernels read their one-entry arrays here) and what they answer
struct DevBuild {
    uint64_t in_off, out_off;
    uint32_t in_len, out_cap;
    uint32_t out_len, in_used;
    int32_t status;
    uint32_t walk[3];  // IndexRec::walk
    uint32_t check, pad;
};

// slot k = content[pt_out[k] - wl .. pt_out[k]) with wl = min(32768, pt_out[k]); four waves per point, 4 KiB per wave and round
__global__ __launch_bounds__(256) void index_windows_kernel(const uint8_t *out, const uint64_t *pt_out, uint8_t *windows)
{
    const uint32_t lane = lane_id(), wave = rdfirst(threadIdx.x >> 6);
    const uint64_t o = rdfirst64(pt_out[blockIdx.x]);
    const uint32_t wl = o < WINDOW ? (uint32_t)o : WINDOW;
    const uint8_t *src = out + (o - wl);
    uint8_t *dst = windows + (uint64_t)WINDOW * blockIdx.x;
    for (uint32_t at = wave * PACK_TILE; at < wl; at += 4 * PACK_TILE)
        copy_span(src + at, dst + at, wl - at < PACK_TILE ? wl - at : PACK_TILE, lane);
}

// pt_check[k] for the n stored points and DevBuild::check, by one wave
__global__ __launch_bounds__(64) void index_checks_kernel(const uint8_t *out, const uint64_t *pt_out, uint32_t *pt_check, uint32_t n, DevBuild *d)
{
    __shared__ uint32_t tab[2048];
    const uint32_t lane = lane_id();
    const uint32_t wrap = rdfirst(d->walk[2]);
    uint32_t run = wrap == 1 ? 1u : 0u, cov = 0;
    auto advance = [&](uint32_t to) {
        if (wrap == 1) run = wave_adler32(out + cov, to - cov, run);
        else if (wrap == 2) run = wave_crc32((LDS_AS uint32_t *)tab, out + cov, to - cov, run);
        cov = to;
    };
    for (uint32_t k = 0; k < n; k++) {
        advance(rdfirst((uint32_t)pt_out[k]));
        if (lane == 0) pt_check[k] = run;
    }
    if (rdfirst((uint32_t)d->status) == (uint32_t)CHIP_FINISHED) {
        advance(rdfirst(d->out_len));
        if (lane == 0) d->check = run;
    }
}

// token rows of the one wave in buffer 0; a launch slot
using BuildSlot = SummarySlot<DevBuild>;
SlotCache<BuildSlot> g_build_cache;

hipError_t build_locked(BuildSlot &sl, int format, const uint8_t *in_base, uint32_t len, uint8_t *out_base, uint32_t out_cap, uint32_t spacing,
                        uint64_t max_points, uint64_t *pt_bit, uint64_t *pt_out, uint32_t *pt_check, uint8_t *windows,
                        chip_inflate_index_summary *summary, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    if ((e = sl.grow(0, (size_t)SCRATCH_WORDS * 4)) != hipSuccess) return e;
    DevBuild *d = sl.d_sum;
    *sl.h_sum = DevBuild{0, 0, len, out_cap, 0, 0, 0, {0, 0, 0}, 0, 0};
    if ((e = hipMemcpyAsync(d, sl.h_sum, sizeof(DevBuild), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    BatchArgs a{};
    a.in_base = in_base, a.in_off = &d->in_off, a.in_len = &d->in_len;
    a.out_base = out_base, a.out_off = &d->out_off, a.out_cap = &d->out_cap;
    a.out_len = &d->out_len, a.in_used = &d->in_used, a.status = &d->status;
    a.n = 1, a.format = format;
    const IndexRec ix{pt_bit, pt_out, max_points, spacing, d->walk};
    hipLaunchKernelGGL(inflate_index_kernel, dim3(1), dim3(64), 0, stream, a, ix, (uint32_t *)sl.buf[0]);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;  // the point count sizes what follows
    const uint64_t n_points = sl.h_sum->walk[0];
    const uint32_t n = (uint32_t)(n_points < max_points ? n_points : max_points), wrap = sl.h_sum->walk[2];
    if (n) hipLaunchKernelGGL(index_windows_kernel, dim3(n), dim3(256), 0, stream, (const uint8_t *)out_base, (const uint64_t *)pt_out, windows);
    if (n || (wrap && sl.h_sum->status == CHIP_FINISHED)) {
        hipLaunchKernelGGL(index_checks_kernel, dim3(1), dim3(64), 0, stream, (const uint8_t *)out_base, (const uint64_t *)pt_out, pt_check, n, d);
        if ((e = sl.fetch(stream)) != hipSuccess) return e;
    }
    const DevBuild &h = *sl.h_sum;
    *summary = chip_inflate_index_summary{n_points, h.out_len, h.in_used, h.walk[1], h.status, h.walk[2], h.check, 0};
    return hipSuccess;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_inflate_index_build(int format, const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, uint32_t spacing, uint64_t max_points,
                             uint64_t *pt_bit, uint64_t *pt_out, uint32_t *pt_check, void *windows, chip_inflate_index_summary *summary,
                             void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (format != CHIP_FMT_DEFLATE && format != CHIP_FMT_ZLIB && format != CHIP_FMT_GZIP && format != CHIP_FMT_AUTO) return CHIP_E_INVALID;
    if (!summary || !in_base || ((uintptr_t)in_base & 3u) || !out_base || len > CHIP_GZPLAN_WINDOW || out_cap > 0xFFFFFFF0ull) return CHIP_E_INVALID;
    if (max_points && (!pt_bit || !pt_out || !pt_check || !windows)) return CHIP_E_INVALID;
    *summary = chip_inflate_index_summary{0, 0, 0, 0, CHIP_NEED_INPUT, 0, 0, 0};
    return with_slot(
        g_build_cache, stream,
        [&](BuildSlot &sl, hipStream_t s) {
            return build_locked(sl, format, (const uint8_t *)in_base, (uint32_t)len, (uint8_t *)out_base, (uint32_t)out_cap, spacing ? spacing : 1u << 20,
                                max_points, pt_bit, pt_out, pt_check, (uint8_t *)windows, summary, s);
        },
        [&] { *summary = chip_inflate_index_summary{0, 0, 0, 0, CHIP_NEED_INPUT, 0, 0, 0}; });
}

}  // extern "C"
