// The block finder of ONE large deflate stream: chip_inflate_find_starts and its host form.
//
// A stream can be decoded from a block boundary on once the boundary is known, and a dynamic block's header is recognisable without
// decoding anything in front of it: the candidate rule of include/compu_hip.h, whose one text for host and device is
// inflate_find_core.h.  The buffer is cut into chunks of chunk_bytes; chunk k's start is its least candidate.
//   find     find_starts_kernel: one wave per 2 KiB piece of a chunk, 64 lanes on 64 consecutive bit positions; the 13-bit pre-filter
//            leaves about seven of them, which check their whole header, each for itself; a wave stops at its first round with a
//            hit, or when a piece in front of it has one: the least hit of a chunk is its start
//   compact  find_compact_kernel: the chunks' answers in ascending order without the gaps, and their count
// No wave waits for another.  Nothing here decodes: whether a start is a real boundary is for the decode that uses it to find out.
#include "chip_internal.h"
#include "inflate_find_core.h"
#include "launch_slots.h"
#include "plan_common.h"

namespace chip {

namespace {

constexpr uint64_t NO_START = ~0ull;
constexpr uint32_t CHUNK_MIN = 256, CHUNK_MAX = CHIP_GZPLAN_WINDOW;
constexpr uint32_t PIECE_BYTES = 2048;  // of a chunk that one wave searches: 256 rounds of 64 positions

// found[k - 1] (NO_START before the launch) = the start of chunk k = blockIdx.x + 1.  A chunk is searched in gridDim.y pieces of
// `piece_bits` (a multiple of 64), a wave each: the least hit wins (atomicMin), and a wave stops at its own first hit or as soon
// as a piece in front of its position has one.  Workgroups are handed out with x running fastest, so the first pieces of every
// chunk run first and most later pieces of a chunk that has a start end at their first look.
__global__ __launch_bounds__(64) void find_starts_kernel(const uint8_t *in, uint64_t len, uint64_t first_bit, uint32_t chunk_bytes, uint64_t piece_bits,
                                                         uint64_t *found)
{
    const uint32_t lane = lane_id();
    uint64_t lo, hi;
    find::chunk_range(len, first_bit, chunk_bytes, (uint64_t)blockIdx.x + 1u, lo, hi);
    lo += piece_bits * blockIdx.y;
    if (hi > lo + piece_bits) hi = lo + piece_bits;
    unsigned long long *const best = (unsigned long long *)&found[blockIdx.x];
    for (uint64_t p0 = lo; p0 < hi; p0 += 64) {
        if (((p0 - lo) & 1023u) == 0 && __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p0) break;  // (every 16 rounds)
        const uint64_t p = p0 + lane;
        bool c = p < hi && find::prefilter(find::peek(in, len, p));
        if (c) c = find::header_ok(in, len, p);
        const uint64_t m = __ballot(c);
        if (m) {
            if (lane == 0) atomicMin(best, (unsigned long long)(p0 + (uint32_t)__ffsll((long long)m) - 1u));
            break;
        }
    }
}

struct FindSum {
    uint64_t n;
};

// starts[0 .. min(n, max)) = the entries of found[0 .. n_chunks) that are starts, in order; sum->n = how many there are.  One
// workgroup: a tile of 1024 entries per trip, ranks by ballot inside a wave and a sum over the 16 waves.
__global__ __launch_bounds__(1024) void find_compact_kernel(const uint64_t *found, uint32_t n_chunks, uint64_t max, uint64_t *starts, FindSum *sum)
{
    __shared__ uint32_t wcount[16];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t base = 0;
    for (uint32_t t0 = 0; t0 < n_chunks; t0 += 1024u) {
        const uint32_t i = t0 + threadIdx.x;
        const uint64_t v = i < n_chunks ? found[i] : NO_START;
        const bool has = v != NO_START;
        const uint64_t m = __ballot(has);
        if (lane == 0) wcount[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 16; w++) {
            const uint32_t c = wcount[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        const uint64_t at = base + before + (uint32_t)__popcll(m & lanemask_lt());
        if (has && at < max) starts[at] = v;
        base += total;
        __syncthreads();  // (the next trip's counts stay behind these reads)
    }
    if (threadIdx.x == 0) sum->n = base;
}

// buffer 0: one answer per chunk; a launch slot
using FindSlot = SummarySlot<FindSum>;
SlotCache<FindSlot> g_find_cache;

bool find_args_ok(const void *in, uint64_t len, uint64_t first_bit, uint32_t chunk_bytes, uint64_t max, const uint64_t *starts, const uint64_t *n)
{
    return n && (in || !len) && (starts || !max) && chunk_bytes >= CHUNK_MIN && chunk_bytes <= CHUNK_MAX && len <= CHIP_GZPLAN_WINDOW &&
           first_bit <= len * 8;
}

// chunks 1 .. n_chunks - 1 are looked at
uint32_t chunks_of(uint64_t len, uint32_t chunk_bytes) { return (uint32_t)((len + chunk_bytes - 1) / chunk_bytes); }

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_inflate_find_starts_host(const uint8_t *in, uint64_t len, uint64_t first_bit, uint32_t chunk_bytes, uint64_t max, uint64_t *starts,
                                  uint64_t *n)
{
    if (!find_args_ok(in, len, first_bit, chunk_bytes, max, starts, n)) return CHIP_E_INVALID;
    uint64_t count = 0;
    const uint32_t n_chunks = chunks_of(len, chunk_bytes);
    for (uint32_t k = 1; k < n_chunks; k++) {
        uint64_t lo, hi;
        find::chunk_range(len, first_bit, chunk_bytes, k, lo, hi);
        for (uint64_t p = lo; p < hi; p++) {
            if (!find::prefilter(find::peek(in, len, p)) || !find::header_ok(in, len, p)) continue;
            if (count < max) starts[count] = p;
            count++;
            break;
        }
    }
    *n = count;
    return CHIP_OK;
}

int chip_inflate_find_starts(const void *in_base, uint64_t len, uint64_t first_bit, uint32_t chunk_bytes, uint64_t max, uint64_t *starts,
                             uint64_t *n, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!find_args_ok(in_base, len, first_bit, chunk_bytes, max, starts, n)) return CHIP_E_INVALID;
    *n = 0;
    const uint32_t n_chunks = chunks_of(len, chunk_bytes);
    if (n_chunks < 2) return CHIP_OK;
    return with_slot(
        g_find_cache, stream,
        [&](FindSlot &sl, hipStream_t s) {
            hipError_t e = sl.summary();
            if (e != hipSuccess) return e;
            if ((e = sl.grow(0, (size_t)(n_chunks - 1) * 8)) != hipSuccess) return e;
            uint64_t *found = (uint64_t *)sl.buf[0];
            if ((e = hipMemsetAsync(found, 0xFF, (size_t)(n_chunks - 1) * 8, s)) != hipSuccess) return e;
            // pieces of PIECE_BYTES, at most as many as a grid's y takes
            uint64_t pieces = ((uint64_t)chunk_bytes + PIECE_BYTES - 1) / PIECE_BYTES;
            if (pieces > 65535) pieces = 65535;
            const uint64_t piece_bits = ((8ull * chunk_bytes + pieces - 1) / pieces + 63) & ~63ull;
            hipLaunchKernelGGL(find_starts_kernel, dim3(n_chunks - 1, (uint32_t)pieces), dim3(64), 0, s, (const uint8_t *)in_base, len, first_bit, chunk_bytes,
                               piece_bits, found);
            hipLaunchKernelGGL(find_compact_kernel, dim3(1), dim3(1024), 0, s, (const uint64_t *)found, n_chunks - 1, max, starts, sl.d_sum);
            if ((e = sl.fetch(s)) != hipSuccess) return e;
            *n = sl.h_sum->n;
            return hipSuccess;
        },
        [&] { *n = 0; });
}

}  // extern "C"
