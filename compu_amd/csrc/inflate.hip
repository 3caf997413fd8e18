// Batched DEFLATE inflate for gfx950 (MI355X): inflate_kernel, the decoder's persistent grid, and the host side of every batched
// inflate launch -- the (device, stream) launch slot, its lock, and the one launch path of decode batches, size passes and routed
// (CHIP_FMT_DETECT) batches.  The device code (one wave decodes one unit: inflate_unit) is inflate_unit.h; the kernels beside this
// one are in inflate_sizes.hip, inflate_members.hip and inflate_index.hip, which this file's launcher reaches through their
// enqueue functions.
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "inflate_unit.h"
#include "launch_slots.h"

namespace chip {

// Persistent grid: each wave takes the next unit from *next_unit until the batch is exhausted.
// (The loop is written out in each of the four batch kernels: shared as an always-inline function template it compiles to other
// code -- inflate_kernel 7038 -> 7033 instructions, 92 -> 100 scalar registers parked in lanes)
__global__ __launch_bounds__(64, CHIP_WAVES_PER_SIMD) void inflate_kernel(BatchArgs a, uint32_t *scratch, uint32_t *next_unit)
{
    __shared__ WaveLds L;
    uint32_t *grow = scratch + (size_t)blockIdx.x * SCRATCH_WORDS;
    const uint32_t limit = a.sel_n ? *a.sel_n : a.n;
    for (;;) {
        uint32_t i = 0;
        if (lane_id() == 0) i = atomicAdd(next_unit, 1u);
        i = rdfirst(i);
        if (i >= limit) break;
        const uint32_t u = a.sel ? rdfirst(a.sel[i]) : i;
        inflate_unit<false>(a, u, L, grow, nullptr);
        WSYNC();  // the next unit reuses the LDS
    }
}

namespace {
// Token scratch and the unit counter of a launch, and the lists of a routed batch: a launch slot ("Launch slots").
// A streaming decoder (batches of one) holds one 64 KiB slot, not the 270 MB a full grid needs.
struct LaunchSlot : WaveScratch {
    uint32_t *route = nullptr;  // routed batches: [0,1] list lengths, then two index lists of route_cap entries
    size_t route_cap = 0;
    void free()
    {
        WaveScratch::free();
        (void)hipFree(route);
    }
};
SlotCache<LaunchSlot> g_slots;
ResidentWaves g_resident;

// (caller holds g_slots.mu) the slot of (current device, stream) with token scratch for min(n, resident waves) waves
hipError_t slot_for(hipStream_t stream, uint32_t n, LaunchSlot *&sl)
{
#ifdef CHIP_EXP_PER_CU  // occupancy probe: a smaller persistent grid (at most this many waves per CU)
    const int per_cu_cap = CHIP_EXP_PER_CU;
#else
    const int per_cu_cap = 0;
#endif
    int max_blocks = 0, per_cu = 0;
    hipError_t e = g_slots.at(stream, sl);
    if (e == hipSuccess) e = g_resident.get((const void *)inflate_kernel, max_blocks, per_cu_cap, &per_cu);
    if (e != hipSuccess) return e;
#ifdef CHIP_STATS
    if (per_cu && getenv("CHIP_DEBUG_GRID"))
        fprintf(stderr, "[chip] inflate_kernel: %d waves per CU x %d CUs resident (LDS %zu B per wave)\n", per_cu, max_blocks / per_cu, sizeof(WaveLds));
#endif
    return sl->reserve(stream, n, max_blocks, (size_t)SCRATCH_WORDS * 4);
}

// (caller holds g_slots.mu) device scratch of a routed batch on `stream`, cached with the inflate slot: two index lists of n
// entries + 2 counters
hipError_t route_scratch_locked(hipStream_t stream, size_t n, uint32_t **sel_inflate, uint32_t **sel_zstd, uint32_t **counts)
{
    LaunchSlot *slp = nullptr;
    hipError_t e = g_slots.at(stream, slp);
    if (e != hipSuccess) return e;
    LaunchSlot &sl = *slp;
    if (n > sl.route_cap) {
        // work queued on the stream may still read the old lists: let it finish before they go
        if (sl.route && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        (void)hipFree(sl.route);
        sl.route = nullptr;
        sl.route_cap = 0;
        const size_t cap = n + (n >> 2) + 1024;
        if ((e = hipMalloc((void **)&sl.route, (2 * cap + 4) * 4)) != hipSuccess) return e;
        sl.route_cap = cap;
    }
    *counts = sl.route;
    *sel_inflate = sl.route + 4;
    *sel_zstd = sl.route + 4 + sl.route_cap;
    return hipSuccess;
}

// (caller holds g_slots.mu) out_size == nullptr: the decoder; else the size pass.  The size pass shares the decoder's slot of
// (device, stream): launches on a stream run in order, so the token scratch serves both (the sizes kernels need no more LDS or
// registers than inflate_kernel: the slot's resident-wave count holds for them too).
hipError_t launch_inflate_locked(const BatchArgs &a, uint64_t *out_size, hipStream_t stream)
{
    LaunchSlot *sl = nullptr;
    hipError_t e = slot_for(stream, a.n, sl);
    if (e != hipSuccess) return e;
    uint32_t blocks = a.n < (uint32_t)sl->blocks ? a.n : (uint32_t)sl->blocks;
#ifdef CHIP_EXP_EVEN_GRID  // probe (decode only): as many waves as give every wave the same number of units (no ragged last round)
    if (blocks && !out_size) {
        const uint32_t per_wave = (a.n + blocks - 1) / blocks;
        blocks = (a.n + per_wave - 1) / per_wave;
    }
#endif
    if ((e = hipMemsetAsync(sl->counter, 0, 4, stream)) != hipSuccess) return e;
    if (a.flags & F_MEMBERS) return enqueue_inflate_members(a, out_size, (uint32_t *)sl->scratch, sl->counter, blocks, stream);
    if (out_size) return enqueue_inflate_sizes(a, out_size, (uint32_t *)sl->scratch, sl->counter, blocks, stream);
    hipLaunchKernelGGL(inflate_kernel, dim3(blocks), dim3(64), 0, stream, a, (uint32_t *)sl->scratch, sl->counter);
    return hipGetLastError();
}
}  // namespace

// A CHIP_FMT_DETECT batch: the router's lists and counters belong to (device, stream), so taking them, the counters' reset, the
// router and both decoders' launches are ONE critical section -- another host thread's routed batch on the same stream cannot put
// its reset or its router between this batch's router and this batch's decoders (which would then read the other batch's lists),
// nor free lists that these launches are about to read.  Replaces the routing of src/decoder/mod.rs:28-114 for a whole batch.
// With out_size the same critical section holds the size kernels behind the router.
hipError_t launch_routed(const BatchArgs &a, uint64_t *out_size, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    std::lock_guard<std::mutex> lk(g_slots.mu);
    uint32_t *sel_i = nullptr, *sel_z = nullptr, *counts = nullptr;
    hipError_t e = route_scratch_locked(stream, a.n, &sel_i, &sel_z, &counts);
    if (e == hipSuccess) e = launch_route(a, out_size, sel_i, sel_z, counts, stream);
    BatchArgs ai = a, az = a;
    ai.format = CHIP_FMT_AUTO;
    ai.sel = sel_i;
    ai.sel_n = counts;
    az.format = CHIP_FMT_ZSTD;
    az.sel = sel_z;
    az.sel_n = counts + 1;
    if (e == hipSuccess) e = launch_inflate_locked(ai, out_size, stream);
    if (e == hipSuccess) e = launch_zstd(az, out_size, 0, stream);
    return e;
}

hipError_t launch_inflate(const BatchArgs &a, uint64_t *out_size, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    // One lock from the slot's lookup to the launch: a second host thread that launches a larger batch on the same stream may
    // free and reallocate the scratch in slot_for(); it must not do so between this thread's lookup and its launch (the
    // stream synchronisation in slot_for() only covers work that is already queued).  The counter reset and the kernel also
    // have to reach the stream back to back.
    std::lock_guard<std::mutex> lk(g_slots.mu);
    return launch_inflate_locked(a, out_size, stream);
}

}  // namespace chip
