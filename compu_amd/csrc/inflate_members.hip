// CHIP_F_MEMBERS for gzip: inflate_members_kernel and inflate_members_sizes_kernel and their launch.
//
// The kernels are inflate_unit.h's unit loop compiled with the member loop (CHIP_INFLATE_MEMBERS, see inflate_unit there): a unit is
// a series of gzip members, decoded one behind the other by the wave that owns the unit; the decoder's and the size pass's persistent
// grids are otherwise inflate_kernel's and inflate_sizes_kernel's.  A translation unit of their own keeps the member loop out of
// those two kernels.  The host side (scratch slot, lock, launch order) is in inflate.hip, whose launcher calls
// enqueue_inflate_members() here.
#define CHIP_INFLATE_MEMBERS 1
#include "inflate_unit.h"

namespace chip {

// (the grid loop is written out as in inflate_kernel, for the reason given there)
__global__ __launch_bounds__(64, CHIP_WAVES_PER_SIMD) void inflate_members_kernel(BatchArgs a, uint32_t *scratch, uint32_t *next_unit)
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
__global__ __launch_bounds__(64, CHIP_WAVES_PER_SIMD) void inflate_members_sizes_kernel(BatchArgs a, uint64_t *out_size, uint32_t *scratch, uint32_t *next_unit)
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
        inflate_unit<true>(a, u, L, grow, out_size);
        WSYNC();
    }
}

// out_size != nullptr launches the size pass, else the decoder
hipError_t enqueue_inflate_members(const BatchArgs &a, uint64_t *out_size, uint32_t *scratch, uint32_t *counter, uint32_t blocks, hipStream_t stream)
{
    if (out_size) hipLaunchKernelGGL(inflate_members_sizes_kernel, dim3(blocks), dim3(64), 0, stream, a, out_size, scratch, counter);
    else hipLaunchKernelGGL(inflate_members_kernel, dim3(blocks), dim3(64), 0, stream, a, scratch, counter);
    return hipGetLastError();
}

}  // namespace chip
