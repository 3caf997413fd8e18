// The size pass of the batched inflate (chip_decode_batch_sizes): inflate_sizes_kernel and its launch.
//
// The kernel is inflate_unit.h's unit loop instantiated without the LZ77 executor (inflate_unit<true>: wrapper, block headers, table
// builds, walk and path resolve as they are, count_tokens() in place of flush_tokens()): the same persistent grid over the same
// scratch slot as inflate_kernel, no output.  It has a translation unit of its own because a second kernel beside inflate_kernel
// changes the compiler's inlining of the functions both call and with it inflate_kernel's register allocation.  The host side
// (scratch slot, lock, launch order) is in inflate.hip, whose launcher calls enqueue_inflate_sizes() here.
#include "inflate_unit.h"

namespace chip {

// (the grid loop is written out as in inflate_kernel, for the reason given there)
__global__ __launch_bounds__(64, CHIP_WAVES_PER_SIMD) void inflate_sizes_kernel(BatchArgs a, uint64_t *out_size, uint32_t *scratch, uint32_t *next_unit)
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
        WSYNC();  // the next unit reuses the LDS
    }
}

hipError_t enqueue_inflate_sizes(const BatchArgs &a, uint64_t *out_size, uint32_t *scratch, uint32_t *counter, uint32_t blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(inflate_sizes_kernel, dim3(blocks), dim3(64), 0, stream, a, out_size, scratch, counter);
    return hipGetLastError();
}

}  // namespace chip
