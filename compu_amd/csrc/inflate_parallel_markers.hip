// The marker decode of chip_inflate_parallel: inflate_markers_kernel and its launch.
//
// The kernel is inflate_unit.h's unit loop compiled with CHIP_INFLATE_MARKERS: header, tables, walk and token rows as they are, and
// flush_tokens16() / wave_copy_stored16() in place of the byte executor.  A unit is one chunk of the chain: it begins at a block
// header inside its first byte, its input ends with the byte that holds the next chunk's first bit, and its output is 16-bit
// elements -- what stands in front of the chunk is not known yet, so a match that reaches there copies a marker instead of a byte.
// A translation unit of its own for the reason inflate_sizes.hip gives: a second kernel beside another changes the first one's code.
#define CHIP_INFLATE_MARKERS 1
#include "inflate_unit.h"

namespace chip {

// (the grid loop is written out as in inflate_kernel)
__global__ __launch_bounds__(64, CHIP_WAVES_PER_SIMD) void inflate_markers_kernel(BatchArgs a, const uint32_t *bit0, uint32_t *scratch, uint32_t *next_unit)
{
    __shared__ WaveLds L;
    uint32_t *grow = scratch + (size_t)blockIdx.x * SCRATCH_WORDS;
    for (;;) {
        uint32_t i = 0;
        if (lane_id() == 0) i = atomicAdd(next_unit, 1u);
        i = rdfirst(i);
        if (i >= a.n) break;
        inflate_unit<false>(a, i, L, grow, nullptr, bit0);
        WSYNC();  // the next unit reuses the LDS
    }
}

hipError_t enqueue_inflate_markers(const BatchArgs &a, const uint32_t *bit0, uint32_t *scratch, uint32_t *counter, uint32_t blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(inflate_markers_kernel, dim3(blocks), dim3(64), 0, stream, a, bit0, scratch, counter);
    return hipGetLastError();
}

}  // namespace chip
