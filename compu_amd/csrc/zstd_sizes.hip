// The size pass of the batched zstd decode (chip_decode_batch_sizes): zstd_sizes_kernel and its launch.
//
// The kernel is zstd_unit.h's kernel body compiled with CHIP_ZSTD_SIZES (see there): headers, table builds, the FSE state chain, offsets
// and placement checks are that header's source, not a copy.  It has a translation unit of its own because a second kernel beside
// zstd_kernel changes the compiler's inlining of the functions both call; the decoder must come out of the build as it was.  The
// launch path is zstd.hip's launch_zstd(), which calls enqueue_zstd_sizes() here.
#define CHIP_ZSTD_KERNEL zstd_sizes_kernel
#define CHIP_ZSTD_SIZES 1
#include "zstd_unit.h"

namespace chip {

hipError_t enqueue_zstd_sizes(const BatchArgs &a, uint64_t *out_size, int wlog_max, hipStream_t stream)
{
    hipLaunchKernelGGL(zstd_sizes_kernel, dim3(a.n), dim3(64), 0, stream, a, wlog_max, out_size);
    return hipGetLastError();
}

}  // namespace chip
