// CHIP_F_MEMBERS for zstd, the size pass: zstd_members_sizes_kernel and its launch.
//
// zstd_unit.h's kernel body compiled with CHIP_ZSTD_SIZES and the frame loop (CHIP_ZSTD_MEMBERS, see there); a translation unit of its
// own as zstd_sizes.hip and zstd_members.hip are.  The launch path is zstd.hip's launch_zstd(), which calls
// enqueue_zstd_members_sizes() here.
#define CHIP_ZSTD_KERNEL zstd_members_sizes_kernel
#define CHIP_ZSTD_SIZES 1
#define CHIP_ZSTD_MEMBERS 1
#include "zstd_unit.h"

namespace chip {

hipError_t enqueue_zstd_members_sizes(const BatchArgs &a, uint64_t *out_size, int wlog_max, hipStream_t stream)
{
    hipLaunchKernelGGL(zstd_members_sizes_kernel, dim3(a.n), dim3(64), 0, stream, a, wlog_max, out_size);
    return hipGetLastError();
}

}  // namespace chip
