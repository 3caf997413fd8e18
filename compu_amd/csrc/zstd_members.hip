// CHIP_F_MEMBERS for zstd: zstd_members_kernel and its launch.
//
// The kernel is zstd_unit.h's kernel body compiled with the frame loop (CHIP_ZSTD_MEMBERS, see there): a unit is a series of zstd
// frames and skippable frames, decoded one behind the other by the wave that owns the unit.  It has a translation unit of its own for
// the reason zstd_sizes.hip has one: zstd_kernel must come out of the build as it was.  The launch path is zstd.hip's launch_zstd(),
// which calls enqueue_zstd_members() here.
#define CHIP_ZSTD_KERNEL zstd_members_kernel
#define CHIP_ZSTD_MEMBERS 1
#include "zstd_unit.h"

namespace chip {

hipError_t enqueue_zstd_members(const BatchArgs &a, int wlog_max, hipStream_t stream)
{
    hipLaunchKernelGGL(zstd_members_kernel, dim3(a.n), dim3(64), 0, stream, a, wlog_max);
    return hipGetLastError();
}

}  // namespace chip
