// Batched zstd frame decode for gfx950 (MI355X): zstd_kernel, one wave per frame, and the one launch path of every batched zstd
// decode and size pass.  The device code is zstd_unit.h, compiled here with no variant flag set; the kernels beside this one are in
// zstd_sizes.hip, zstd_members.hip and zstd_members_sizes.hip, which this file's launcher reaches through their enqueue functions
// (zstd_tokens.hip's kernel is chip_zstd_parallel's and has a launcher of its own).
#define CHIP_ZSTD_KERNEL zstd_kernel
#include "zstd_unit.h"

namespace chip {

// out_size == nullptr: the decoder; else the size pass.  window_log_max 0 = 27, the limit of a decoder built without options.
hipError_t launch_zstd(const BatchArgs &a, uint64_t *out_size, int window_log_max, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const int wlog_max = window_log_max ? window_log_max : 27;
    if (a.flags & F_MEMBERS) return out_size ? enqueue_zstd_members_sizes(a, out_size, wlog_max, stream) : enqueue_zstd_members(a, wlog_max, stream);
    if (out_size) return enqueue_zstd_sizes(a, out_size, wlog_max, stream);
    hipLaunchKernelGGL(zstd_kernel, dim3(a.n), dim3(64), 0, stream, a, wlog_max);
    return hipGetLastError();
}

}  // namespace chip
