// The token pass of chip_zstd_parallel: zstd_tokens_kernel and its launch, and the XXH64 of the delivered content.
//
// The kernel is zstd.hip's kernel body compiled with CHIP_ZSTD_TOKENS set (see there): headers, table builds, literal decode and the
// FSE state chain are that file's source, not a copy.  It has a translation unit of its own for the reason zstd_sizes.hip has one.
// zpar_xxh_kernel is here because xxh_stripes / xxh_finish are that file's too.
#define CHIP_ZSTD_TOKENS 1
#include "zstd.hip"

namespace chip {

namespace {

// one wave: the chain of XXH64's four accumulators cannot be split
__global__ __launch_bounds__(64) void zpar_xxh_kernel(const uint8_t *p, uint32_t n, uint32_t *got)
{
    __shared__ uint64_t stage[128 * 4];
    const uint32_t v = wave_xxh64_low32(stage, p, n);
    if (lane_id() == 0) *got = v;
}

}  // namespace

hipError_t launch_zstd_tokens(const BatchArgs &a, const ZTokArgs &tk, hipStream_t stream)
{
    hipLaunchKernelGGL(zstd_tokens_kernel, dim3(a.n), dim3(64), 0, stream, a, 31, tk);
    return hipGetLastError();
}

hipError_t launch_zstd_xxh(const uint8_t *p, uint32_t n, uint32_t *got, hipStream_t stream)
{
    hipLaunchKernelGGL(zpar_xxh_kernel, dim3(1), dim3(64), 0, stream, p, n, got);
    return hipGetLastError();
}

}  // namespace chip
