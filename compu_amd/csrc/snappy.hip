// Batched Snappy decode for gfx950 (MI355X): snappy_kernel and snappy_sizes_kernel, one wave per unit (a raw block or a framed
// stream), and the one launch path of both.  The device code is snappy_unit.h; neither kernel needs launch scratch.  Beside them
// chip_crc32c_batch, the CRC-32C of many device ranges, and the host block decoder's C entry point.
#include "snappy_unit.h"

namespace chip {

namespace {

__global__ __launch_bounds__(64) void snappy_kernel(BatchArgs a) { snappy_unit<false>(a, nullptr); }
__global__ __launch_bounds__(64) void snappy_sizes_kernel(BatchArgs a, uint64_t *out_size) { snappy_unit<true>(a, out_size); }

// one wave per range
__global__ __launch_bounds__(64) void crc32c_batch_kernel(const uint8_t *base, const uint64_t *off, const uint32_t *len, uint32_t *crc)
{
    __shared__ uint32_t tab[1024];
    snappy_crc_tables((LDS_AS uint32_t *)tab);
    const uint32_t c = wave_crc32c((LDS_AS uint32_t *)tab, base + off[blockIdx.x], len[blockIdx.x]);
    if (lane_id() == 0) crc[blockIdx.x] = c;
}

}  // namespace

// out_size == nullptr: the decoder; else the size pass
hipError_t launch_snappy(const BatchArgs &a, uint64_t *out_size, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    if (out_size) hipLaunchKernelGGL(snappy_sizes_kernel, dim3(a.n), dim3(64), 0, stream, a, out_size);
    else hipLaunchKernelGGL(snappy_kernel, dim3(a.n), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace chip

using namespace chip;

extern "C" {

int chip_snappy_block_decode_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used)
{
    if (!out_len || !in_used || (len && !in) || (cap && !out) || len > 0xFFFFFFFFull || cap > 0xFFFFFFFFull) return CHIP_E_INVALID;
    return snappy::block_decode_host(in, (uint32_t)len, out, cap, *out_len, *in_used);
}

int chip_crc32c_batch(size_t n, const void *base, const uint64_t *off, const uint32_t *len32, uint32_t *crc, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if ((uint64_t)n > 0x7fffffffull || (n && (!base || !off || !len32 || !crc))) return CHIP_E_INVALID;
    if (n == 0) return CHIP_OK;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) return CHIP_E_NO_DEVICE;
    hipLaunchKernelGGL(crc32c_batch_kernel, dim3((uint32_t)n), dim3(64), 0, (hipStream_t)stream, (const uint8_t *)base, off, len32, crc);
    return hipGetLastError() == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}

}  // extern "C"
