// Batched LZ4 decode for gfx950 (MI355X): lz4_kernel and lz4_sizes_kernel, one wave per unit (a raw block or a frame), and the one
// launch path of both.  The device code is lz4_unit.h; neither kernel needs launch scratch.  Beside them chip_xxh32_batch, the
// XXH32 of many device ranges, and the host block decoder's C entry point.
#include "lz4_unit.h"

namespace chip {

namespace {

__global__ __launch_bounds__(64) void lz4_kernel(BatchArgs a) { lz4_unit<false>(a, nullptr); }
__global__ __launch_bounds__(64) void lz4_sizes_kernel(BatchArgs a, uint64_t *out_size) { lz4_unit<true>(a, out_size); }

// one wave per range
__global__ __launch_bounds__(64) void xxh32_batch_kernel(const uint8_t *base, const uint64_t *off, const uint32_t *len, uint32_t seed, uint32_t *digest)
{
    __shared__ uint32_t stage[LZ4_STAGE];
    const uint32_t h = wave_xxh32(stage, base + off[blockIdx.x], len[blockIdx.x], seed);
    if (lane_id() == 0) digest[blockIdx.x] = h;
}

// one range of any length (64-bit) on one wave
__global__ __launch_bounds__(64) void xxh32_one_kernel(const uint8_t *p, uint64_t n, uint32_t *got)
{
    __shared__ uint32_t stage[LZ4_STAGE];
    const uint32_t h = wave_xxh32(stage, p, n, 0);
    if (lane_id() == 0) *got = h;
}

}  // namespace

// out_size == nullptr: the decoder; else the size pass
hipError_t launch_lz4(const BatchArgs &a, uint64_t *out_size, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    if (out_size) hipLaunchKernelGGL(lz4_sizes_kernel, dim3(a.n), dim3(64), 0, stream, a, out_size);
    else hipLaunchKernelGGL(lz4_kernel, dim3(a.n), dim3(64), 0, stream, a);
    return hipGetLastError();
}

// the content checksum of chip_lz4_parallel: XXH32, seed 0, of n bytes on one wave, to *got (device memory)
hipError_t launch_lz4_xxh(const uint8_t *p, uint64_t n, uint32_t *got, hipStream_t stream)
{
    hipLaunchKernelGGL(xxh32_one_kernel, dim3(1), dim3(64), 0, stream, p, n, got);
    return hipGetLastError();
}

}  // namespace chip

using namespace chip;

extern "C" {

int chip_lz4_block_decode_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used)
{
    if (!out_len || !in_used || (len && !in) || (cap && !out) || len > 0xFFFFFFFFull || cap > 0xFFFFFFFFull) return CHIP_E_INVALID;
    return lz4::block_decode_host(in, (uint32_t)len, out, cap, *out_len, *in_used);
}

int chip_xxh32_batch(size_t n, const void *base, const uint64_t *off, const uint32_t *len, uint32_t seed, uint32_t *digest, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if ((uint64_t)n > 0x7fffffffull || (n && (!base || !off || !len || !digest))) return CHIP_E_INVALID;
    if (n == 0) return CHIP_OK;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) return CHIP_E_NO_DEVICE;
    hipLaunchKernelGGL(xxh32_batch_kernel, dim3((uint32_t)n), dim3(64), 0, (hipStream_t)stream, (const uint8_t *)base, off, len, seed, digest);
    return hipGetLastError() == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}

}  // extern "C"
