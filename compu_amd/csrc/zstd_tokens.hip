// The token pass of chip_zstd_parallel: zstd_tokens_kernel and its launch, and the XXH64 of the delivered content.
//
// The kernel is zstd_unit.h's kernel body compiled with CHIP_ZSTD_TOKENS set (see there): headers, table builds, literal decode and the
// FSE state chain are that header's source, not a copy.  It has a translation unit of its own for the reason zstd_sizes.hip has one.
// zpar_xxh_kernel and zpar_xxh_update_kernel stay here, with their launchers, though zstd_parallel.hip is what launches them: they use
// the header's xxh_stripes / xxh_finish, and zstd_tokens_kernel's inlining depends on sharing its translation unit with them -- with the
// XXH64 functions in a header of their own and the two kernels in zstd_parallel.hip, tools/kernel_diff.py reports zstd_tokens_kernel and
// wave_xxh64_low32 DIFF.
#define CHIP_ZSTD_KERNEL zstd_tokens_kernel
#define CHIP_ZSTD_TOKENS 1
#include "zstd_unit.h"

namespace chip {

namespace {

// one wave: the chain of XXH64's four accumulators cannot be split
__global__ __launch_bounds__(64) void zpar_xxh_kernel(const uint8_t *p, uint32_t n, uint32_t *got)
{
    __shared__ uint64_t stage[128 * 4];
    const uint32_t v = wave_xxh64_low32(stage, p, n);
    if (lane_id() == 0) *got = v;
}

// The running XXH64 of chip_zstd_parallel_next (sec. 4.20) brought forward over p[0 .. n): one wave again.  The state comes by value.
// The stripe that straddles the old tail is put together in LDS and run by lanes 0..3 themselves; the whole stripes behind it are
// xxh_stripes'; what is left becomes the new tail.  A state that has hashed nothing has its accumulators started here.
__global__ __launch_bounds__(64) void zpar_xxh_update_kernel(const uint8_t *p, uint32_t n, chip_xxh64_state st, chip_xxh64_state *out)
{
    __shared__ uint64_t stage[128 * 4];
    __shared__ uint64_t first[4];
    constexpr uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL;
    const uint32_t lane = lane_id(), t = st.tail_n;
    uint64_t acc = st.total == 0 ? xxh_init() : (lane < 4 ? st.acc[lane] : 0ull);
    uint32_t skip = 0;
    if (t + n >= 32 && t) {
        skip = 32 - t;
        if (lane < 32) ((uint8_t *)first)[lane] = lane < t ? st.tail[lane] : p[lane - t];
        WSYNC();
        if (lane < 4) {
            const uint64_t x = acc + first[lane] * P2;
            acc = ((x << 31) | (x >> 33)) * P1;
        }
    }
    uint32_t tail_n, from;  // the new tail: tail_n bytes, the first `keep` of them the old tail's
    const uint32_t keep = t + n < 32 ? t : 0u;
    if (t + n < 32) {
        tail_n = t + n;
        from = 0;
    } else {
        const uint32_t stripes = (n - skip) >> 5;
        if (stripes) xxh_stripes(stage, 128, p + skip, stripes, acc);
        from = skip + (stripes << 5);
        tail_n = n - from;
    }
    if (lane < 4) out->acc[lane] = acc;
    if (lane < 32) out->tail[lane] = lane < keep ? st.tail[lane] : lane < tail_n ? p[from + lane - keep] : (uint8_t)0;
    if (lane == 0) {
        out->total = st.total + n;
        out->tail_n = tail_n;
        out->pad = 0;
    }
}

}  // namespace

hipError_t launch_zstd_xxh_update(const uint8_t *p, uint32_t n, const chip_xxh64_state &st, chip_xxh64_state *out, hipStream_t stream)
{
    hipLaunchKernelGGL(zpar_xxh_update_kernel, dim3(1), dim3(64), 0, stream, p, n, st, out);
    return hipGetLastError();
}

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
