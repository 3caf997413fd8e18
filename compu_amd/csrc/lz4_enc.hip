// LZ4 encoder for gfx950 (MI355X): one wavefront encodes one unit into one raw block (CHIP_FMT_LZ4_BLOCK) or one frame
// (CHIP_FMT_LZ4) -- two compile modes of one body.  Persistent grid: each wave takes the next unit from a counter.  Everything that
// decides a byte is lz4_enc_core.h, the same templates the host forms run (chip_lz4_block_encode_host and
// chip_lz4_frame_encode_host define the bytes); this file adds the lanes of a wavefront, the LDS and the launch.
// LDS per wave: the hash table (16 KiB), the chunk's six rows (1.5 KiB) and, for frames, the XXH32 staging of lz4_unit.h (2 KiB):
// 9 waves per CU for blocks, 8 for frames; the registers (73 / 74 VGPRs, no scratch) would allow more.
#include <mutex>

#include "chip_internal.h"
#include "launch_slots.h"
#include "lz4_enc_core.h"
#include "lz4_unit.h"

namespace chip {

namespace {

struct LEncArgs {
    BatchArgs b;
    lz4enc::Cfg cfg;
    uint32_t opts;  // CHIP_LZ4_S_* (frames)
};

template <bool FRAME>
struct alignas(16) LEncLds {
    uint16_t ht[lz4enc::HSIZE];
    lz4enc::Chunk k;
    uint32_t stage[FRAME ? LZ4_STAGE : 4];  // XXH32 staging: frames only
};

// the lanes of lz4_enc_core.h's templates on a wavefront: a per-lane step runs on its lane, an LDS wait ends it
struct WaveLanes {
    static constexpr uint32_t stride = 64;
    uint32_t *stage;
    __device__ __forceinline__ uint32_t lane() const { return lane_id(); }
    template <class F>
    __device__ __forceinline__ void each(F f) const
    {
        f(lane_id());
        LSYNC();
    }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return rdfirst(v); }
    __device__ __forceinline__ void sync() const { LSYNC(); }
    __device__ __forceinline__ void fence() const
    {
        __threadfence();
        WSYNC();
    }
    __device__ __forceinline__ uint32_t xxh32(const uint8_t *p, uint64_t n) const { return wave_xxh32(stage, p, n, 0); }
};

template <bool FRAME>
__device__ __forceinline__ void lz4_enc_unit(const LEncArgs &a, uint32_t u, LEncLds<FRAME> &L)
{
    const uint32_t lane = lane_id();
    const uint32_t n = rdfirst(a.b.in_len[u]), cap = rdfirst(a.b.out_cap[u]);
    if (n > lz4enc::MAX_UNIT) {
        if (lane == 0) {
            a.b.out_len[u] = 0;
            a.b.status[u] = CHIP_ENC_ERROR;
        }
        return;
    }
    const uint8_t *src = rdfirst_ptr(a.b.in_base + a.b.in_off[u]);
    zenc::Out o = {rdfirst_ptr(a.b.out_base + a.b.out_off[u]), 0, cap, false};
    const WaveLanes ln{L.stage};
    if (FRAME) lz4enc::frame_encode(ln, a.cfg, a.opts, L.ht, L.k, src, n, o);
    else lz4enc::block_encode(ln, a.cfg, L.ht, L.k, src, n, o);
    if (lane == 0) {
        a.b.out_len[u] = o.ovf ? 0u : o.pos;
        a.b.status[u] = o.ovf ? CHIP_ENC_NEED_OUTPUT : CHIP_ENC_FINISHED;
    }
}

template <bool FRAME>
__global__ __launch_bounds__(64) void lz4_enc_kernel(LEncArgs a, uint32_t *next_unit)
{
    __shared__ LEncLds<FRAME> L;
    for (;;) {
        uint32_t i = 0;
        if (lane_id() == 0) i = atomicAdd(next_unit, 1u);
        i = rdfirst(i);
        if (i >= a.b.n) break;
        lz4_enc_unit<FRAME>(a, i, L);
        WSYNC();  // the next unit reuses the LDS
    }
}

// the unit counter: a launch slot without per-wave scratch ("Launch slots")
SlotCache<WaveScratch> g_lenc_cache;
ResidentWaves g_lenc_resident[2];

template <bool FRAME>
hipError_t launch(const LEncArgs &a, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(g_lenc_cache.mu);  // from the slot's lookup to the launch
    WaveScratch *sl = nullptr;
    int max_blocks = 0;
    hipError_t e = g_lenc_cache.at(stream, sl);
    if (e == hipSuccess) e = g_lenc_resident[FRAME].get((const void *)lz4_enc_kernel<FRAME>, max_blocks);
    if (e == hipSuccess) e = sl->reserve(stream, a.b.n, max_blocks, 0);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(sl->counter, 0, 4, stream)) != hipSuccess) return e;
    const uint32_t blocks = a.b.n < (uint32_t)max_blocks ? a.b.n : (uint32_t)max_blocks;
    hipLaunchKernelGGL(lz4_enc_kernel<FRAME>, dim3(blocks), dim3(64), 0, stream, a, sl->counter);
    return hipGetLastError();
}

}  // namespace

bool lz4_encode_args_ok(int format, int level, int strategy)
{
    lz4enc::Cfg c;
    if (!lz4enc::level_cfg(level, c)) return false;
    return format == CHIP_FMT_LZ4 ? lz4enc::frame_opts_ok(strategy) : strategy == 0;
}

hipError_t launch_lz4_encode(const BatchArgs &b, int level, int strategy, hipStream_t stream)
{
    if (b.n == 0) return hipSuccess;
    LEncArgs a;
    a.b = b;
    a.opts = (uint32_t)strategy;
    if (!lz4enc::level_cfg(level, a.cfg)) return hipErrorInvalidValue;
    return b.format == CHIP_FMT_LZ4 ? launch<true>(a, stream) : launch<false>(a, stream);
}

}  // namespace chip

using namespace chip;

extern "C" {

int chip_lz4_block_encode_host(const uint8_t *in, uint64_t len, int level, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
    lz4enc::Cfg c;
    if (!out_len || (len && !in) || (cap && !out) || !lz4enc::level_cfg(level, c)) return CHIP_E_INVALID;
    return lz4enc::block_encode_host(in, len, c, out, cap, *out_len);
}

int chip_lz4_frame_encode_host(const uint8_t *in, uint64_t len, int level, int strategy, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
    lz4enc::Cfg c;
    if (!out_len || (len && !in) || (cap && !out) || !lz4enc::level_cfg(level, c) || !lz4enc::frame_opts_ok(strategy)) return CHIP_E_INVALID;
    return lz4enc::frame_encode_host(in, len, c, (uint32_t)strategy, out, cap, *out_len);
}

}  // extern "C"
