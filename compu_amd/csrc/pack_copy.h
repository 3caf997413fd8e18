// The destination-driven copy of the file writer (file_write.hip), shared with the range reader
// (read_ranges.hip, sec. 4.14): ranges of one device buffer land end to end in another.  One wave per PACK_TILE bytes of
// destination, cut at absolute addresses that are multiples of 16.  The wave finds the unit that holds the tile's first byte with a
// binary search over the offsets, then walks the units that intersect the tile, their offsets and lengths loaded 64 units at a
// time; each intersection is byte stores up to the first 16-byte aligned destination address, aligned 16-byte stores fed by
// unaligned 16-byte loads, byte stores for the rest.  A destination byte belongs to exactly one tile and is written once, by that
// tile's wave; no store is wider than its bytes, so no wave ever touches a 16-byte granule's bytes that belong to another.  The
// copy writes dst[0 .. total) only, whatever the arrays hold by then: every store is clipped to its tile, and the tiles end at the
// total the host compared with the room.  Everything sits in an anonymous namespace, as in plan_common.h: each translation unit
// gets a kernel of its own.
#pragma once
#include "chip_internal.h"

namespace chip {

namespace {

typedef uint32_t pk_u32x4 __attribute__((ext_vector_type(4)));
typedef pk_u32x4 pk_u32x4_u __attribute__((aligned(1)));  // 16 bytes at any address (gfx950 does unaligned global loads)

// Destination bytes per wave: 4 rounds of 64 lanes x 16 bytes, all four loads of a lane issued before its first store.  With
// 16 waves resident per CU that is 64 KiB of loads in flight per CU, the amount that hides most of an HBM miss on this chip;
// a larger tile adds nothing to that and makes the many-small-units case walk more units per wave.
constexpr uint32_t PACK_TILE = 4096;
constexpr uint32_t PACK_ROUNDS = PACK_TILE / (64 * 16);
constexpr uint32_t PACK_WAVES = 4;  // waves (tiles) per workgroup

__device__ __forceinline__ uint64_t rdfirst64(uint64_t v) { return ((uint64_t)rdfirst((uint32_t)(v >> 32)) << 32) | rdfirst((uint32_t)v); }

// `chunks` >= 1 aligned 16-byte stores at db fed by unaligned 16-byte loads at sb, R rounds of 64 lanes.  No load sits under an exec
// mask (a lane behind the last chunk loads that chunk again), so all of a lane's loads are in flight before its first store.
template <uint32_t R>
__device__ __forceinline__ void copy_chunks(const uint8_t *sb, uint8_t *db, uint32_t chunks, uint32_t lane)
{
    pk_u32x4 v[R];
#pragma unroll
    for (uint32_t k = 0; k < R; k++) {
        const uint32_t c = lane + 64u * k;
        v[k] = *(const pk_u32x4_u *)(sb + 16u * (c < chunks ? c : chunks - 1u));
    }
#pragma unroll
    for (uint32_t k = 0; k < R; k++) {
        const uint32_t c = lane + 64u * k;
        if (c < chunks) *(pk_u32x4 *)(db + 16u * c) = v[k];
    }
}

// cnt <= PACK_TILE bytes from src to dst, by the whole wave; src, dst and cnt are wave-uniform
__device__ __forceinline__ void copy_span(const uint8_t *src, uint8_t *dst, uint32_t cnt, uint32_t lane)
{
    uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
    head = head < cnt ? head : cnt;
    const uint8_t *sb = src + head;
    uint8_t *db = dst + head;  // 16-byte aligned (or cnt == head)
    const uint32_t chunks = (cnt - head) >> 4, tail = (cnt - head) & 15u;
    // head and tail: lanes 0..14 the bytes in front of the first chunk, lanes 16..30 those behind the last
    const uint32_t edge = lane < 16u ? lane : head + 16u * chunks + (lane - 16u);
    const bool on_edge = lane < 16u ? lane < head : lane - 16u < tail;
    uint8_t eb = 0;
    if (on_edge) eb = src[edge];
    if (chunks > 64u) copy_chunks<PACK_ROUNDS>(sb, db, chunks, lane);  // (uniform)
    else if (chunks) copy_chunks<1>(sb, db, chunks, lane);
    if (on_edge) dst[edge] = eb;
}

__global__ __launch_bounds__(64 * PACK_WAVES) void pack_copy_kernel(const uint8_t *src_base, const uint64_t *src_off, const uint32_t *src_len,
                                                                    uint8_t *dst_base, const uint64_t *__restrict__ dst_off, uint32_t n, uint64_t total)
{
    const uint32_t lane = lane_id();
    const uint64_t t = (uint64_t)blockIdx.x * PACK_WAVES + rdfirst(threadIdx.x >> 6);
    // tile t in destination offsets: absolute addresses [A + t * PACK_TILE, + PACK_TILE) with A = dst_base rounded down to 16
    const uint32_t mis = (uint32_t)((uintptr_t)dst_base & 15u);
    const uint64_t lo = t ? t * PACK_TILE - mis : 0;
    uint64_t hi = (t + 1) * PACK_TILE - mis;
    hi = hi < total ? hi : total;
    if (lo >= total) return;  // (uniform) the last workgroup's spare waves
    // the last unit that starts at or in front of lo: the one that holds byte lo (empty units at lo sit in front of it)
    uint32_t u = 0, b = n;  // dst_off[u] <= lo, and dst_off[b] > lo or b == n
    while (b - u > 1u) {
        const uint32_t mid = u + ((b - u) >> 1);
        if (rdfirst64(dst_off[mid]) <= lo) u = mid;
        else b = mid;
    }
    // the units that intersect the tile, 64 at a time: lane j holds unit u + j, one round trip for all of them
    for (uint64_t first = u;; first += 64u) {  // (64-bit: n may be 2^32 - 1)
        const uint64_t uj = first + lane;
        uint64_t d_v = ~0ull, so_v = 0;
        uint32_t len_v = 0;
        if (uj < n) d_v = dst_off[uj], so_v = src_off[uj], len_v = src_len[uj];
        const uint32_t here = (uint32_t)__popcll(__ballot(d_v < hi));  // (the offsets ascend: a prefix of the lanes)
        for (uint32_t j = 0; j < here; j++) {
            const uint64_t d = ((uint64_t)rdlane((uint32_t)(d_v >> 32), j) << 32) | rdlane((uint32_t)d_v, j);
            const uint64_t so = ((uint64_t)rdlane((uint32_t)(so_v >> 32), j) << 32) | rdlane((uint32_t)so_v, j);
            const uint64_t s = d > lo ? d : lo, end = d + rdlane(len_v, j), e = end < hi ? end : hi;
            if (e > s) copy_span(src_base + so + (s - d), dst_base + s, (uint32_t)(e - s), lane);
        }
        if (here < 64u) break;
    }
}

// only enqueues; total > 0 and total <= the room behind dst_base  ([[maybe_unused]]: inflate_index.hip takes copy_span only)
[[maybe_unused]] void enqueue_copy(uint64_t n, const uint8_t *src_base, const uint64_t *src_off, const uint32_t *src_len, uint8_t *dst_base, const uint64_t *off,
                  uint64_t total, hipStream_t stream)
{
    const uint64_t tiles = (total + ((uintptr_t)dst_base & 15u) + PACK_TILE - 1) / PACK_TILE;
    hipLaunchKernelGGL(pack_copy_kernel, dim3((uint32_t)((tiles + PACK_WAVES - 1) / PACK_WAVES)), dim3(64 * PACK_WAVES), 0, stream, src_base, src_off,
                       src_len, dst_base, off, (uint32_t)n, total);
}

}  // namespace

}  // namespace chip
