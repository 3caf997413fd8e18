// What the container plans (bgzf.hip, zstd_plan.hip) have in common: the tile geometry of the
// candidate search, the chunk loader, the reduce-then-scan kernels, the doubling and marking kernels over a successor table,
// and the growing device buffer of their slots.  The file writer (file_write.hip, sec. 4.13) takes the scans and the buffer.
// Everything sits in an anonymous namespace, as it did inside bgzf.hip: each translation unit gets kernels of its own, and
// nothing here is seen from outside them.
#pragma once
#include "chip_internal.h"

namespace chip {

namespace {

constexpr uint32_t TILE_THREADS = 256, TILE_ITERS = 4;
constexpr uint32_t TILE_CHUNKS = TILE_THREADS * TILE_ITERS;  // 16-byte chunks per workgroup: a 16 KiB tile
constexpr uint32_t SCAN_THREADS = 1024;

// The scans are templated on the sum type T: T{} is the zero, operator+ and shfl_up_t(T, d) are found at the instantiation.
__device__ __forceinline__ uint64_t shfl_up_t(uint64_t v, uint32_t d) { return __shfl_up((unsigned long long)v, d, 64); }

// inclusive scan across the wave (Hillis-Steele over ds_bpermute; the 64-bit sums have no DPP form)
template <class T>
__device__ __forceinline__ T wave_incl_scan_t(T v)
{
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T t = shfl_up_t(v, d);
        if (lane >= d) v = v + t;
    }
    return v;
}

// exclusive scan across a workgroup of SCAN_THREADS; s_wave has SCAN_THREADS / 64 + 1 entries; every thread takes part
template <class T>
__device__ __forceinline__ T block_excl_scan(const T v, T *s_wave, T &total)
{
    constexpr uint32_t NW = SCAN_THREADS / 64;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const T inc = wave_incl_scan_t(v);
    T exc = shfl_up_t(inc, 1);
    if (lane == 0) exc = T{};
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run{};
        for (uint32_t w = 0; w < NW; w++) {
            const T t = s_wave[w];
            s_wave[w] = run;
            run = run + t;
        }
        s_wave[NW] = run;
    }
    __syncthreads();
    const T r = s_wave[wave] + exc;
    total = s_wave[NW];
    __syncthreads();  // s_wave is free again
    return r;
}

// out[i] = sum of in[b * SCAN_THREADS .. i) for the workgroup b that holds i; partial[b] = the workgroup's total
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void plan_scan_local_kernel(const T *in, T *out, uint64_t n, T *partial)
{
    __shared__ T s_wave[SCAN_THREADS / 64 + 1];
    const uint64_t i = (uint64_t)blockIdx.x * SCAN_THREADS + threadIdx.x;
    T total;
    const T r = block_excl_scan(i < n ? in[i] : T{}, s_wave, total);
    if (i < n) out[i] = r;
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: partial[0 .. nb) becomes its exclusive scan, *total the sum
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void plan_scan_partials_kernel(T *partial, uint64_t nb, T *total)
{
    __shared__ T s_wave[SCAN_THREADS / 64 + 1];
    T carry{};
    for (uint64_t b0 = 0; b0 < nb; b0 += SCAN_THREADS) {
        const uint64_t i = b0 + threadIdx.x;
        T t;
        const T r = block_excl_scan(i < nb ? partial[i] : T{}, s_wave, t);
        if (i < nb) partial[i] = carry + r;
        carry = carry + t;
    }
    if (threadIdx.x == 0) *total = carry;
}

struct __attribute__((packed, aligned(4))) Chunk16 {
    uint32_t w[4];
};

// the 16 bytes of chunk g and the 4 behind them (in_base is 4-byte aligned and padded to len4 = len rounded up to 4; nothing
// outside [0, len4) is read, what lies beyond reads as 0)
__device__ __forceinline__ void load_chunk(const uint8_t *base, uint64_t len4, uint64_t g, uint32_t w[5])
{
    const uint64_t b = g * 16;
    if (b + 20 <= len4) {
        const Chunk16 v = *(const Chunk16 *)(base + b);
        w[0] = v.w[0], w[1] = v.w[1], w[2] = v.w[2], w[3] = v.w[3];
        w[4] = *(const uint32_t *)(base + b + 16);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) w[k] = b + 4 * k + 4 <= len4 ? *(const uint32_t *)(base + b + 4 * k) : 0u;
    }
}

// the four bytes at offset k (0..15) of a loaded chunk, little endian
__device__ __forceinline__ uint32_t chunk_word(const uint32_t w[5], uint32_t k)
{
    const uint32_t lo = w[k >> 2], hi = w[(k >> 2) + 1], sh = 8 * (k & 3);
    return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
}

// jump table k + 1 = jump table k applied twice; n_cand is the sink  ([[maybe_unused]]: file_write.hip takes the scans only)
[[maybe_unused]] __global__ __launch_bounds__(256) void plan_double_kernel(const uint32_t *jump, uint32_t *jump2, uint32_t n_cand)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    const uint32_t j = jump[i];
    jump2[i] = j < n_cand ? (jump[j] < n_cand ? jump[j] : n_cand) : n_cand;
}

// One level of the top-down marking.  A candidate marked by another thread of this very launch may or may not hand its mark
// on at once: either way only candidates on the chain from 0 get one, and those marked before the launch all hand it on.
[[maybe_unused]] __global__ __launch_bounds__(256) void plan_mark_kernel(const uint32_t *jump, uint32_t *marked, uint32_t n_cand)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand || !marked[i]) return;
    const uint32_t j = jump[i];
    if (j < n_cand) marked[j] = 1u;
}

// first candidate of pos[lo .. n_cand) at or behind nx, if it sits exactly there; else the sink
__device__ __forceinline__ uint32_t candidate_at(const uint64_t *pos, uint32_t lo, uint32_t n_cand, uint64_t nx)
{
    uint32_t hi = n_cand;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (pos[mid] < nx) lo = mid + 1u;
        else hi = mid;
    }
    return lo < n_cand && pos[lo] == nx ? lo : n_cand;
}

// 2^levels > n_cand: every distance on a chain of candidates has its bits below `levels`
inline uint32_t jump_levels(uint32_t n_cand)
{
    uint32_t levels = 1;
    while (levels < 32 && (1ull << levels) <= n_cand) levels++;
    return levels;
}

// A device buffer of a plan's slot that only grows (the call that used it last has waited for the stream, under the cache's
// lock: nothing in flight reads it)
inline hipError_t grow_buffer(uint8_t *&p, size_t &cap, size_t want)
{
    if (cap >= want) return hipSuccess;
    (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t take = want + want / 4;
    const hipError_t e = hipMalloc((void **)&p, take);
    if (e == hipSuccess) cap = take;
    return e;
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

}  // namespace chip
