// What the container plans (bgzf.hip, zstd_plan.hip, gzip_plan.hip) have in common, which is everything but the format:
// the tile geometry of the candidate search, the chunk loader, the reduce-then-scan kernels and the helper that enqueues them, the
// plan pipeline as templates over a format policy (count, emit, describe, successor, doubling, marking, flags, output and the
// driver that enqueues them: "The container plan" below), the slot with its two growing buffers and its summary, and the scaffold
// of an entry point (device check, the cache's lock, the slot, the error mapping).  The file writer (file_write.hip, sec. 4.13)
// and the range reader (read_ranges.hip, sec. 4.14) take the scans, the slot and the scaffold.  Everything sits in an anonymous namespace: each translation unit gets kernels of
// its own, and nothing here is seen from outside them.
#pragma once
#include <mutex>
#include <type_traits>

#include "chip_internal.h"
#include "launch_slots.h"

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

inline uint64_t scan_parts(uint64_t n) { return (n + SCAN_THREADS - 1) / SCAN_THREADS; }

// enqueues the exclusive scan of in[0 .. n) into out (in place when out == in): out[i] still lacks part[i / SCAN_THREADS], which
// the kernel behind the scan adds; `part` has scan_parts(n) entries, *total (device memory) gets the sum
template <class T>
inline void enqueue_scan(const T *in, T *out, uint64_t n, T *part, T *total, hipStream_t stream)
{
    const uint64_t parts = scan_parts(n);
    hipLaunchKernelGGL(plan_scan_local_kernel<T>, dim3((uint32_t)parts), dim3(SCAN_THREADS), 0, stream, in, out, n, part);
    hipLaunchKernelGGL(plan_scan_partials_kernel<T>, dim3(1), dim3(SCAN_THREADS), 0, stream, part, parts, total);
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

// jump table k + 1 = jump table k applied twice; n_cand is the sink  ([[maybe_unused]]: file_write.hip and read_ranges.hip take the scans only)
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

// A device buffer of a slot that only grows (the call that used it last has waited for the stream, under the cache's
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

// The scratch of one (device, stream): two device buffers that only grow, the summary the kernels write and its pinned copy.  A
// launch slot; what the two buffers hold is the business of the code that takes the slot.
template <class DevSummary>
struct SummarySlot {
    uint8_t *buf[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
    DevSummary *d_sum = nullptr, *h_sum = nullptr;

    hipError_t summary()
    {
        hipError_t e = hipSuccess;
        if (!d_sum) e = hipMalloc((void **)&d_sum, sizeof(DevSummary));
        if (e == hipSuccess && !h_sum) e = hipHostMalloc((void **)&h_sum, sizeof(DevSummary), hipHostMallocDefault);
        return e;
    }
    hipError_t grow(uint32_t k, size_t want) { return grow_buffer(buf[k], cap[k], want); }
    // what has been enqueued so far is checked, the summary copied to h_sum and waited for
    hipError_t fetch(hipStream_t stream)
    {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if ((e = hipMemcpyAsync(h_sum, d_sum, sizeof(DevSummary), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        return hipStreamSynchronize(stream);
    }
    void free()
    {
        (void)hipFree(buf[0]);
        (void)hipFree(buf[1]);
        (void)hipFree(d_sum);
        if (h_sum) (void)hipHostFree(h_sum);
    }
};

// What an entry point does once its arguments are in order: looks for a device, locks the cache from the slot's lookup to the
// last launch (and the wait behind it), runs body(slot, stream) with the slot of (current device, stream) and maps its error.  A
// failed body: the stream is waited for (the slot is handed on only with nothing in flight), then failed() resets the caller's
// outputs.
template <class Slot, class Body, class Failed>
int with_slot(SlotCache<Slot> &cache, void *stream, Body body, Failed failed)
{
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) return CHIP_E_NO_DEVICE;
    std::lock_guard<std::mutex> lk(cache.mu);
    Slot *sl = nullptr;
    if (cache.at((hipStream_t)stream, sl) != hipSuccess) return CHIP_E_LAUNCH;
    const hipError_t e = body(*sl, (hipStream_t)stream);
    if (e == hipSuccess) return CHIP_OK;
    (void)hipStreamSynchronize((hipStream_t)stream);
    failed();
    return e == hipErrorOutOfMemory ? CHIP_E_NOMEM : CHIP_E_LAUNCH;
}

// ---- The container plan --------------------------------------------------------------------------------------------------------
// A format F is a struct of constants and static functions, no state:
//   F::MIN_HEADER                              the shortest header: what the walk needs in front of `len` to look at a position
//   F::candidates(base, len, n_chunks, g)      the positions of chunk g that may start a unit, as a 16-bit mask
//   F::describe(base, len, p, gone)            the unit whose header sits at candidate p; gone = p is no candidate (any more)
// and every kernel below that depends on it is instantiated once per format.  A format whose units do not state their length in a
// header a single thread can read supplies the describe phase itself (the policy D of plan_locked, KernelDescribe<F> by default:
// gzip_plan.hip runs the inflate size pass there) and needs no F::describe.  The phases, in stream order:
//   1. count     plan_count_kernel<F>: one count of candidates per 16 KiB tile
//   2. scan      exclusive scan of the tile counts (enqueue_scan)
//      -- the host reads the candidate count and sizes the candidate scratch --
//   3. emit      plan_emit_kernel<F>: tiles with candidates are read again and the positions written in ascending order;
//      describe  D::describe, by default plan_describe_kernel<F>: each candidate's own thread stores the end position, the cap, the
//                verdict and the kind
//   4. succ      plan_succ_kernel<F>: successor of a whole candidate = the candidate at its end position (binary search);
//                everything else leads to the sink (index = number of candidates)
//   5. double    plan_double_kernel: jump table k+1 = jump table k applied twice, ceil(log2(candidates + 1)) tables
//   6. mark      plan_mark_kernel: from candidate 0 (if it sits at position 0) top-down through the tables.  What is never marked
//                is a decoy
//   7. output    plan_flags_kernel, exclusive 64-bit scan of {frames, skippable, unsized, content bytes}, plan_output_kernel<F>:
//                scatter of the frames' rows; the one marked candidate without a successor says where and why the walk stopped;
//                D::finish, by default nothing
// Order between the phases comes from kernel boundaries on the stream only: no workgroup ever waits for another one.  Every index
// is checked against the count it belongs to; data that changes under the kernels sets PlanSummary::fault instead of writing out
// of range.

// the status of a walk that stops at the end, inside a header, at bytes that are no header: the same numbers in both formats
constexpr int32_t PLAN_OK = 0, PLAN_TRUNCATED = 1, PLAN_BAD_HEADER = 2;
static_assert(CHIP_BGZF_OK == PLAN_OK && CHIP_BGZF_TRUNCATED == PLAN_TRUNCATED && CHIP_BGZF_BAD_HEADER == PLAN_BAD_HEADER, "stop_status");
static_assert(CHIP_ZPLAN_OK == PLAN_OK && CHIP_ZPLAN_TRUNCATED == PLAN_TRUNCATED && CHIP_ZPLAN_BAD_HEADER == PLAN_BAD_HEADER, "stop_status");
static_assert(CHIP_GZPLAN_OK == PLAN_OK && CHIP_GZPLAN_TRUNCATED == PLAN_TRUNCATED && CHIP_GZPLAN_BAD_HEADER == PLAN_BAD_HEADER, "stop_status");

constexpr uint32_t KIND_FRAME = 0, KIND_SKIP = 1;  // a unit of the batch / a unit that is stepped over and counted

struct Described {
    uint64_t end;      // position behind the unit (verdict 0 only)
    uint32_t cap;      // decoded size, or CHIP_ZPLAN_UNSIZED (KIND_SKIP: 0)
    uint32_t verdict;  // 0 a whole unit, else the status the walk stops with at p
    uint32_t kind;
};

// what the walk answers where no unit starts at e (the end of the last unit, or 0)
template <class F>
__host__ __device__ __forceinline__ int32_t stop_status(uint64_t len, uint64_t e)
{
    return e == len ? PLAN_OK : len - e < F::MIN_HEADER ? PLAN_TRUNCATED : PLAN_BAD_HEADER;
}

struct PlanAcc {
    uint64_t frames, skips, unsized, bytes;  // marked whole candidates of each kind, the frames without a size, the decoded sizes
};
__host__ __device__ __forceinline__ PlanAcc operator+(const PlanAcc &a, const PlanAcc &b)
{
    return PlanAcc{a.frames + b.frames, a.skips + b.skips, a.unsized + b.unsized, a.bytes + b.bytes};
}
__device__ __forceinline__ PlanAcc shfl_up_t(const PlanAcc &v, uint32_t d)
{
    return PlanAcc{shfl_up_t(v.frames, d), shfl_up_t(v.skips, d), shfl_up_t(v.unsized, d), shfl_up_t(v.bytes, d)};
}

// what the kernels hand to the host (device memory, copied back once the candidates are counted and once at the end)
struct PlanSummary {
    PlanAcc sum;  // total of the output scan
    uint64_t in_used;
    int32_t status;
    uint32_t fault;     // a kernel met data that contradicts an earlier pass
    uint64_t cand;      // total of the tile scan: number of candidates
    uint32_t last_cap;  // cap of the last frame of the walk
    uint32_t pad;
};

template <class F>
__global__ __launch_bounds__(TILE_THREADS) void plan_count_kernel(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t *tile_cnt)
{
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t it = 0; it < TILE_ITERS; it++)
        cnt += (uint32_t)__popc(F::candidates(base, len, n_chunks, (uint64_t)blockIdx.x * TILE_CHUNKS + it * TILE_THREADS + threadIdx.x));
    const uint32_t wave_total = rdlane(wave_incl_scan(cnt), 63);
    if (lane_id() == 0 && wave_total) atomicAdd(&s_cnt, wave_total);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_cnt;
}

// the positions of the candidates, ascending
template <class F>
__global__ __launch_bounds__(TILE_THREADS) void plan_emit_kernel(const uint8_t *base, uint64_t len, uint64_t n_chunks, const uint64_t *tile_cnt,
                                                                 const uint64_t *tile_excl, const uint64_t *tile_part, uint64_t *pos, uint32_t n_cand,
                                                                 PlanSummary *ds)
{
    __shared__ uint32_t s_wave[TILE_THREADS / 64];
    const uint64_t want = tile_cnt[blockIdx.x];
    if (want == 0) return;  // (uniform) most tiles of a file of large units
    const uint64_t first = tile_excl[blockIdx.x] + tile_part[blockIdx.x / SCAN_THREADS];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t done = 0;
    for (uint32_t it = 0; it < TILE_ITERS; it++) {
        const uint64_t g = (uint64_t)blockIdx.x * TILE_CHUNKS + it * TILE_THREADS + threadIdx.x;
        uint32_t m = F::candidates(base, len, n_chunks, g);
        const uint32_t inc = wave_incl_scan((uint32_t)__popc(m));
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < TILE_THREADS / 64; w++) {
            before += w < wave ? s_wave[w] : 0u;
            total += s_wave[w];
        }
        __syncthreads();
        uint64_t idx = first + done + before + inc - (uint32_t)__popc(m);
        while (m) {
            const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            if (idx < n_cand) pos[idx] = g * 16 + k;
            else ds->fault = 1;
            idx++;
        }
        done += total;
    }
    if (threadIdx.x == 0 && done != want) ds->fault = 1;
}

// per candidate: end position, cap, info = verdict | kind << 8.  A position that is no candidate (the data changed under the
// kernels) is a fault, and a bad header so that nothing follows it.
template <class F>
__global__ __launch_bounds__(256) void plan_describe_kernel(const uint8_t *base, uint64_t len, const uint64_t *pos, uint32_t n_cand, uint64_t *end,
                                                            uint32_t *cap, uint32_t *info, PlanSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    bool gone = false;
    Described r = F::describe(base, len, pos[i], gone);
    if (gone) {
        r = Described{0, 0, (uint32_t)PLAN_BAD_HEADER, KIND_FRAME};
        ds->fault = 1;
    }
    end[i] = r.end;
    cap[i] = r.cap;
    info[i] = r.verdict | (r.kind << 8);
}

// jump[i] = index of the candidate a whole unit at candidate i leads to, n_cand (the sink) for everything else: the end of the
// buffer, a position without a header, a candidate that is no whole unit.  Starts the marks and the summary of an empty chain.
template <class F>
__global__ __launch_bounds__(256) void plan_succ_kernel(const uint64_t *pos, const uint64_t *end, const uint32_t *info, uint32_t n_cand, uint64_t len,
                                                        uint32_t *jump, uint32_t *marked, PlanSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    jump[i] = (info[i] & 0xffu) == 0 ? candidate_at(pos, i + 1u, n_cand, end[i]) : n_cand;
    marked[i] = (i == 0 && pos[0] == 0) ? 1u : 0u;
    if (i == 0) {  // the walk that stops at position 0 (no candidate there)
        ds->in_used = 0;
        ds->status = stop_status<F>(len, 0);
    }
}

[[maybe_unused]] __global__ __launch_bounds__(256) void plan_flags_kernel(const uint32_t *info, const uint32_t *cap, const uint32_t *marked,
                                                                          uint32_t n_cand, PlanAcc *acc)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    PlanAcc a{0, 0, 0, 0};
    if (marked[i] && (info[i] & 0xffu) == 0) {
        if ((info[i] >> 8) == KIND_SKIP) a.skips = 1;
        else if (cap[i] == CHIP_ZPLAN_UNSIZED) a.frames = a.unsized = 1;
        else a.frames = 1, a.bytes = cap[i];
    }
    acc[i] = a;
}

template <class F>
__global__ __launch_bounds__(256) void plan_output_kernel(const uint64_t *pos, const uint64_t *end, const uint32_t *cap, const uint32_t *info,
                                                          const uint32_t *marked, const uint32_t *jump, const PlanAcc *acc, const PlanAcc *acc_part,
                                                          uint32_t n_cand, uint64_t len, uint64_t max_units, uint64_t *in_off, uint32_t *in_len,
                                                          uint64_t *out_off, uint32_t *out_cap, PlanSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand || !marked[i]) return;
    const uint32_t verdict = info[i] & 0xffu;
    const uint64_t p = pos[i];
    // the one marked candidate without a successor: where the walk stopped
    if (verdict != 0) {
        ds->in_used = p;
        ds->status = (int32_t)verdict;
        return;
    }
    const uint64_t q = end[i];
    if ((info[i] >> 8) == KIND_FRAME) {
        const PlanAcc e = acc[i] + acc_part[i / SCAN_THREADS];
        if (e.frames < max_units) {
            in_off[e.frames] = p;
            in_len[e.frames] = (uint32_t)(q - p);
            out_off[e.frames] = e.bytes;
            out_cap[e.frames] = cap[i];
        }
        if (e.frames + 1 == ds->sum.frames) ds->last_cap = cap[i];
    }
    if (jump[i] >= n_cand) {
        ds->in_used = q;
        ds->status = stop_status<F>(len, q);
    }
}

// The describe phase plan_locked enqueues when the format brings none of its own: plan_describe_kernel<F>, no scratch, nothing
// behind the output.  A policy D of a format's own has the same three members --
//   D::EXTRA                      bytes of scratch per candidate, handed to both calls as `extra` (16-byte aligned, in buffer 1)
//   D::describe(..)               enqueues on `stream`, between emit and succ, whatever fills end / cap / info of every candidate
//                                 (info = verdict | kind << 8) from pos; sets ds->fault where the data contradicts the candidates
//   D::finish(..)                 enqueues behind the output kernel what else the format's summary needs (ds is the slot's summary)
// and neither waits for the stream.
template <class F>
struct KernelDescribe {
    static constexpr size_t EXTRA = 0;
    static hipError_t describe(const uint8_t *base, uint64_t len, const uint64_t *pos, uint32_t n_cand, uint64_t *end, uint32_t *cap, uint32_t *info,
                               uint8_t *, PlanSummary *ds, hipStream_t stream)
    {
        hipLaunchKernelGGL(plan_describe_kernel<F>, dim3((n_cand + 255u) / 256u), dim3(256), 0, stream, base, len, pos, n_cand, end, cap, info, ds);
        return hipSuccess;
    }
    static void finish(const uint32_t *, const uint32_t *, uint32_t, const uint8_t *, PlanSummary *, hipStream_t) {}
};

// The plan of base[0 .. len), len > 0: enqueues everything, waits twice (candidate count, summary) and leaves the summary in
// `res`; too_many = more candidates than an index holds.  The caller holds the cache's lock.  The slot's buffer 0 holds the tile
// counts and their scan (16 bytes per 16 KiB of input), buffer 1 the candidate tables (60 + 4 * levels + D::EXTRA bytes per
// candidate).
template <class F, class D = KernelDescribe<F>, class Sum>
hipError_t plan_locked(SummarySlot<Sum> &sl, const uint8_t *base, uint64_t len, uint64_t max_units, uint64_t *in_off, uint32_t *in_len,
                       uint64_t *out_off, uint32_t *out_cap, hipStream_t stream, PlanSummary &res, bool &too_many)
{
    static_assert(std::is_base_of<PlanSummary, Sum>::value, "the slot's summary starts with the plan's");
    res = PlanSummary{};
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    PlanSummary *ds = sl.d_sum;
    const uint64_t n_chunks = (len + 15) / 16, n_tiles = (n_chunks + TILE_CHUNKS - 1) / TILE_CHUNKS;
    if ((e = sl.grow(0, (size_t)(2 * n_tiles + scan_parts(n_tiles)) * 8)) != hipSuccess) return e;
    uint64_t *tile_cnt = (uint64_t *)sl.buf[0], *tile_excl = tile_cnt + n_tiles, *tile_part = tile_excl + n_tiles;
    if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(Sum), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(plan_count_kernel<F>, dim3((uint32_t)n_tiles), dim3(TILE_THREADS), 0, stream, base, len, n_chunks, tile_cnt);
    enqueue_scan<uint64_t>(tile_cnt, tile_excl, n_tiles, tile_part, &ds->cand, stream);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const uint64_t cand64 = sl.h_sum->cand;
    if (cand64 == 0) {  // no header anywhere: the walk stops at position 0
        res.status = stop_status<F>(len, 0);
        return hipSuccess;
    }
    if (cand64 > 0x7fffffffull) {
        too_many = true;
        return hipSuccess;
    }
    const uint32_t n_cand = (uint32_t)cand64;
    const uint32_t levels = jump_levels(n_cand);
    const size_t o_acc = 0, o_part = o_acc + (size_t)n_cand * sizeof(PlanAcc), o_pos = o_part + (size_t)scan_parts(n_cand) * sizeof(PlanAcc);
    const size_t o_end = o_pos + (size_t)n_cand * 8, o_cap = o_end + (size_t)n_cand * 8, o_info = up16(o_cap + (size_t)n_cand * 4);
    const size_t o_mark = up16(o_info + (size_t)n_cand * 4), o_jump = up16(o_mark + (size_t)n_cand * 4), jump_stride = up16((size_t)n_cand * 4);
    const size_t o_extra = o_jump + jump_stride * levels;
    if ((e = sl.grow(1, o_extra + (size_t)n_cand * D::EXTRA)) != hipSuccess) return e;
    uint8_t *c = sl.buf[1];
    PlanAcc *acc = (PlanAcc *)(c + o_acc), *acc_part = (PlanAcc *)(c + o_part);
    uint64_t *pos = (uint64_t *)(c + o_pos), *end = (uint64_t *)(c + o_end);
    uint32_t *cap = (uint32_t *)(c + o_cap), *info = (uint32_t *)(c + o_info), *marked = (uint32_t *)(c + o_mark);
    auto jump = [&](uint32_t k) { return (uint32_t *)(c + o_jump + jump_stride * k); };
    const dim3 cgrid((n_cand + 255u) / 256u);

    hipLaunchKernelGGL(plan_emit_kernel<F>, dim3((uint32_t)n_tiles), dim3(TILE_THREADS), 0, stream, base, len, n_chunks, (const uint64_t *)tile_cnt,
                       (const uint64_t *)tile_excl, (const uint64_t *)tile_part, pos, n_cand, ds);
    if ((e = D::describe(base, len, (const uint64_t *)pos, n_cand, end, cap, info, c + o_extra, ds, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(plan_succ_kernel<F>, cgrid, dim3(256), 0, stream, (const uint64_t *)pos, (const uint64_t *)end, (const uint32_t *)info, n_cand,
                       len, jump(0), marked, ds);
    for (uint32_t k = 0; k + 1 < levels; k++)
        hipLaunchKernelGGL(plan_double_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), jump(k + 1), n_cand);
    for (uint32_t k = levels; k-- > 0;) hipLaunchKernelGGL(plan_mark_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), marked, n_cand);
    hipLaunchKernelGGL(plan_flags_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)info, (const uint32_t *)cap, (const uint32_t *)marked, n_cand,
                       acc);
    enqueue_scan<PlanAcc>(acc, acc, n_cand, acc_part, &ds->sum, stream);
    hipLaunchKernelGGL(plan_output_kernel<F>, cgrid, dim3(256), 0, stream, (const uint64_t *)pos, (const uint64_t *)end, (const uint32_t *)cap,
                       (const uint32_t *)info, (const uint32_t *)marked, (const uint32_t *)jump(0), (const PlanAcc *)acc, (const PlanAcc *)acc_part, n_cand,
                       len, max_units, in_off, in_len, out_off, out_cap, ds);
    D::finish((const uint32_t *)info, (const uint32_t *)marked, n_cand, (const uint8_t *)(c + o_extra), ds, stream);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    if (sl.h_sum->fault) return hipErrorUnknown;  // the input changed between two passes
    res = *sl.h_sum;
    return hipSuccess;
}

}  // namespace

}  // namespace chip
