// The frame index of a buffer of zstd frames (pzstd output, the seekable format, one frame per chunk, `cat a.zst b.zst`): on the
// host (chip_zstd_plan_host) and on the GPU (chip_zstd_plan), and chip_layout_units, the device step from a size pass to a
// decode.  DESIGN.md sec. 4.12.
//
// The plan of a buffer is DEFINED by the serial walk of include/compu_hip.h (walk_frame below is its per-frame part, shared by
// the host walk and the kernel).  The GPU version has the shape of bgzf.hip and shares its generic kernels (plan_common.h):
//   1. count    every byte position is tested in 16-byte loads for the frame magic (`28 b5 2f fd`) and the skippable range
//               (`5x 2a 4d 18`); one count per 16 KiB tile
//   2. scan     exclusive scan of the tile counts
//      -- the host reads the candidate count and sizes the candidate scratch --
//   3. emit     tiles with candidates are read again and their positions written in ascending order;
//      walk     each candidate's own thread runs walk_frame: the frame header, then one 3-byte block header per block (a
//               skippable frame: one size field); it stores the end position, the verdict, Frame_Content_Size and the kind
//   4. succ     successor of a whole frame = the candidate at its end position (binary search); everything else leads to the sink
//   5. double   jump table k+1 = jump table k applied twice, ceil(log2(candidates + 1)) tables
//   6. mark     from candidate 0 (if it sits at position 0) top-down through the tables.  What is never marked is a decoy: magic
//               bytes inside block data, or a whole frame embedded in a raw block
//   7. output   {frames, skippable, unsized, content bytes} of the marked whole candidates, exclusive 64-bit scan, scatter of the
//               frames' rows; the one marked candidate without a successor says where and why the walk stopped
// Order between the phases comes from kernel boundaries on the stream only: no workgroup ever waits for another one.  Every index
// is checked against the count it belongs to; data that changes under the kernels sets DevSummary::fault instead of writing out of
// range.  No byte outside [0, len4) is loaded and none outside [0, len) decides anything.
#include <mutex>

#include "chip_internal.h"
#include "launch_slots.h"
#include "plan_common.h"

namespace chip {

namespace {

constexpr uint32_t ZSTD_MAGIC = 0xFD2FB528u, SKIP_MAGIC = 0x184D2A50u;  // the skippable range: SKIP_MAGIC | 0..15
constexpr uint32_t KIND_FRAME = 0, KIND_SKIP = 1;

struct FrameWalk {
    uint64_t end;      // position behind the frame (verdict 0 only)
    uint32_t cap;      // Frame_Content_Size, or CHIP_ZPLAN_UNSIZED (a skippable frame: 0)
    uint32_t verdict;  // 0 a whole frame, else the CHIP_ZPLAN_* status the walk stops with at p
    uint32_t kind;
};

__host__ __device__ __forceinline__ uint64_t le_bytes(const uint8_t *b, uint32_t n)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < n; k++) v |= (uint64_t)b[k] << (8 * k);
    return v;
}

// The per-frame part of the walk for the frame or skippable frame whose magic sits at p (p + 4 <= len, m = LE32(p) is one of the
// two kinds).  Reads bytes of [p, len) only.
__host__ __device__ __forceinline__ FrameWalk walk_frame(const uint8_t *in, uint64_t len, uint64_t p, uint32_t m)
{
    FrameWalk r{0, 0, 0, KIND_FRAME};
    const uint64_t room = len - p;
    if (m != ZSTD_MAGIC) {
        r.kind = KIND_SKIP;
        if (room < 8) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        const uint64_t s = le_bytes(in + p + 4, 4);
        if (s > room - 8) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        r.end = p + 8 + s;
        return r;
    }
    if (room < 5) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
    const uint32_t fhd = in[p + 4], f = fhd >> 6, ss = (fhd >> 5) & 1u, d = fhd & 3u;
    const uint32_t did_bytes = d == 3 ? 4u : d, fcs_bytes = f == 0 ? ss : 1u << f, fcs_at = 5u + (ss ? 0u : 1u) + did_bytes;
    const uint32_t hs = fcs_at + fcs_bytes;
    if (room < hs) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
    const bool sized = fcs_bytes != 0;
    const uint64_t fcs = sized ? le_bytes(in + p + fcs_at, fcs_bytes) + (fcs_bytes == 2 ? 256u : 0u) : 0;
    uint64_t q = p + hs;
    for (uint32_t blocks = 0;;) {
        if (len - q < 3) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        const uint32_t h = (uint32_t)le_bytes(in + q, 3), type = (h >> 1) & 3u;
        if (type == 3) return r.verdict = CHIP_ZPLAN_BAD_HEADER, r;
        if (++blocks > CHIP_ZPLAN_MAX_BLOCKS) return r.verdict = CHIP_ZPLAN_TOO_LARGE, r;
        const uint64_t body = type == 1 ? 1u : h >> 3;
        if (body > len - q - 3) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        q += 3 + body;
        if (h & 1u) break;
    }
    if (fhd & 4u) {
        if (len - q < 4) return r.verdict = CHIP_ZPLAN_TRUNCATED, r;
        q += 4;
    }
    if (q - p > 0xFFFFFFFFull || (sized && fcs >= 0xFFFFFFFFull)) return r.verdict = CHIP_ZPLAN_TOO_LARGE, r;
    r.end = q;
    r.cap = sized ? (uint32_t)fcs : CHIP_ZPLAN_UNSIZED;
    return r;
}

__host__ __device__ __forceinline__ bool is_magic(uint32_t m) { return m == ZSTD_MAGIC || (m & 0xFFFFFFF0u) == SKIP_MAGIC; }

// what the walk answers where no frame starts at e (the end of the last frame, or 0)
__host__ __device__ __forceinline__ int32_t stop_status(uint64_t len, uint64_t e)
{
    return e == len ? CHIP_ZPLAN_OK : len - e < 4 ? CHIP_ZPLAN_TRUNCATED : CHIP_ZPLAN_BAD_HEADER;
}

// what the kernels hand to the host (device memory, copied back once the candidates are counted and once at the end)
struct DevSummary {
    uint64_t n_frames, n_skippable, n_unsized, total_out;  // (the total of the output scan: the layout of Acc)
    uint64_t in_used;
    int32_t status;
    uint32_t fault;  // a kernel met data that contradicts an earlier pass
    uint64_t cand;   // total of the tile scan: number of candidates
    // chip_layout_units
    uint64_t layout_total, layout_over;
};

struct Acc {
    uint64_t frames, skips, unsized, bytes;  // marked whole candidates of each kind, the frames without a size, Frame_Content_Size
};
__host__ __device__ __forceinline__ Acc operator+(const Acc &a, const Acc &b)
{
    return Acc{a.frames + b.frames, a.skips + b.skips, a.unsized + b.unsized, a.bytes + b.bytes};
}
__device__ __forceinline__ Acc shfl_up_t(const Acc &v, uint32_t d)
{
    return Acc{shfl_up_t(v.frames, d), shfl_up_t(v.skips, d), shfl_up_t(v.unsized, d), shfl_up_t(v.bytes, d)};
}

// candidates of chunk g as a 16-bit mask: the positions whose four bytes, all in front of `len`, are one of the magics
__device__ __forceinline__ uint32_t chunk_candidates(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t g)
{
    if (g >= n_chunks) return 0;
    uint32_t w[5];
    load_chunk(base, (len + 3) & ~(uint64_t)3, g, w);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) m |= (is_magic(chunk_word(w, k)) ? 1u : 0u) << k;
    const uint64_t b = g * 16;
    if (b + 20 > len) {  // (the last two chunks) drop what reaches behind len: the padding up to len4 holds anything
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (b + k + 4 > len) m &= ~(1u << k);
    }
    return m;
}

__global__ __launch_bounds__(TILE_THREADS) void zplan_count_kernel(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t *tile_cnt)
{
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t it = 0; it < TILE_ITERS; it++)
        cnt += (uint32_t)__popc(chunk_candidates(base, len, n_chunks, (uint64_t)blockIdx.x * TILE_CHUNKS + it * TILE_THREADS + threadIdx.x));
    const uint32_t wave_total = rdlane(wave_incl_scan(cnt), 63);
    if (lane_id() == 0 && wave_total) atomicAdd(&s_cnt, wave_total);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_cnt;
}

// the positions of the candidates, ascending
__global__ __launch_bounds__(TILE_THREADS) void zplan_emit_kernel(const uint8_t *base, uint64_t len, uint64_t n_chunks, const uint64_t *tile_cnt,
                                                                  const uint64_t *tile_excl, const uint64_t *tile_part, uint64_t *pos, uint32_t n_cand,
                                                                  DevSummary *ds)
{
    __shared__ uint32_t s_wave[TILE_THREADS / 64];
    const uint64_t want = tile_cnt[blockIdx.x];
    if (want == 0) return;  // (uniform) most tiles of a file of large frames
    const uint64_t first = tile_excl[blockIdx.x] + tile_part[blockIdx.x / SCAN_THREADS];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint64_t done = 0;
    for (uint32_t it = 0; it < TILE_ITERS; it++) {
        const uint64_t g = (uint64_t)blockIdx.x * TILE_CHUNKS + it * TILE_THREADS + threadIdx.x;
        uint32_t m = chunk_candidates(base, len, n_chunks, g);
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

// per candidate: end position, cap, info = verdict | kind << 8.  A position that no longer holds a magic (the data changed
// under the kernels) or lies out of range is a fault, and a bad header so that nothing follows it.
__global__ __launch_bounds__(256) void zplan_walk_kernel(const uint8_t *base, uint64_t len, const uint64_t *pos, uint32_t n_cand, uint64_t *end,
                                                         uint32_t *cap, uint32_t *info, DevSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    const uint64_t p = pos[i];
    FrameWalk r{0, 0, CHIP_ZPLAN_BAD_HEADER, KIND_FRAME};
    const uint32_t m = p < len && len - p >= 4 ? (uint32_t)le_bytes(base + p, 4) : 0u;
    if (is_magic(m)) r = walk_frame(base, len, p, m);
    else ds->fault = 1;
    end[i] = r.end;
    cap[i] = r.cap;
    info[i] = r.verdict | (r.kind << 8);
}

// jump[i] = index of the candidate a whole frame at candidate i leads to, n_cand (the sink) for everything else.  Starts the
// marks and the summary of an empty chain.
__global__ __launch_bounds__(256) void zplan_succ_kernel(const uint64_t *pos, const uint64_t *end, const uint32_t *info, uint32_t n_cand, uint64_t len,
                                                         uint32_t *jump, uint32_t *marked, DevSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    jump[i] = (info[i] & 0xffu) == 0 ? candidate_at(pos, i + 1u, n_cand, end[i]) : n_cand;
    marked[i] = (i == 0 && pos[0] == 0) ? 1u : 0u;
    if (i == 0) {  // the walk that stops at position 0 (no magic there)
        ds->in_used = 0;
        ds->status = stop_status(len, 0);
    }
}

__global__ __launch_bounds__(256) void zplan_flags_kernel(const uint32_t *info, const uint32_t *cap, const uint32_t *marked, uint32_t n_cand, Acc *acc)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    Acc a{0, 0, 0, 0};
    if (marked[i] && (info[i] & 0xffu) == 0) {
        if ((info[i] >> 8) == KIND_SKIP) a.skips = 1;
        else if (cap[i] == CHIP_ZPLAN_UNSIZED) a.frames = a.unsized = 1;
        else a.frames = 1, a.bytes = cap[i];
    }
    acc[i] = a;
}

__global__ __launch_bounds__(256) void zplan_output_kernel(const uint64_t *pos, const uint64_t *end, const uint32_t *cap, const uint32_t *info,
                                                           const uint32_t *marked, const uint32_t *jump, const Acc *acc, const Acc *acc_part,
                                                           uint32_t n_cand, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len,
                                                           uint64_t *out_off, uint32_t *out_cap, DevSummary *ds)
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
        const Acc e = acc[i] + acc_part[i / SCAN_THREADS];
        if (e.frames < max_frames) {
            in_off[e.frames] = p;
            in_len[e.frames] = (uint32_t)(q - p);
            out_off[e.frames] = e.bytes;
            out_cap[e.frames] = cap[i];
        }
    }
    if (jump[i] >= n_cand) {
        ds->in_used = q;
        ds->status = stop_status(len, q);
    }
}

// chip_layout_units behind the two scan kernels: out_off[i] gets its workgroup's offset, out_cap[i] the clipped size
__global__ __launch_bounds__(256) void layout_finish_kernel(const uint64_t *out_size, uint64_t *out_off, uint32_t *out_cap, const uint64_t *part,
                                                            uint64_t n, DevSummary *ds)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = out_size[i];
    out_off[i] += part[i / SCAN_THREADS];
    out_cap[i] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
    if (s > 0xFFFFFFFFull) atomicAdd((unsigned long long *)&ds->layout_over, 1ull);  // (rare: a unit above 4 GiB)
}

// The scratch of one (device, stream): tile counts and their scan (16 bytes per 16 KiB of input; chip_layout_units: 8 bytes per
// 1024 units), the candidate tables (60 + 4 * levels bytes per candidate), the summary on the device and its pinned copy.  A
// launch slot.
struct ZplanSlot {
    uint8_t *tiles = nullptr, *cand = nullptr;
    size_t tiles_cap = 0, cand_cap = 0;
    DevSummary *d_sum = nullptr, *h_sum = nullptr;

    hipError_t summary()
    {
        hipError_t e = hipSuccess;
        if (!d_sum) e = hipMalloc((void **)&d_sum, sizeof(DevSummary));
        if (e == hipSuccess && !h_sum) e = hipHostMalloc((void **)&h_sum, sizeof(DevSummary), hipHostMallocDefault);
        return e;
    }
    void free()
    {
        (void)hipFree(tiles);
        (void)hipFree(cand);
        (void)hipFree(d_sum);
        if (h_sum) (void)hipHostFree(h_sum);
    }
};
SlotCache<ZplanSlot> g_zplan_cache;

hipError_t fetch_summary(ZplanSlot &sl, hipStream_t stream)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(sl.h_sum, sl.d_sum, sizeof(DevSummary), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}

// Enqueues everything, waits twice (candidate count, summary).  The caller holds the cache's lock.
hipError_t plan_locked(ZplanSlot &sl, const uint8_t *base, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len,
                       uint64_t *out_off, uint32_t *out_cap, chip_zstd_plan_summary *summary, hipStream_t stream, bool &too_many)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    const uint64_t n_chunks = (len + 15) / 16, n_tiles = (n_chunks + TILE_CHUNKS - 1) / TILE_CHUNKS;
    const uint64_t tile_parts = (n_tiles + SCAN_THREADS - 1) / SCAN_THREADS;
    if ((e = grow_buffer(sl.tiles, sl.tiles_cap, (size_t)(2 * n_tiles + tile_parts) * 8)) != hipSuccess) return e;
    uint64_t *tile_cnt = (uint64_t *)sl.tiles, *tile_excl = tile_cnt + n_tiles, *tile_part = tile_excl + n_tiles;
    if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(DevSummary), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(zplan_count_kernel, dim3((uint32_t)n_tiles), dim3(TILE_THREADS), 0, stream, base, len, n_chunks, tile_cnt);
    hipLaunchKernelGGL(plan_scan_local_kernel<uint64_t>, dim3((uint32_t)tile_parts), dim3(SCAN_THREADS), 0, stream, (const uint64_t *)tile_cnt,
                       tile_excl, n_tiles, tile_part);
    hipLaunchKernelGGL(plan_scan_partials_kernel<uint64_t>, dim3(1), dim3(SCAN_THREADS), 0, stream, tile_part, tile_parts, &sl.d_sum->cand);
    if ((e = fetch_summary(sl, stream)) != hipSuccess) return e;
    const uint64_t cand64 = sl.h_sum->cand;
    if (cand64 == 0) {  // no magic anywhere: the walk stops at position 0
        summary->status = stop_status(len, 0);
        return hipSuccess;
    }
    if (cand64 > 0x7fffffffull) {
        too_many = true;
        return hipSuccess;
    }
    const uint32_t n_cand = (uint32_t)cand64;
    const uint32_t levels = jump_levels(n_cand);
    const size_t cand_parts = ((size_t)n_cand + SCAN_THREADS - 1) / SCAN_THREADS;
    const size_t o_acc = 0, o_part = o_acc + (size_t)n_cand * sizeof(Acc), o_pos = o_part + cand_parts * sizeof(Acc);
    const size_t o_end = o_pos + (size_t)n_cand * 8, o_cap = o_end + (size_t)n_cand * 8, o_info = up16(o_cap + (size_t)n_cand * 4);
    const size_t o_mark = up16(o_info + (size_t)n_cand * 4), o_jump = up16(o_mark + (size_t)n_cand * 4), jump_stride = up16((size_t)n_cand * 4);
    if ((e = grow_buffer(sl.cand, sl.cand_cap, o_jump + jump_stride * levels)) != hipSuccess) return e;
    Acc *acc = (Acc *)(sl.cand + o_acc), *acc_part = (Acc *)(sl.cand + o_part);
    uint64_t *pos = (uint64_t *)(sl.cand + o_pos), *end = (uint64_t *)(sl.cand + o_end);
    uint32_t *cap = (uint32_t *)(sl.cand + o_cap), *info = (uint32_t *)(sl.cand + o_info), *marked = (uint32_t *)(sl.cand + o_mark);
    auto jump = [&](uint32_t k) { return (uint32_t *)(sl.cand + o_jump + jump_stride * k); };
    const dim3 cgrid((n_cand + 255u) / 256u);

    hipLaunchKernelGGL(zplan_emit_kernel, dim3((uint32_t)n_tiles), dim3(TILE_THREADS), 0, stream, base, len, n_chunks, (const uint64_t *)tile_cnt,
                       (const uint64_t *)tile_excl, (const uint64_t *)tile_part, pos, n_cand, sl.d_sum);
    hipLaunchKernelGGL(zplan_walk_kernel, cgrid, dim3(256), 0, stream, base, len, (const uint64_t *)pos, n_cand, end, cap, info, sl.d_sum);
    hipLaunchKernelGGL(zplan_succ_kernel, cgrid, dim3(256), 0, stream, (const uint64_t *)pos, (const uint64_t *)end, (const uint32_t *)info, n_cand,
                       len, jump(0), marked, sl.d_sum);
    for (uint32_t k = 0; k + 1 < levels; k++)
        hipLaunchKernelGGL(plan_double_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), jump(k + 1), n_cand);
    for (uint32_t k = levels; k-- > 0;) hipLaunchKernelGGL(plan_mark_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), marked, n_cand);
    hipLaunchKernelGGL(zplan_flags_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)info, (const uint32_t *)cap, (const uint32_t *)marked, n_cand,
                       acc);
    hipLaunchKernelGGL(plan_scan_local_kernel<Acc>, dim3((uint32_t)cand_parts), dim3(SCAN_THREADS), 0, stream, (const Acc *)acc, acc, (uint64_t)n_cand,
                       acc_part);
    hipLaunchKernelGGL(plan_scan_partials_kernel<Acc>, dim3(1), dim3(SCAN_THREADS), 0, stream, acc_part, (uint64_t)cand_parts, (Acc *)sl.d_sum);
    hipLaunchKernelGGL(zplan_output_kernel, cgrid, dim3(256), 0, stream, (const uint64_t *)pos, (const uint64_t *)end, (const uint32_t *)cap,
                       (const uint32_t *)info, (const uint32_t *)marked, (const uint32_t *)jump(0), (const Acc *)acc, (const Acc *)acc_part, n_cand, len,
                       max_frames, in_off, in_len, out_off, out_cap, sl.d_sum);
    if ((e = fetch_summary(sl, stream)) != hipSuccess) return e;
    if (sl.h_sum->fault) return hipErrorUnknown;  // the input changed between two passes
    summary->n_frames = sl.h_sum->n_frames;
    summary->n_skippable = sl.h_sum->n_skippable;
    summary->n_unsized = sl.h_sum->n_unsized;
    summary->total_out = sl.h_sum->total_out;
    summary->in_used = sl.h_sum->in_used;
    summary->status = sl.h_sum->status;
    return hipSuccess;
}

hipError_t layout_locked(ZplanSlot &sl, uint64_t n, const uint64_t *out_size, uint64_t *out_off, uint32_t *out_cap, uint64_t *total,
                         uint64_t *n_over, hipStream_t stream)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    const uint64_t parts = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    if ((e = grow_buffer(sl.tiles, sl.tiles_cap, (size_t)parts * 8)) != hipSuccess) return e;
    uint64_t *part = (uint64_t *)sl.tiles;
    if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(DevSummary), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(plan_scan_local_kernel<uint64_t>, dim3((uint32_t)parts), dim3(SCAN_THREADS), 0, stream, out_size, out_off, n, part);
    hipLaunchKernelGGL(plan_scan_partials_kernel<uint64_t>, dim3(1), dim3(SCAN_THREADS), 0, stream, part, parts, &sl.d_sum->layout_total);
    hipLaunchKernelGGL(layout_finish_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, out_size, out_off, out_cap,
                       (const uint64_t *)part, n, sl.d_sum);
    if ((e = fetch_summary(sl, stream)) != hipSuccess) return e;
    *total = sl.h_sum->layout_total;
    *n_over = sl.h_sum->layout_over;
    return hipSuccess;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_zstd_plan_host(const uint8_t *in, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                        uint32_t *out_cap, chip_zstd_plan_summary *summary)
{
    if (!summary || (len && !in) || (max_frames && (!in_off || !in_len || !out_off || !out_cap))) return CHIP_E_INVALID;
    uint64_t p = 0, n = 0, skipped = 0, unsized = 0, total = 0;
    int32_t status = CHIP_ZPLAN_OK;
    for (;;) {
        const uint32_t m = len - p >= 4 ? (uint32_t)le_bytes(in + p, 4) : 0u;
        if (len - p < 4 || !is_magic(m)) {
            status = stop_status(len, p);
            break;
        }
        const FrameWalk r = walk_frame(in, len, p, m);
        if (r.verdict) {
            status = (int32_t)r.verdict;
            break;
        }
        if (r.kind == KIND_SKIP) {
            skipped++;
        } else {
            const bool sized = r.cap != CHIP_ZPLAN_UNSIZED;
            if (n < max_frames) {
                in_off[n] = p;
                in_len[n] = (uint32_t)(r.end - p);
                out_off[n] = total;
                out_cap[n] = r.cap;
            }
            n++;
            unsized += sized ? 0 : 1;
            total += sized ? r.cap : 0;
        }
        p = r.end;
    }
    *summary = chip_zstd_plan_summary{n, skipped, unsized, total, p, status, 0};
    return CHIP_OK;
}

int chip_zstd_plan(const void *in_base, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                   uint32_t *out_cap, chip_zstd_plan_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_frames && (!in_off || !in_len || !out_off || !out_cap)) || ((uintptr_t)in_base & 3u) ||
        len > ((uint64_t)1 << 40))
        return CHIP_E_INVALID;
    *summary = chip_zstd_plan_summary{0, 0, 0, 0, 0, CHIP_ZPLAN_OK, 0};
    if (len == 0) return CHIP_OK;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) return CHIP_E_NO_DEVICE;
    std::lock_guard<std::mutex> lk(g_zplan_cache.mu);  // from the slot's lookup to the last launch (and the wait behind it)
    ZplanSlot *sl = nullptr;
    if (g_zplan_cache.at((hipStream_t)stream, sl) != hipSuccess) return CHIP_E_LAUNCH;
    bool too_many = false;
    const hipError_t e = plan_locked(*sl, (const uint8_t *)in_base, len, max_frames, in_off, in_len, out_off, out_cap, summary, (hipStream_t)stream, too_many);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize((hipStream_t)stream);  // the slot is handed on only with nothing in flight
        *summary = chip_zstd_plan_summary{0, 0, 0, 0, 0, CHIP_ZPLAN_BAD_HEADER, 0};
        return e == hipErrorOutOfMemory ? CHIP_E_NOMEM : CHIP_E_LAUNCH;
    }
    return too_many ? CHIP_E_NOMEM : CHIP_OK;
}

int chip_layout_units(size_t n, const uint64_t *out_size, uint64_t *out_off, uint32_t *out_cap, uint64_t *total, uint64_t *n_over, void *stream)
{
    if (!total || !n_over || (n && (!out_size || !out_off || !out_cap || (const void *)out_size == (const void *)out_off)) ||
        (uint64_t)n > 0xFFFFFFFFull)
        return CHIP_E_INVALID;
    *total = *n_over = 0;
    if (n == 0) return CHIP_OK;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) return CHIP_E_NO_DEVICE;
    std::lock_guard<std::mutex> lk(g_zplan_cache.mu);
    ZplanSlot *sl = nullptr;
    if (g_zplan_cache.at((hipStream_t)stream, sl) != hipSuccess) return CHIP_E_LAUNCH;
    const hipError_t e = layout_locked(*sl, n, out_size, out_off, out_cap, total, n_over, (hipStream_t)stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        *total = *n_over = 0;
        return e == hipErrorOutOfMemory ? CHIP_E_NOMEM : CHIP_E_LAUNCH;
    }
    return CHIP_OK;
}

}  // extern "C"
