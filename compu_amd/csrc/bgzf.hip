// BGZF (the blocked gzip of BAM / BCF / bgzip): the block index of a buffer, on the host (chip_bgzf_plan_host) and on the GPU
// (chip_bgzf_plan), and htslib's EOF marker.  DESIGN.md sec. 4.10.
//
// The plan of a buffer is DEFINED by the serial walk of include/compu_hip.h (chip_bgzf_plan_host below is that walk).  The GPU
// version gives the same answer without chasing BSIZE through HBM one block after the other:
//   1. count    every byte position is tested for the gzip magic with FEXTRA (`1f 8b 08 04`) in 16-byte loads, the rare hits for the
//               other fixed header bytes; one count per 16 KiB tile
//   2. scan     exclusive scan of the tile counts (reduce-then-scan: plan_scan_local_kernel, plan_scan_partials_kernel)
//      -- the host reads the candidate count and sizes the candidate scratch --
//   3. emit     tiles with candidates are read again and their candidates written in ascending order: position, BSIZE and the
//               per-candidate verdict (block too short / runs past the end / ISIZE too large), ISIZE
//   4. succ     successor of a valid candidate = the candidate at position + BSIZE + 1 (binary search); everything else leads to
//               the sink (index = number of candidates)
//   5. double   jump table k+1 = jump table k applied twice, ceil(log2(candidates + 1)) tables
//   6. mark     from candidate 0 (if it sits at position 0) top-down through the tables: after the level-k launch every candidate
//               whose distance from 0 has bits >= k only is marked.  What is never marked is a decoy (valid compressed data may
//               hold the header bytes, e.g. inside a stored block)
//   7. output   flags + ISIZE of the marked valid candidates, exclusive 64-bit scan (the same two scan kernels), scatter to the
//               caller's arrays; the one marked candidate without a successor says where and why the walk stopped
// Order between the phases comes from kernel boundaries on the stream only: no workgroup ever waits for another one.  Every
// index is checked against the count it belongs to; data that changes under the kernels (count and emit disagree) sets
// DevSummary::fault instead of writing out of range.
#include <mutex>

#include "chip_internal.h"
#include "launch_slots.h"
#include "plan_common.h"

namespace chip {

namespace {

constexpr uint32_t BGZF_HDR = 18;               // bytes of the header this library accepts (XLEN 6: the BC subfield alone)
constexpr uint32_t BGZF_MIN = 28;               // header + empty deflate body (2) + CRC-32 + ISIZE
constexpr uint32_t BGZF_MAGIC = 0x04088b1fu;    // 1f 8b 08 04, little endian

// what the kernels hand to the host (device memory, copied back once the candidates are counted and once at the end)
struct DevSummary {
    uint64_t n_blocks, total_out;  // (the total of the output scan: the layout of Acc)
    uint64_t in_used;
    int32_t status;
    uint32_t eof;
    uint64_t cand;   // total of the tile scan: number of candidates
    uint32_t fault;  // a kernel met data that contradicts an earlier pass
    uint32_t pad;
};

struct Acc {
    uint64_t c, s;  // marked valid candidates, their ISIZE
};
__host__ __device__ __forceinline__ Acc operator+(const Acc &a, const Acc &b) { return Acc{a.c + b.c, a.s + b.s}; }

__device__ __forceinline__ Acc shfl_up_t(const Acc &v, uint32_t d) { return Acc{shfl_up_t(v.c, d), shfl_up_t(v.s, d)}; }

// bit k: the four bytes at offset k of the chunk are the magic
__device__ __forceinline__ uint32_t magic_mask(const uint32_t w[5])
{
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) m |= (chunk_word(w, k) == BGZF_MAGIC ? 1u : 0u) << k;
    return m;
}

// the rest of the fixed header bytes at a position that holds the magic: a whole header in front of `len`, XLEN 6, `B C 02 00`
__device__ __forceinline__ bool header_rest(const uint8_t *base, uint64_t len, uint64_t p)
{
    if (len < BGZF_HDR || p > len - BGZF_HDR) return false;
    const uint8_t *h = base + p;
    return h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0;
}

// candidates of chunk g as a 16-bit mask
__device__ __forceinline__ uint32_t chunk_candidates(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t g)
{
    if (g >= n_chunks) return 0;
    uint32_t w[5];
    load_chunk(base, (len + 3) & ~(uint64_t)3, g, w);
    uint32_t m = magic_mask(w), keep = 0;
    while (m) {
        const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        if (header_rest(base, len, g * 16 + k)) keep |= 1u << k;
    }
    return keep;
}

__global__ __launch_bounds__(TILE_THREADS) void bgzf_count_kernel(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t *tile_cnt)
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

// per candidate: info = BSIZE | verdict << 16 (0 a whole block, else the CHIP_BGZF_* status the walk stops with there)
__global__ __launch_bounds__(TILE_THREADS) void bgzf_emit_kernel(const uint8_t *base, uint64_t len, uint64_t n_chunks, const uint64_t *tile_cnt,
                                                                 const uint64_t *tile_excl, const uint64_t *tile_part, uint64_t *pos,
                                                                 uint32_t *info, uint32_t *isz, uint32_t n_cand, DevSummary *ds)
{
    __shared__ uint32_t s_wave[TILE_THREADS / 64];
    const uint64_t want = tile_cnt[blockIdx.x];
    if (want == 0) return;  // (uniform) most tiles of a file of large blocks
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
            const uint64_t p = g * 16 + k;
            if (idx < n_cand) {
                const uint32_t bsize = (uint32_t)base[p + 16] | ((uint32_t)base[p + 17] << 8), bs = bsize + 1u;
                uint32_t verdict = 0, isize = 0;
                if (bs < BGZF_MIN) verdict = CHIP_BGZF_BAD_HEADER;
                else if (bs > len - p) verdict = CHIP_BGZF_TRUNCATED;
                else {
                    const uint8_t *t = base + p + bs - 4;
                    isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
                    if (isize > 65536u) verdict = CHIP_BGZF_BAD_HEADER, isize = 0;
                }
                pos[idx] = p;
                info[idx] = bsize | (verdict << 16);
                isz[idx] = isize;
            } else {
                ds->fault = 1;
            }
            idx++;
        }
        done += total;
    }
    if (threadIdx.x == 0 && done != want) ds->fault = 1;
}

// jump[i] = index of the candidate a whole block at candidate i leads to, n_cand (the sink) for everything else: the end of the
// buffer, a position without a header, a candidate that is no whole block.  Starts the marks and the summary of an empty chain.
__global__ __launch_bounds__(256) void bgzf_succ_kernel(const uint64_t *pos, const uint32_t *info, uint32_t n_cand, uint64_t len, uint32_t *jump,
                                                        uint32_t *marked, DevSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    uint32_t j = n_cand;
    const uint32_t f = info[i];
    if ((f >> 16) == 0) {
        const uint64_t nx = pos[i] + (f & 0xffffu) + 1u;
        j = candidate_at(pos, i + 1u, n_cand, nx);
    }
    jump[i] = j;
    marked[i] = (i == 0 && pos[0] == 0) ? 1u : 0u;
    if (i == 0) {  // the walk that stops at position 0 (len >= 18 here, or there would be no candidate)
        ds->n_blocks = ds->total_out = ds->in_used = 0;
        ds->status = len < BGZF_HDR ? CHIP_BGZF_TRUNCATED : CHIP_BGZF_BAD_HEADER;
        ds->eof = 0;
    }
}

__global__ __launch_bounds__(256) void bgzf_flags_kernel(const uint32_t *info, const uint32_t *isz, const uint32_t *marked, uint32_t n_cand, Acc *acc)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    const bool block = marked[i] && (info[i] >> 16) == 0;
    acc[i] = block ? Acc{1u, isz[i]} : Acc{0u, 0u};
}

__global__ __launch_bounds__(256) void bgzf_output_kernel(const uint64_t *pos, const uint32_t *info, const uint32_t *isz, const uint32_t *marked,
                                                          const uint32_t *jump, const Acc *acc, const Acc *acc_part, uint32_t n_cand, uint64_t len,
                                                          uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                                                          uint32_t *out_cap, DevSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand || !marked[i]) return;
    const uint32_t f = info[i], verdict = f >> 16, bs = (f & 0xffffu) + 1u;
    const uint64_t p = pos[i];
    if (verdict == 0) {
        const Acc e = acc[i] + acc_part[i / SCAN_THREADS];
        if (e.c < max_blocks) {
            in_off[e.c] = p;
            in_len[e.c] = bs;
            out_off[e.c] = e.s;
            out_cap[e.c] = isz[i];
        }
        if (e.c + 1 == ds->n_blocks) ds->eof = isz[i] == 0 ? 1u : 0u;
    }
    // the one marked candidate without a successor: where the walk stopped
    if (verdict != 0) {
        ds->in_used = p;
        ds->status = (int32_t)verdict;
    } else if (jump[i] >= n_cand) {
        const uint64_t nx = p + bs;
        ds->in_used = nx;
        ds->status = nx == len ? CHIP_BGZF_OK : len - nx < BGZF_HDR ? CHIP_BGZF_TRUNCATED : CHIP_BGZF_BAD_HEADER;
    }
}

// The plan's scratch of one (device, stream): tile counts and their scan (16 bytes per 16 KiB of input), the candidate tables
// (36 + 4 * levels bytes per candidate), the summary on the device and its pinned copy.  A launch slot.
struct BgzfSlot {
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
SlotCache<BgzfSlot> g_bgzf_cache;

// Enqueues everything, waits twice (candidate count, summary).  The caller holds the cache's lock.
hipError_t plan_locked(BgzfSlot &sl, const uint8_t *base, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len,
                       uint64_t *out_off, uint32_t *out_cap, chip_bgzf_summary *summary, hipStream_t stream, bool &too_many)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    const uint64_t n_chunks = (len + 15) / 16, n_tiles = (n_chunks + TILE_CHUNKS - 1) / TILE_CHUNKS;
    const uint64_t tile_parts = (n_tiles + SCAN_THREADS - 1) / SCAN_THREADS;
    if ((e = grow_buffer(sl.tiles, sl.tiles_cap, (size_t)(2 * n_tiles + tile_parts) * 8)) != hipSuccess) return e;
    uint64_t *tile_cnt = (uint64_t *)sl.tiles, *tile_excl = tile_cnt + n_tiles, *tile_part = tile_excl + n_tiles;
    if ((e = hipMemsetAsync(sl.d_sum, 0, sizeof(DevSummary), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(bgzf_count_kernel, dim3((uint32_t)n_tiles), dim3(TILE_THREADS), 0, stream, base, len, n_chunks, tile_cnt);
    hipLaunchKernelGGL(plan_scan_local_kernel<uint64_t>, dim3((uint32_t)tile_parts), dim3(SCAN_THREADS), 0, stream, (const uint64_t *)tile_cnt,
                       tile_excl, n_tiles, tile_part);
    hipLaunchKernelGGL(plan_scan_partials_kernel<uint64_t>, dim3(1), dim3(SCAN_THREADS), 0, stream, tile_part, tile_parts, &sl.d_sum->cand);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(sl.h_sum, sl.d_sum, sizeof(DevSummary), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    const uint64_t cand64 = sl.h_sum->cand;
    if (cand64 == 0) {  // no header anywhere: the walk stops at position 0
        summary->status = len < BGZF_HDR ? CHIP_BGZF_TRUNCATED : CHIP_BGZF_BAD_HEADER;
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
    const size_t o_info = o_pos + (size_t)n_cand * 8, o_isz = up16(o_info + (size_t)n_cand * 4), o_mark = up16(o_isz + (size_t)n_cand * 4);
    const size_t o_jump = up16(o_mark + (size_t)n_cand * 4), jump_stride = up16((size_t)n_cand * 4);
    if ((e = grow_buffer(sl.cand, sl.cand_cap, o_jump + jump_stride * levels)) != hipSuccess) return e;
    Acc *acc = (Acc *)(sl.cand + o_acc), *acc_part = (Acc *)(sl.cand + o_part);
    uint64_t *pos = (uint64_t *)(sl.cand + o_pos);
    uint32_t *info = (uint32_t *)(sl.cand + o_info), *isz = (uint32_t *)(sl.cand + o_isz), *marked = (uint32_t *)(sl.cand + o_mark);
    auto jump = [&](uint32_t k) { return (uint32_t *)(sl.cand + o_jump + jump_stride * k); };
    const dim3 cgrid((n_cand + 255u) / 256u);

    hipLaunchKernelGGL(bgzf_emit_kernel, dim3((uint32_t)n_tiles), dim3(TILE_THREADS), 0, stream, base, len, n_chunks, (const uint64_t *)tile_cnt,
                       (const uint64_t *)tile_excl, (const uint64_t *)tile_part, pos, info, isz, n_cand, sl.d_sum);
    hipLaunchKernelGGL(bgzf_succ_kernel, cgrid, dim3(256), 0, stream, (const uint64_t *)pos, (const uint32_t *)info, n_cand, len, jump(0), marked,
                       sl.d_sum);
    for (uint32_t k = 0; k + 1 < levels; k++)
        hipLaunchKernelGGL(plan_double_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), jump(k + 1), n_cand);
    for (uint32_t k = levels; k-- > 0;) hipLaunchKernelGGL(plan_mark_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), marked, n_cand);
    hipLaunchKernelGGL(bgzf_flags_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)info, (const uint32_t *)isz, (const uint32_t *)marked, n_cand,
                       acc);
    hipLaunchKernelGGL(plan_scan_local_kernel<Acc>, dim3((uint32_t)cand_parts), dim3(SCAN_THREADS), 0, stream, (const Acc *)acc, acc, (uint64_t)n_cand,
                       acc_part);
    hipLaunchKernelGGL(plan_scan_partials_kernel<Acc>, dim3(1), dim3(SCAN_THREADS), 0, stream, acc_part, (uint64_t)cand_parts, (Acc *)sl.d_sum);
    hipLaunchKernelGGL(bgzf_output_kernel, cgrid, dim3(256), 0, stream, (const uint64_t *)pos, (const uint32_t *)info, (const uint32_t *)isz,
                       (const uint32_t *)marked, (const uint32_t *)jump(0), (const Acc *)acc, (const Acc *)acc_part, n_cand, len, max_blocks, in_off,
                       in_len, out_off, out_cap, sl.d_sum);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(sl.h_sum, sl.d_sum, sizeof(DevSummary), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if (sl.h_sum->fault) return hipErrorUnknown;  // the input changed between two passes
    summary->n_blocks = sl.h_sum->n_blocks;
    summary->total_out = sl.h_sum->total_out;
    summary->in_used = sl.h_sum->in_used;
    summary->status = sl.h_sum->status;
    summary->eof = sl.h_sum->eof;
    return hipSuccess;
}

const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

const uint8_t *chip_bgzf_eof_block(size_t *len)
{
    if (len) *len = sizeof(EOF_BLOCK);
    return EOF_BLOCK;
}

int chip_bgzf_plan_host(const uint8_t *in, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                        uint32_t *out_cap, chip_bgzf_summary *summary)
{
    if (!summary || (len && !in) || (max_blocks && (!in_off || !in_len || !out_off || !out_cap))) return CHIP_E_INVALID;
    uint64_t p = 0, n = 0, total = 0;
    uint32_t last_isize = 1;
    int32_t status = CHIP_BGZF_OK;
    while (p != len) {
        if (len - p < BGZF_HDR) {
            status = CHIP_BGZF_TRUNCATED;
            break;
        }
        const uint8_t *h = in + p;
        const bool header = h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && h[3] == 4 && h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' &&
                            h[14] == 2 && h[15] == 0;
        const uint32_t bs = ((uint32_t)h[16] | ((uint32_t)h[17] << 8)) + 1u;
        if (!header || bs < BGZF_MIN) {
            status = CHIP_BGZF_BAD_HEADER;
            break;
        }
        if (bs > len - p) {
            status = CHIP_BGZF_TRUNCATED;
            break;
        }
        const uint8_t *t = h + bs - 4;
        const uint32_t isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        if (isize > 65536u) {
            status = CHIP_BGZF_BAD_HEADER;
            break;
        }
        if (n < max_blocks) {
            in_off[n] = p;
            in_len[n] = bs;
            out_off[n] = total;
            out_cap[n] = isize;
        }
        last_isize = isize;
        n++;
        total += isize;
        p += bs;
    }
    summary->n_blocks = n;
    summary->total_out = total;
    summary->in_used = p;
    summary->status = status;
    summary->eof = n && last_isize == 0 ? 1u : 0u;
    return CHIP_OK;
}

int chip_bgzf_plan(const void *in_base, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                   uint32_t *out_cap, chip_bgzf_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_blocks && (!in_off || !in_len || !out_off || !out_cap)) || ((uintptr_t)in_base & 3u) ||
        len > ((uint64_t)1 << 40))
        return CHIP_E_INVALID;
    *summary = chip_bgzf_summary{0, 0, 0, CHIP_BGZF_OK, 0};
    if (len == 0) return CHIP_OK;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) return CHIP_E_NO_DEVICE;
    std::lock_guard<std::mutex> lk(g_bgzf_cache.mu);  // from the slot's lookup to the last launch (and the wait behind it)
    BgzfSlot *sl = nullptr;
    if (g_bgzf_cache.at((hipStream_t)stream, sl) != hipSuccess) return CHIP_E_LAUNCH;
    bool too_many = false;
    const hipError_t e = plan_locked(*sl, (const uint8_t *)in_base, len, max_blocks, in_off, in_len, out_off, out_cap, summary, (hipStream_t)stream, too_many);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize((hipStream_t)stream);  // the slot is handed on only with nothing in flight
        *summary = chip_bgzf_summary{0, 0, 0, CHIP_BGZF_BAD_HEADER, 0};
        return e == hipErrorOutOfMemory ? CHIP_E_NOMEM : CHIP_E_LAUNCH;
    }
    return too_many ? CHIP_E_NOMEM : CHIP_OK;
}

}  // extern "C"
