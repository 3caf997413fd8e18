// tar archives: chip_tar_plan[_host].  The definitions are in include/compu_hip.h; the host walk and the
// per-group code that host and device share are in tar_plan_core.h.
//
// A tar image has no directory: the index is the chain of headers through the data, and member data may hold valid headers of its
// own.  The unit of the chain is the GROUP (extension headers and the member header behind them), because a pax `size` makes a
// member's end depend on the header in front of it: a member header alone does not say where the next group starts.  The phases, in
// stream order, with the scans, the doubling, the marking, the slot and the scaffold of plan_common.h:
//   candidates          tar_count_kernel / scan / tar_emit_kernel: one lane per 512-byte block looks at the 8 bytes at +256 for the
//                       magic; counts per tile of TILE_BLOCKS blocks, positions in ascending order.  tar_stop0_kernel answers the
//                       walk that stops at position 0.
//   describe            tar_describe_kernel: one lane per candidate reads its whole group (tar::read_group, checksums included) and
//                       stores the group's end, the verdict, the offending header and the member's record.  A header inside member
//                       data, and a member header with extension headers in front of it, are described like any other: the marking
//                       never reaches them (the decoys).
//   succ, double, mark  tar_succ_kernel, plan_double_kernel, plan_mark_kernel from the candidate at 0
//   output              tar_flags_kernel, a 64-bit scan of {members, globals, bytes}, tar_output_kernel: the members' records in
//                       order; the one marked candidate without a successor says where and why the walk stopped (tar::stop_at
//                       behind the last group: the end, a cut block, the zero blocks, no header)
// Order between the phases comes from kernel boundaries on the stream only; every index is checked against its count, and every read
// of the image against `len`, whatever the earlier passes said: data that changes under the kernels sets TarDev::fault.
#include "chip_internal.h"
#include "launch_slots.h"
#include "plan_common.h"
#include "tar_plan_core.h"

namespace chip {

namespace {

static_assert(sizeof(chip_tar_entry) == 72 && alignof(chip_tar_entry) == 8, "chip_tar_entry: 72 bytes, no padding");
static_assert(sizeof(chip_tar_plan_summary) == 48, "chip_tar_plan_summary");

constexpr uint32_t TILE_BLOCKS = 256;  // 512-byte blocks per workgroup of the candidate search, one per lane: a 128 KiB tile

struct TarAcc {
    uint64_t members, globals, bytes;  // marked whole groups of each kind, the members' sizes
};
__host__ __device__ __forceinline__ TarAcc operator+(const TarAcc &a, const TarAcc &b)
{
    return TarAcc{a.members + b.members, a.globals + b.globals, a.bytes + b.bytes};
}
__device__ __forceinline__ TarAcc shfl_up_t(const TarAcc &v, uint32_t d)
{
    return TarAcc{shfl_up_t(v.members, d), shfl_up_t(v.globals, d), shfl_up_t(v.bytes, d)};
}

// what the kernels hand to the host (device memory, zeroed per call, copied back twice)
struct TarDev {
    TarAcc sum;     // total of the output scan
    uint64_t cand;  // total of the tile scan: number of candidates
    uint64_t stop_off, bad_off;
    int32_t status, zero_blocks;
    uint32_t fault, pad;  // a kernel met data that contradicts an earlier pass
};

struct __attribute__((packed, aligned(4))) Magic8 {
    uint32_t w[2];
};

// does block k (k < n_blocks: its 512 bytes lie in front of len) hold the magic?  One 8-byte access at +256.
__device__ __forceinline__ bool magic_at(const uint8_t *base, uint64_t k)
{
    const Magic8 m = *(const Magic8 *)(base + k * tar::BLOCK + 256);
    return (m.w[0] & 0xffffff00u) == 0x74737500u && (m.w[1] & 0xffffu) == 0x7261u;  // . u s t | a r
}

__global__ __launch_bounds__(TILE_BLOCKS) void tar_count_kernel(const uint8_t *base, uint64_t n_blocks, uint64_t *tile_cnt)
{
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * TILE_BLOCKS + threadIdx.x;
    const uint32_t wave_total = (uint32_t)__popcll(__ballot(k < n_blocks && magic_at(base, k)));
    if (lane_id() == 0 && wave_total) atomicAdd(&s_cnt, wave_total);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_cnt;
}

// the positions of the candidates, ascending
__global__ __launch_bounds__(TILE_BLOCKS) void tar_emit_kernel(const uint8_t *base, uint64_t n_blocks, const uint64_t *tile_cnt, const uint64_t *tile_excl,
                                                               const uint64_t *tile_part, uint64_t *pos, uint32_t n_cand, TarDev *ds)
{
    __shared__ uint32_t s_wave[TILE_BLOCKS / 64];
    const uint64_t want = tile_cnt[blockIdx.x];
    if (want == 0) return;  // (uniform) the tiles inside a large member
    const uint64_t first = tile_excl[blockIdx.x] + tile_part[blockIdx.x / SCAN_THREADS];
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t k = (uint64_t)blockIdx.x * TILE_BLOCKS + threadIdx.x;
    const bool is = k < n_blocks && magic_at(base, k);
    const uint64_t mask = __ballot(is);
    if (lane_id() == 0) s_wave[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < TILE_BLOCKS / 64; w++) {
        before += w < wave ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    if (is) {
        const uint64_t idx = first + before + (uint32_t)__popcll(mask & lanemask_lt());
        if (idx < n_cand) pos[idx] = k * tar::BLOCK;
        else ds->fault = 1;
    }
    if (threadIdx.x == 0 && total != want) ds->fault = 1;
}

// the walk that stops at position 0 (what stands unless the candidate at 0 is marked: the output kernel then says otherwise)
__global__ void tar_stop0_kernel(const uint8_t *base, uint64_t len, TarDev *ds)
{
    if (threadIdx.x || blockIdx.x) return;
    const tar::Stop st = tar::stop_at(base, len, 0);
    ds->stop_off = ds->bad_off = 0;
    ds->status = st.status, ds->zero_blocks = st.zero_blocks;
}

// per candidate: the end of its group, info = verdict | kind << 8, the offending header, the member's record.  A position that is no
// candidate (the data changed under the kernels) is a fault, and a bad header so that nothing follows it.
__global__ __launch_bounds__(256) void tar_describe_kernel(const uint8_t *base, uint64_t len, const uint64_t *pos, uint32_t n_cand, uint64_t *end,
                                                           uint64_t *bad, uint32_t *info, chip_tar_entry *rec, TarDev *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    const uint64_t p = pos[i];
    tar::Group g;
    g.end = 0, g.bad_off = p, g.verdict = CHIP_TAR_BAD_HEADER, g.kind = tar::KIND_MEMBER;
    g.ent = chip_tar_entry{};
    if ((p & (tar::BLOCK - 1)) || p > len || len - p < tar::BLOCK || !magic_at(base, p / tar::BLOCK)) ds->fault = 1;
    else if (tar::is_header(base, len, p)) tar::read_group(base, len, p, g);
    end[i] = g.end;
    bad[i] = g.bad_off;
    info[i] = (uint32_t)g.verdict | (g.kind << 8);
    rec[i] = g.ent;
}

// jump[i] = index of the candidate a whole group at candidate i leads to, n_cand (the sink) for everything else; starts the marks
__global__ __launch_bounds__(256) void tar_succ_kernel(const uint64_t *pos, const uint64_t *end, const uint32_t *info, uint32_t n_cand, uint32_t *jump,
                                                       uint32_t *marked)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    jump[i] = (info[i] & 0xffu) == 0 ? candidate_at(pos, i + 1u, n_cand, end[i]) : n_cand;
    marked[i] = (i == 0 && pos[0] == 0) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void tar_flags_kernel(const uint32_t *info, const chip_tar_entry *rec, const uint32_t *marked, uint32_t n_cand,
                                                        TarAcc *acc)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    TarAcc a{0, 0, 0};
    if (marked[i] && (info[i] & 0xffu) == 0) {
        if ((info[i] >> 8) == tar::KIND_GLOBAL) a.globals = 1;
        else a.members = 1, a.bytes = rec[i].size;
    }
    acc[i] = a;
}

__global__ __launch_bounds__(256) void tar_output_kernel(const uint8_t *base, uint64_t len, const uint64_t *pos, const uint64_t *end, const uint64_t *bad,
                                                         const uint32_t *info, const chip_tar_entry *rec, const uint32_t *marked, const uint32_t *jump,
                                                         const TarAcc *acc, const TarAcc *acc_part, uint32_t n_cand, uint64_t max_entries,
                                                         chip_tar_entry *entries, TarDev *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand || !marked[i]) return;
    const uint32_t verdict = info[i] & 0xffu;
    // the one marked candidate without a successor: where the walk stopped
    if (verdict != 0) {
        ds->stop_off = pos[i], ds->bad_off = bad[i];
        ds->status = (int32_t)verdict, ds->zero_blocks = 0;
        return;
    }
    if ((info[i] >> 8) == tar::KIND_MEMBER) {
        const uint64_t k = acc[i].members + acc_part[i / SCAN_THREADS].members;
        if (k < max_entries) entries[k] = rec[i];
    }
    if (jump[i] >= n_cand) {
        const uint64_t q = end[i];
        if (q > len) {  // (read_group checked it)
            ds->fault = 1;
            return;
        }
        const tar::Stop st = tar::stop_at(base, len, q);
        ds->stop_off = ds->bad_off = q;
        ds->status = st.status, ds->zero_blocks = st.zero_blocks;
    }
}

using TarSlot = SummarySlot<TarDev>;
SlotCache<TarSlot> g_tar_cache;

// The plan of base[0 .. len), len > 0: enqueues everything, waits twice (candidate count, summary).  The caller holds the cache's
// lock.  Buffer 0 holds the tile counts and their scan (16 bytes per 128 KiB of input), buffer 1 the candidate tables
// (128 + 4 * levels bytes per candidate).
hipError_t tar_plan_locked(TarSlot &sl, const uint8_t *base, uint64_t len, uint64_t max_entries, chip_tar_entry *entries, hipStream_t stream,
                           chip_tar_plan_summary &out, bool &too_many)
{
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    TarDev *ds = sl.d_sum;
    if ((e = hipMemsetAsync(ds, 0, sizeof(TarDev), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(tar_stop0_kernel, dim3(1), dim3(64), 0, stream, base, len, ds);
    const uint64_t n_blocks = len / tar::BLOCK, n_tiles = (n_blocks + TILE_BLOCKS - 1) / TILE_BLOCKS;
    uint64_t *tile_cnt = nullptr, *tile_excl = nullptr, *tile_part = nullptr;
    if (n_tiles) {
        if ((e = sl.grow(0, (size_t)(2 * n_tiles + scan_parts(n_tiles)) * 8)) != hipSuccess) return e;
        tile_cnt = (uint64_t *)sl.buf[0], tile_excl = tile_cnt + n_tiles, tile_part = tile_excl + n_tiles;
        hipLaunchKernelGGL(tar_count_kernel, dim3((uint32_t)n_tiles), dim3(TILE_BLOCKS), 0, stream, base, n_blocks, tile_cnt);
        enqueue_scan<uint64_t>(tile_cnt, tile_excl, n_tiles, tile_part, &ds->cand, stream);
    }
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    auto answer = [&](const TarDev &h) {
        out = chip_tar_plan_summary{h.sum.members, h.sum.globals, h.sum.bytes, h.stop_off, h.bad_off, h.status, h.zero_blocks};
    };
    const uint64_t cand64 = sl.h_sum->cand;
    if (cand64 == 0) {  // no header anywhere: the walk stops at position 0
        answer(*sl.h_sum);
        return hipSuccess;
    }
    if (cand64 > 0x7fffffffull) {
        too_many = true;
        return hipSuccess;
    }
    if (cand64 > n_blocks) return hipErrorUnknown;
    const uint32_t n_cand = (uint32_t)cand64, levels = jump_levels(n_cand);
    const size_t o_acc = 0, o_part = o_acc + (size_t)n_cand * sizeof(TarAcc), o_rec = up16(o_part + (size_t)scan_parts(n_cand) * sizeof(TarAcc));
    const size_t o_pos = up16(o_rec + (size_t)n_cand * sizeof(chip_tar_entry)), o_end = o_pos + (size_t)n_cand * 8, o_bad = o_end + (size_t)n_cand * 8;
    const size_t o_info = up16(o_bad + (size_t)n_cand * 8), o_mark = up16(o_info + (size_t)n_cand * 4), o_jump = up16(o_mark + (size_t)n_cand * 4);
    const size_t jump_stride = up16((size_t)n_cand * 4);
    if ((e = sl.grow(1, o_jump + jump_stride * levels)) != hipSuccess) return e;
    uint8_t *c = sl.buf[1];
    TarAcc *acc = (TarAcc *)(c + o_acc), *acc_part = (TarAcc *)(c + o_part);
    chip_tar_entry *rec = (chip_tar_entry *)(c + o_rec);
    uint64_t *pos = (uint64_t *)(c + o_pos), *end = (uint64_t *)(c + o_end), *bad = (uint64_t *)(c + o_bad);
    uint32_t *info = (uint32_t *)(c + o_info), *marked = (uint32_t *)(c + o_mark);
    auto jump = [&](uint32_t k) { return (uint32_t *)(c + o_jump + jump_stride * k); };
    const dim3 cgrid((n_cand + 255u) / 256u);

    hipLaunchKernelGGL(tar_emit_kernel, dim3((uint32_t)n_tiles), dim3(TILE_BLOCKS), 0, stream, base, n_blocks, (const uint64_t *)tile_cnt,
                       (const uint64_t *)tile_excl, (const uint64_t *)tile_part, pos, n_cand, ds);
    hipLaunchKernelGGL(tar_describe_kernel, cgrid, dim3(256), 0, stream, base, len, (const uint64_t *)pos, n_cand, end, bad, info, rec, ds);
    hipLaunchKernelGGL(tar_succ_kernel, cgrid, dim3(256), 0, stream, (const uint64_t *)pos, (const uint64_t *)end, (const uint32_t *)info, n_cand, jump(0),
                       marked);
    for (uint32_t k = 0; k + 1 < levels; k++)
        hipLaunchKernelGGL(plan_double_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), jump(k + 1), n_cand);
    for (uint32_t k = levels; k-- > 0;) hipLaunchKernelGGL(plan_mark_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)jump(k), marked, n_cand);
    hipLaunchKernelGGL(tar_flags_kernel, cgrid, dim3(256), 0, stream, (const uint32_t *)info, (const chip_tar_entry *)rec, (const uint32_t *)marked, n_cand,
                       acc);
    enqueue_scan<TarAcc>(acc, acc, n_cand, acc_part, &ds->sum, stream);
    hipLaunchKernelGGL(tar_output_kernel, cgrid, dim3(256), 0, stream, base, len, (const uint64_t *)pos, (const uint64_t *)end, (const uint64_t *)bad,
                       (const uint32_t *)info, (const chip_tar_entry *)rec, (const uint32_t *)marked, (const uint32_t *)jump(0), (const TarAcc *)acc,
                       (const TarAcc *)acc_part, n_cand, max_entries, entries, ds);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const TarDev &h = *sl.h_sum;
    if (h.fault || h.sum.members + h.sum.globals > n_cand) return hipErrorUnknown;  // the input changed between two passes
    answer(h);
    return hipSuccess;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_tar_plan_host(const uint8_t *in, uint64_t len, uint64_t max_entries, chip_tar_entry *entries, chip_tar_plan_summary *summary)
{
    if (!summary || (len && !in) || (max_entries && !entries) || len > ((uint64_t)1 << 40)) return CHIP_E_INVALID;
    tar::plan_host(in, len, max_entries, entries, summary);
    return CHIP_OK;
}

int chip_tar_plan(const void *in_base, uint64_t len, uint64_t max_entries, chip_tar_entry *entries, chip_tar_plan_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_entries && !entries) || ((uintptr_t)in_base & 3u) || len > ((uint64_t)1 << 40)) return CHIP_E_INVALID;
    constexpr chip_tar_plan_summary NOTHING{0, 0, 0, 0, 0, CHIP_TAR_OK, 0};
    *summary = NOTHING;
    if (len == 0) return CHIP_OK;
    chip_tar_plan_summary r = NOTHING;
    bool too_many = false;
    const int rc = with_slot(
        g_tar_cache, stream,
        [&](TarSlot &sl, hipStream_t s) { return tar_plan_locked(sl, (const uint8_t *)in_base, len, max_entries, entries, s, r, too_many); },
        [&] { *summary = NOTHING; });
    if (rc != CHIP_OK) return rc;
    if (too_many) return CHIP_E_NOMEM;
    *summary = r;
    return CHIP_OK;
}

}  // extern "C"
