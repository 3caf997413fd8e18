// The member index of a buffer of gzip members (WARC records, `pigz -i` output, `cat a.gz b.gz`, the files
// chip_encode_file(CHIP_FMT_GZIP) writes): chip_gzip_plan.  DESIGN.md sec. 4.15.
//
// The plan of a buffer is DEFINED by the serial walk of include/compu_hip.h.  A member does not state its length, so the walk's
// per-member part is an inflate: the size pass (chip_decode_batch_sizes, inflate_sizes.hip) over the unit that starts at the member
// and reaches to the end of the buffer; its in_used is the member's length.  The GPU version is the plan pipeline of plan_common.h
// ("The container plan") with the format below and a describe phase of its own.
//   candidates  every byte position is tested in 16-byte loads for `1f 8b 08` and a FLG byte without reserved bits
//   describe    gzip_room_kernel: in_len of candidate i = what lies behind it, at most CHIP_GZPLAN_WINDOW;
//               launch_inflate() with out_size: one wave per candidate, all members (and all decoys) in parallel, pos[] is the batch's in_off;
//               gzip_convert_kernel: (status, out_size, in_used) becomes end / cap / verdict by the rules of the walk
// What the marking never reaches is a decoy: header bytes inside a stored block, a whole member inside an FEXTRA field, an MTIME
// that spells the magic.  A decoy's size pass ends with an error or at the end of the buffer like any damaged unit's.
// Locks: the plan's cache first, then the inflate slot's (launch_inflate takes it itself), the order read_ranges.hip has;
// nothing in inflate.hip takes a plan's lock.
#include "chip_internal.h"
#include "launch_slots.h"
#include "plan_common.h"

namespace chip {

namespace {

constexpr uint32_t GZIP_MAGIC = 0x00088B1Fu, GZIP_MASK = 0xE0FFFFFFu;  // 1f 8b 08, FLG & 0xe0 == 0 (little endian)
static_assert(CHIP_GZPLAN_WINDOW * 8ull + 24 <= 0xFFFFFFFFull, "the inflate kernels' 32-bit bit cursor: 3 bytes of misalignment + in_len");

__host__ __device__ __forceinline__ bool is_member_start(uint32_t w) { return (w & GZIP_MASK) == GZIP_MAGIC; }

struct GzipFormat {
    static constexpr uint32_t MIN_HEADER = 4;

    // candidates of chunk g as a 16-bit mask: the positions whose four bytes, all in front of `len`, start a member
    static __device__ __forceinline__ uint32_t candidates(const uint8_t *base, uint64_t len, uint64_t n_chunks, uint64_t g)
    {
        if (g >= n_chunks) return 0;
        uint32_t w[5];
        load_chunk(base, (len + 3) & ~(uint64_t)3, g, w);
        uint32_t m = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) m |= (is_member_start(chunk_word(w, k)) ? 1u : 0u) << k;
        const uint64_t b = g * 16;
        if (b + 20 > len) {  // (the last two chunks) drop what reaches behind len: the padding up to len4 holds anything
#pragma unroll
            for (uint32_t k = 0; k < 16; k++)
                if (b + k + 4 > len) m &= ~(1u << k);
        }
        return m;
    }
};

// the plan's summary, and the size pass's status of the member the walk refused
struct DevSummary : PlanSummary {
    int32_t member_status;
    uint32_t pad;
};

// the describe phase's scratch of n candidates: the size batch's in_len and its three answers (20 bytes per candidate)
struct SizeArrays {
    uint64_t *out_size;
    uint32_t *in_len, *in_used;
    int32_t *status;
    SizeArrays(const uint8_t *extra, uint32_t n)
        : out_size((uint64_t *)extra), in_len((uint32_t *)(extra + (size_t)n * 8)), in_used((uint32_t *)(extra + (size_t)n * 12)),
          status((int32_t *)(extra + (size_t)n * 16))
    {
    }
};

// in_len of the size batch: candidate i's unit reaches to the end of the buffer, or as far as a unit may.  A position out of
// range (the data changed under the kernels) gets an empty unit; gzip_convert_kernel reports it.
__global__ __launch_bounds__(256) void gzip_room_kernel(const uint64_t *pos, uint32_t n_cand, uint64_t len, uint32_t *in_len)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    const uint64_t p = pos[i], room = p < len ? len - p : 0;
    in_len[i] = room < CHIP_GZPLAN_WINDOW ? (uint32_t)room : CHIP_GZPLAN_WINDOW;
}

// per candidate: end position, cap, info = verdict (kind: KIND_FRAME, every member is a unit), by the rules of the walk.  A
// position that is no candidate (any more), or an answer that cannot be one for its unit, is a fault, and a bad header so that
// nothing follows it.
__global__ __launch_bounds__(256) void gzip_convert_kernel(const uint8_t *base, uint64_t len, const uint64_t *pos, uint32_t n_cand,
                                                           const uint32_t *in_len, const int32_t *status, const uint64_t *out_size,
                                                           const uint32_t *in_used, uint64_t *end, uint32_t *cap, uint32_t *info, PlanSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand) return;
    const uint64_t p = pos[i];
    const int32_t st = status[i];
    const uint64_t size = out_size[i];
    const uint32_t room = in_len[i], iu = in_used[i];
    uint64_t e = 0;
    uint32_t c = 0, verdict = 0;
    bool gone = !(p < len && len - p >= 4);
    if (!gone) {
        const uint32_t w = (uint32_t)base[p] | ((uint32_t)base[p + 1] << 8) | ((uint32_t)base[p + 2] << 16) | ((uint32_t)base[p + 3] << 24);
        gone = !is_member_start(w);
    }
    if (!gone) {
        if (st == CHIP_NEED_INPUT) verdict = room < len - p ? CHIP_GZPLAN_TOO_LARGE : CHIP_GZPLAN_TRUNCATED;
        else if (st != CHIP_FINISHED) verdict = CHIP_GZPLAN_BAD_MEMBER;
        else if (size > 0xFFFFFFFEull) verdict = CHIP_GZPLAN_TOO_LARGE;
        else if (iu < 4 || iu > room) gone = true;  // (a finished member holds its header)
        else e = p + iu, c = (uint32_t)size;
    }
    if (gone) {
        verdict = (uint32_t)PLAN_BAD_HEADER;
        ds->fault = 1;
    }
    end[i] = e;
    cap[i] = c;
    info[i] = verdict | (KIND_FRAME << 8);
}

// behind the output kernel: the one marked candidate whose verdict is BAD_MEMBER says what the size pass said
__global__ __launch_bounds__(256) void gzip_member_status_kernel(const uint32_t *info, const uint32_t *marked, const int32_t *status,
                                                                 uint32_t n_cand, DevSummary *ds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_cand || !marked[i]) return;
    if ((info[i] & 0xffu) == (uint32_t)CHIP_GZPLAN_BAD_MEMBER) ds->member_status = status[i];
}

// the describe phase of plan_locked (plan_common.h, KernelDescribe)
struct SizePassDescribe {
    static constexpr size_t EXTRA = 20;

    static hipError_t describe(const uint8_t *base, uint64_t len, const uint64_t *pos, uint32_t n_cand, uint64_t *end, uint32_t *cap,
                               uint32_t *info, uint8_t *extra, PlanSummary *ds, hipStream_t stream)
    {
        const SizeArrays s(extra, n_cand);
        const dim3 cgrid((n_cand + 255u) / 256u);
        hipLaunchKernelGGL(gzip_room_kernel, cgrid, dim3(256), 0, stream, pos, n_cand, len, s.in_len);
        BatchArgs a{};
        a.in_base = base;
        a.in_off = pos;
        a.in_len = s.in_len;
        a.in_used = s.in_used;
        a.status = s.status;
        a.n = n_cand;
        a.format = CHIP_FMT_GZIP;
        const hipError_t e = launch_inflate(a, s.out_size, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gzip_convert_kernel, cgrid, dim3(256), 0, stream, base, len, pos, n_cand, (const uint32_t *)s.in_len,
                           (const int32_t *)s.status, (const uint64_t *)s.out_size, (const uint32_t *)s.in_used, end, cap, info, ds);
        return hipSuccess;
    }

    static void finish(const uint32_t *info, const uint32_t *marked, uint32_t n_cand, const uint8_t *extra, PlanSummary *ds, hipStream_t stream)
    {
        const SizeArrays s(extra, n_cand);
        hipLaunchKernelGGL(gzip_member_status_kernel, dim3((n_cand + 255u) / 256u), dim3(256), 0, stream, info, marked, (const int32_t *)s.status,
                           n_cand, static_cast<DevSummary *>(ds));
    }
};

using GzplanSlot = SummarySlot<DevSummary>;
SlotCache<GzplanSlot> g_gzplan_cache;

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_gzip_plan(const void *in_base, uint64_t len, uint64_t max_members, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                   uint32_t *out_cap, chip_gzip_plan_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_members && (!in_off || !in_len || !out_off || !out_cap)) || ((uintptr_t)in_base & 3u) ||
        len > ((uint64_t)1 << 40))
        return CHIP_E_INVALID;
    *summary = chip_gzip_plan_summary{0, 0, 0, CHIP_GZPLAN_OK, 0};
    if (len == 0) return CHIP_OK;
    PlanSummary r{};
    int32_t member_status = 0;
    bool too_many = false;
    const int rc = with_slot(
        g_gzplan_cache, stream,
        [&](GzplanSlot &sl, hipStream_t s) {
            const hipError_t e = plan_locked<GzipFormat, SizePassDescribe>(sl, (const uint8_t *)in_base, len, max_members, in_off, in_len, out_off,
                                                                           out_cap, s, r, too_many);
            if (e == hipSuccess && r.status == CHIP_GZPLAN_BAD_MEMBER) member_status = sl.h_sum->member_status;
            return e;
        },
        [&] { *summary = chip_gzip_plan_summary{0, 0, 0, CHIP_GZPLAN_BAD_HEADER, 0}; });
    if (rc != CHIP_OK) return rc;
    if (too_many) return CHIP_E_NOMEM;
    *summary = chip_gzip_plan_summary{r.sum.frames, r.sum.bytes, r.in_used, r.status, member_status};
    return CHIP_OK;
}

}  // extern "C"
