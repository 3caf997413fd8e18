// One LZ4 frame: the description of its blocks (chip_lz4_blocks_host on the host, chip_lz4_blocks on the GPU) and its decode with a
// wave per block, chip_lz4_parallel.  A frame states every block's size in a 4-byte header, so the index is a
// hop over headers; with independent blocks (the `lz4` command's default) every block is a unit of the CHIP_FMT_LZ4_BLOCK batch.
#include "launch_slots.h"
#include "lz4_core.h"
#include "pack_copy.h"
#include "plan_common.h"

namespace chip {

namespace {

struct GlobalReader {
    const uint8_t *p;
    __device__ uint32_t byte(uint64_t pos) const { return p[pos]; }
};

// One lane hops over the block headers: every step needs the size the one before it read.
__global__ __launch_bounds__(64) void lz4_hop_kernel(const uint8_t *in, uint64_t len, uint64_t max_blocks, chip_lz4_block *blocks, chip_lz4_blocks_summary *sum)
{
    if (threadIdx.x != 0) return;
    GlobalReader rd{in};
    *sum = lz4::walk_blocks(rd, len, max_blocks, blocks);
}

typedef SummarySlot<chip_lz4_blocks_summary> Lz4BlocksSlot;
SlotCache<Lz4BlocksSlot> g_lz4blocks_cache;

constexpr chip_lz4_blocks_summary NO_FRAME = {0, 0, CHIP_LZ4BLOCKS_UNSIZED, 0, 0, 0, 0, 0, CHIP_ZPLAN_TRUNCATED};

// ---- chip_lz4_parallel ----------------------------------------------------------------------------------------------------------
// What the kernels leave for the host, and the one unit of the serial path (its BatchArgs point into this block).
struct Lz4ParDev {
    uint64_t in_off, out_off;
    uint32_t in_len, out_cap, out_len, in_used;
    int32_t status;
    uint32_t check;     // the content checksum computed
    uint32_t n_bad;     // blocks the size pass, the decode or a block checksum did not accept
    uint32_t n_stored;  // stored blocks with bytes
    chip_lz4_blocks_summary walk;
};

// The per-block arrays of one frame in the slot's second buffer, n entries each.
struct Lz4ParArrays {
    uint64_t *in_off, *out_size, *out_off;
    uint32_t *in_len, *out_cap, *out_len, *in_used, *src_len, *digest, *full_len;
    int32_t *status;
    static size_t bytes(uint64_t n) { return (size_t)n * 56 + 64; }
    explicit Lz4ParArrays(uint8_t *b, uint64_t n)
    {
        in_off = (uint64_t *)b;
        out_size = in_off + n;
        out_off = out_size + n;
        in_len = (uint32_t *)(out_off + n);
        out_cap = in_len + n;
        out_len = out_cap + n;
        in_used = out_len + n;
        src_len = in_used + n;
        digest = src_len + n;
        full_len = digest + n;
        status = (int32_t *)(full_len + n);
    }
};

struct Lz4ParSlot : SummarySlot<Lz4ParDev> {};
SlotCache<Lz4ParSlot> g_lz4par_cache;

__global__ __launch_bounds__(64) void lz4par_init_kernel(Lz4ParDev *d, uint64_t in_len, uint64_t out_cap)
{
    if (threadIdx.x != 0) return;
    d->in_off = d->out_off = 0;
    d->in_len = (uint32_t)in_len;
    d->out_cap = (uint32_t)out_cap;
    d->out_len = d->in_used = 0;
    d->status = CHIP_NEED_INPUT;
    d->check = d->n_bad = d->n_stored = 0;
}

// the blocks as units of a CHIP_FMT_LZ4_BLOCK batch: a stored block is an empty unit (it decodes nothing and writes nothing)
__global__ __launch_bounds__(256) void lz4par_units_kernel(const chip_lz4_block *blocks, uint32_t n, Lz4ParArrays a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const chip_lz4_block b = blocks[i];
    const bool stored = b.flags & CHIP_LZ4BLOCK_STORED;
    a.in_off[i] = b.offset + 4;
    a.in_len[i] = stored ? 0u : b.size;
    a.src_len[i] = stored ? b.size : 0u;
    a.full_len[i] = b.size;
}

// behind the size pass: a stored block's size is its own; a compressed block must have been counted to its end, within block_max
__global__ __launch_bounds__(256) void lz4par_sizes_kernel(uint32_t n, Lz4ParArrays a, uint32_t block_max, Lz4ParDev *d)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (a.src_len[i] || a.in_len[i] == 0) {  // stored (an empty stored block included)
        a.out_size[i] = a.src_len[i];
        if (a.src_len[i]) atomicAdd(&d->n_stored, 1u);
    } else if (a.status[i] != CHIP_FINISHED || a.out_size[i] > block_max) {
        atomicAdd(&d->n_bad, 1u);
    }
}

// behind the decode and the checksum batch
__global__ __launch_bounds__(256) void lz4par_verify_kernel(const chip_lz4_block *blocks, uint32_t n, Lz4ParArrays a, uint32_t block_checksums, Lz4ParDev *d)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    bool bad = false;
    if (a.in_len[i]) bad = a.status[i] != CHIP_FINISHED || a.out_len[i] != a.out_cap[i];
    if (block_checksums && a.digest[i] != blocks[i].checksum) bad = true;
    if (bad) atomicAdd(&d->n_bad, 1u);
}

struct Lz4ParCall {
    const uint8_t *in;
    uint64_t len;
    uint8_t *out;
    uint64_t out_cap;
    uint32_t flags;
    chip_lz4_parallel_summary *sum;
};

hipError_t hop(const uint8_t *in, uint64_t len, uint64_t max_blocks, chip_lz4_block *blocks, chip_lz4_blocks_summary *d_sum, hipStream_t s)
{
    hipLaunchKernelGGL(lz4_hop_kernel, dim3(1), dim3(64), 0, s, in, len, max_blocks, blocks, d_sum);
    return hipGetLastError();
}

// the one-unit CHIP_FMT_LZ4 decode, the arbiter of every verdict
hipError_t lz4par_serial(Lz4ParSlot &sl, const Lz4ParCall &c, uint64_t unit_len, hipStream_t s)
{
    if (unit_len > 0xFFFFFFFFull || c.out_cap > 0xFFFFFFFFull) {
        c.sum->path = CHIP_LZ4PAR_REFUSED;
        return hipSuccess;
    }
    Lz4ParDev *const d = sl.d_sum;
    hipLaunchKernelGGL(lz4par_init_kernel, dim3(1), dim3(64), 0, s, d, unit_len, c.out_cap);
    BatchArgs a;
    a.in_base = c.in;
    a.in_off = &d->in_off;
    a.in_len = &d->in_len;
    a.out_base = c.out;
    a.out_off = &d->out_off;
    a.out_cap = &d->out_cap;
    a.out_len = &d->out_len;
    a.in_used = &d->in_used;
    a.status = &d->status;
    a.n = 1;
    a.format = CHIP_FMT_LZ4;
    a.stats = nullptr;
    a.resume = nullptr;
    hipError_t e = launch_lz4(a, nullptr, s);
    if (e != hipSuccess) return e;
    if ((e = sl.fetch(s)) != hipSuccess) return e;
    c.sum->path = CHIP_LZ4PAR_SERIAL;
    c.sum->status = sl.h_sum->status;
    c.sum->out_len = sl.h_sum->out_len;
    c.sum->in_used = sl.h_sum->in_used;
    c.sum->total_out = sl.h_sum->out_len;
    c.sum->check = 0;
    return hipSuccess;
}

// serial = true on return: not clean, the serial path decides; unit_len: the bytes that path gets
hipError_t lz4par_parallel(Lz4ParSlot &sl, const Lz4ParCall &c, hipStream_t s, bool &serial, uint64_t &unit_len)
{
    serial = true;
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    Lz4ParDev *const d = sl.d_sum;
    // 1. the walk, into the records the slot has room for; a frame of more blocks is walked again
    hipLaunchKernelGGL(lz4par_init_kernel, dim3(1), dim3(64), 0, s, d, 0, 0);
    if ((e = sl.grow(0, 4096 * sizeof(chip_lz4_block))) != hipSuccess) return e;
    chip_lz4_blocks_summary w;
    for (;;) {
        const uint64_t room = sl.cap[0] / sizeof(chip_lz4_block);
        if ((e = hop(c.in, c.len, room, (chip_lz4_block *)sl.buf[0], &d->walk, s)) != hipSuccess) return e;
        if ((e = sl.fetch(s)) != hipSuccess) return e;
        w = sl.h_sum->walk;
        if (w.n_blocks <= room) break;
        if ((e = sl.grow(0, (size_t)w.n_blocks * sizeof(chip_lz4_block))) != hipSuccess) return e;
    }
    c.sum->n_blocks = w.n_blocks;
    if (w.status == CHIP_ZPLAN_OK) unit_len = w.in_used;
    if (w.status != CHIP_ZPLAN_OK || !((w.flg >> 5) & 1u) || w.n_blocks < 2) return hipSuccess;
    const uint32_t n = (uint32_t)w.n_blocks;  // (at most CHIP_ZPLAN_MAX_BLOCKS)
    const chip_lz4_block *const blocks = (const chip_lz4_block *)sl.buf[0];
    if ((e = sl.grow(1, Lz4ParArrays::bytes(n))) != hipSuccess) return e;
    const Lz4ParArrays A(sl.buf[1], n);
    const dim3 grid((n + 255u) / 256u);
    // 2. the size pass over the blocks
    hipLaunchKernelGGL(lz4par_units_kernel, grid, dim3(256), 0, s, blocks, n, A);
    BatchArgs a;
    a.in_base = c.in;
    a.in_off = A.in_off;
    a.in_len = A.in_len;
    a.out_base = nullptr;
    a.out_off = nullptr;
    a.out_cap = nullptr;
    a.out_len = nullptr;
    a.in_used = A.in_used;
    a.status = A.status;
    a.n = n;
    a.format = CHIP_FMT_LZ4_BLOCK;
    a.stats = nullptr;
    a.resume = nullptr;
    if ((e = launch_lz4(a, A.out_size, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(lz4par_sizes_kernel, grid, dim3(256), 0, s, n, A, w.block_max, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // 3. the layout: a device scan (it waits for the stream)
    uint64_t total = 0, n_over = 0;
    if (chip_layout_units(n, A.out_size, A.out_off, A.out_cap, &total, &n_over, s) != CHIP_OK) return hipErrorUnknown;
    if ((e = sl.fetch(s)) != hipSuccess) return e;
    if (sl.h_sum->n_bad || n_over) return hipSuccess;
    if (w.content_size != CHIP_LZ4BLOCKS_UNSIZED && w.content_size != total) return hipSuccess;
    const uint32_t n_stored = sl.h_sum->n_stored;
    serial = false;
    c.sum->path = CHIP_LZ4PAR_PARALLEL;
    c.sum->total_out = total;
    if (total > c.out_cap) {
        c.sum->status = CHIP_NEED_OUTPUT;
        return hipSuccess;
    }
    // 4. the blocks straight into out_base, 5. the stored ones by the file writer's copy (units of length 0 are stepped over)
    a.out_base = c.out;
    a.out_off = A.out_off;
    a.out_cap = A.out_cap;
    a.out_len = A.out_len;
    if ((e = launch_lz4(a, nullptr, s)) != hipSuccess) return e;
    if (n_stored && total) enqueue_copy(n, c.in, A.in_off, A.src_len, c.out, A.out_off, total, s);
    // 6. the block checksums, 7. the content checksum on one wave
    const uint32_t bchk = (w.flg >> 4) & 1u;
    if (bchk && chip_xxh32_batch(n, c.in, A.in_off, A.full_len, 0, A.digest, s) != CHIP_OK) return hipErrorUnknown;
    hipLaunchKernelGGL(lz4par_verify_kernel, grid, dim3(256), 0, s, blocks, n, A, bchk, d);
    const bool cchk = ((w.flg >> 2) & 1u) && !(c.flags & CHIP_LZ4PAR_NO_CHECKSUM);
    if (cchk && (e = launch_lz4_xxh(c.out, total, &d->check, s)) != hipSuccess) return e;
    if ((e = sl.fetch(s)) != hipSuccess) return e;
    if (sl.h_sum->n_bad || (cchk && sl.h_sum->check != w.content_checksum)) {
        serial = true;
        return hipSuccess;
    }
    c.sum->status = CHIP_FINISHED;
    c.sum->out_len = total;
    c.sum->in_used = w.in_used;
    c.sum->check = cchk ? sl.h_sum->check : 0;
    return hipSuccess;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_lz4_blocks_host(const uint8_t *in, uint64_t len, uint64_t max_blocks, chip_lz4_block *blocks, chip_lz4_blocks_summary *summary)
{
    if (!summary || (len && !in) || (max_blocks && !blocks)) return CHIP_E_INVALID;
    lz4::MemReader rd{in};
    *summary = lz4::walk_blocks(rd, len, max_blocks, blocks);
    return CHIP_OK;
}

int chip_lz4_blocks(const void *in_base, uint64_t len, uint64_t max_blocks, chip_lz4_block *blocks, chip_lz4_blocks_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_blocks && !blocks) || ((uintptr_t)in_base & 3u) || len > ((uint64_t)1 << 40)) return CHIP_E_INVALID;
    *summary = NO_FRAME;
    if (len < 7) return CHIP_OK;  // (what the walk says of it)
    return with_slot(
        g_lz4blocks_cache, stream,
        [&](Lz4BlocksSlot &sl, hipStream_t s) {
            hipError_t e = sl.summary();
            if (e != hipSuccess) return e;
            if ((e = hop((const uint8_t *)in_base, len, max_blocks, blocks, sl.d_sum, s)) != hipSuccess) return e;
            if ((e = sl.fetch(s)) != hipSuccess) return e;
            *summary = *sl.h_sum;
            return hipSuccess;
        },
        [&] { *summary = NO_FRAME; });
}

int chip_lz4_parallel(const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, uint32_t flags, chip_lz4_parallel_summary *summary,
                      void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (out_cap && !out_base) || ((uintptr_t)in_base & 3u) || (flags & ~CHIP_LZ4PAR_NO_CHECKSUM) ||
        len > ((uint64_t)1 << 40))
        return CHIP_E_INVALID;
    const auto blank = [&] { *summary = chip_lz4_parallel_summary{0, 0, 0, 0, CHIP_NEED_INPUT, CHIP_LZ4PAR_SERIAL, 0, 0}; };
    blank();
    const Lz4ParCall c{(const uint8_t *)in_base, len, (uint8_t *)out_base, out_cap, flags, summary};
    return with_slot(
        g_lz4par_cache, stream,
        [&](Lz4ParSlot &sl, hipStream_t s) {
            bool serial = true;
            uint64_t unit_len = c.len;
            hipError_t e = lz4par_parallel(sl, c, s, serial, unit_len);
            if (e == hipSuccess && serial) e = lz4par_serial(sl, c, unit_len, s);
            return e;
        },
        blank);
}

}  // extern "C"
