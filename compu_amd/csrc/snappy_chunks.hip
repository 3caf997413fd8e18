// One stream of the Snappy framing format: the description of its data chunks (chip_snappy_chunks_host on the host,
// chip_snappy_chunks on the GPU) and its decode with a wave per chunk, chip_snappy_parallel.  A chunk states
// its size in a 4-byte header, holds at most 65 536 bytes of content, carries a CRC of its own and never refers to another chunk:
// the index is a hop over headers, and every compressed chunk is a unit of the CHIP_FMT_SNAPPY_BLOCK batch.
#include "launch_slots.h"
#include "pack_copy.h"
#include "plan_common.h"
#include "snappy_core.h"

namespace chip {

namespace {

struct GlobalReader {
    const uint8_t *p;
    __device__ uint32_t byte(uint64_t pos) const { return p[pos]; }
};

// One lane hops over the chunk headers: every step needs the size the one before it read.
__global__ __launch_bounds__(64) void snappy_hop_kernel(const uint8_t *in, uint64_t len, uint64_t max_chunks, chip_snappy_chunk *chunks,
                                                        chip_snappy_chunks_summary *sum)
{
    if (threadIdx.x != 0) return;
    GlobalReader rd{in};
    *sum = snappy::walk_chunks(rd, len, max_chunks, chunks);
}

typedef SummarySlot<chip_snappy_chunks_summary> SnappyChunksSlot;
SlotCache<SnappyChunksSlot> g_snappychunks_cache;

constexpr chip_snappy_chunks_summary NO_STREAM = {0, 0, 0, CHIP_ZPLAN_TRUNCATED, 0};

// ---- chip_snappy_parallel --------------------------------------------------------------------------------------------------------
// What the kernels leave for the host, and the one unit of the serial path (its BatchArgs point into this block).
struct SnappyParDev {
    uint64_t in_off, out_off;
    uint32_t in_len, out_cap, out_len, in_used;
    int32_t status;
    uint32_t n_bad;     // chunks the size pass, the decode or the CRC did not accept
    uint32_t n_stored;  // uncompressed chunks with bytes
    uint32_t pad;
    chip_snappy_chunks_summary walk;
};

// The per-chunk arrays of one stream in the slot's second buffer, n entries each.
struct SnappyParArrays {
    uint64_t *in_off, *out_size, *out_off;
    uint32_t *in_len, *out_cap, *out_len, *in_used, *src_len, *crc;
    int32_t *status;
    static size_t bytes(uint64_t n) { return (size_t)n * 52 + 64; }
    explicit SnappyParArrays(uint8_t *b, uint64_t n)
    {
        in_off = (uint64_t *)b;
        out_size = in_off + n;
        out_off = out_size + n;
        in_len = (uint32_t *)(out_off + n);
        out_cap = in_len + n;
        out_len = out_cap + n;
        in_used = out_len + n;
        src_len = in_used + n;
        crc = src_len + n;
        status = (int32_t *)(crc + n);
    }
};

struct SnappyParSlot : SummarySlot<SnappyParDev> {};
SlotCache<SnappyParSlot> g_snappypar_cache;

__global__ __launch_bounds__(64) void snappypar_init_kernel(SnappyParDev *d, uint64_t in_len, uint64_t out_cap)
{
    if (threadIdx.x != 0) return;
    d->in_off = d->out_off = 0;
    d->in_len = (uint32_t)in_len;
    d->out_cap = (uint32_t)out_cap;
    d->out_len = d->in_used = 0;
    d->status = CHIP_NEED_INPUT;
    d->n_bad = d->n_stored = 0;
}

// the chunks as units of a CHIP_FMT_SNAPPY_BLOCK batch: an uncompressed chunk is an empty unit (it decodes nothing and writes nothing)
__global__ __launch_bounds__(256) void snappypar_units_kernel(const chip_snappy_chunk *chunks, uint32_t n, SnappyParArrays a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const chip_snappy_chunk c = chunks[i];
    a.in_off[i] = c.offset + 8;
    a.in_len[i] = c.type ? 0u : c.size - 4;
    a.src_len[i] = c.type ? c.size - 4 : 0u;
}

// behind the size pass: an uncompressed chunk's size is its own; a compressed chunk must have been counted to its end; neither
// may hold more than 65 536 bytes
__global__ __launch_bounds__(256) void snappypar_sizes_kernel(const chip_snappy_chunk *chunks, uint32_t n, SnappyParArrays a, SnappyParDev *d)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    bool bad = false;
    if (chunks[i].type) {
        a.out_size[i] = a.src_len[i];
        if (a.src_len[i]) atomicAdd(&d->n_stored, 1u);
    } else {
        bad = a.status[i] != CHIP_FINISHED;
    }
    if (bad || a.out_size[i] > snappy::CHUNK_MAX) atomicAdd(&d->n_bad, 1u);
}

// behind the decode and the CRC batch
__global__ __launch_bounds__(256) void snappypar_verify_kernel(const chip_snappy_chunk *chunks, uint32_t n, SnappyParArrays a, SnappyParDev *d)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    bool bad = snappy::mask(a.crc[i]) != chunks[i].crc;
    if (!chunks[i].type && (a.status[i] != CHIP_FINISHED || a.out_len[i] != a.out_cap[i])) bad = true;
    if (bad) atomicAdd(&d->n_bad, 1u);
}

struct SnappyParCall {
    const uint8_t *in;
    uint64_t len;
    uint8_t *out;
    uint64_t out_cap;
    chip_snappy_parallel_summary *sum;
};

hipError_t hop(const uint8_t *in, uint64_t len, uint64_t max_chunks, chip_snappy_chunk *chunks, chip_snappy_chunks_summary *d_sum, hipStream_t s)
{
    hipLaunchKernelGGL(snappy_hop_kernel, dim3(1), dim3(64), 0, s, in, len, max_chunks, chunks, d_sum);
    return hipGetLastError();
}

// the one-unit CHIP_FMT_SNAPPY decode of the whole buffer, the arbiter of every verdict
hipError_t snappypar_serial(SnappyParSlot &sl, const SnappyParCall &c, hipStream_t s)
{
    if (c.len > 0xFFFFFFFFull || c.out_cap > 0xFFFFFFFFull) {
        c.sum->path = CHIP_SNAPPYPAR_REFUSED;
        return hipSuccess;
    }
    SnappyParDev *const d = sl.d_sum;
    hipLaunchKernelGGL(snappypar_init_kernel, dim3(1), dim3(64), 0, s, d, c.len, c.out_cap);
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
    a.format = CHIP_FMT_SNAPPY;
    a.stats = nullptr;
    a.resume = nullptr;
    hipError_t e = launch_snappy(a, nullptr, s);
    if (e != hipSuccess) return e;
    if ((e = sl.fetch(s)) != hipSuccess) return e;
    c.sum->path = CHIP_SNAPPYPAR_SERIAL;
    c.sum->status = sl.h_sum->status;
    c.sum->out_len = sl.h_sum->out_len;
    c.sum->in_used = sl.h_sum->in_used;
    c.sum->total_out = sl.h_sum->out_len;
    return hipSuccess;
}

// serial = true on return: not clean, the serial path decides
hipError_t snappypar_parallel(SnappyParSlot &sl, const SnappyParCall &c, hipStream_t s, bool &serial)
{
    serial = true;
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    SnappyParDev *const d = sl.d_sum;
    // 1. the walk, into the records the slot has room for; a stream of more chunks is walked again
    hipLaunchKernelGGL(snappypar_init_kernel, dim3(1), dim3(64), 0, s, d, 0, 0);
    if ((e = sl.grow(0, 4096 * sizeof(chip_snappy_chunk))) != hipSuccess) return e;
    chip_snappy_chunks_summary w;
    for (;;) {
        const uint64_t room = sl.cap[0] / sizeof(chip_snappy_chunk);
        if ((e = hop(c.in, c.len, room, (chip_snappy_chunk *)sl.buf[0], &d->walk, s)) != hipSuccess) return e;
        if ((e = sl.fetch(s)) != hipSuccess) return e;
        w = sl.h_sum->walk;
        if (w.n_chunks <= room) break;
        if ((e = sl.grow(0, (size_t)w.n_chunks * sizeof(chip_snappy_chunk))) != hipSuccess) return e;
    }
    c.sum->n_chunks = w.n_chunks;
    c.sum->n_skipped = (uint32_t)(w.n_skipped > 0xFFFFFFFFull ? 0xFFFFFFFFull : w.n_skipped);
    if (w.status != CHIP_ZPLAN_OK || w.n_chunks < 2) return hipSuccess;
    const uint32_t n = (uint32_t)w.n_chunks;  // (at most CHIP_ZPLAN_MAX_BLOCKS)
    const chip_snappy_chunk *const chunks = (const chip_snappy_chunk *)sl.buf[0];
    if ((e = sl.grow(1, SnappyParArrays::bytes(n))) != hipSuccess) return e;
    const SnappyParArrays A(sl.buf[1], n);
    const dim3 grid((n + 255u) / 256u);
    // 2. the size pass over the chunks
    hipLaunchKernelGGL(snappypar_units_kernel, grid, dim3(256), 0, s, chunks, n, A);
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
    a.format = CHIP_FMT_SNAPPY_BLOCK;
    a.stats = nullptr;
    a.resume = nullptr;
    if ((e = launch_snappy(a, A.out_size, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(snappypar_sizes_kernel, grid, dim3(256), 0, s, chunks, n, A, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // 3. the layout: a device scan (it waits for the stream)
    uint64_t total = 0, n_over = 0;
    if (chip_layout_units(n, A.out_size, A.out_off, A.out_cap, &total, &n_over, s) != CHIP_OK) return hipErrorUnknown;
    if ((e = sl.fetch(s)) != hipSuccess) return e;
    if (sl.h_sum->n_bad || n_over) return hipSuccess;
    const uint32_t n_stored = sl.h_sum->n_stored;
    serial = false;
    c.sum->path = CHIP_SNAPPYPAR_PARALLEL;
    c.sum->total_out = total;
    if (total > c.out_cap) {
        c.sum->status = CHIP_NEED_OUTPUT;
        return hipSuccess;
    }
    // 4. the blocks straight into out_base, 5. the uncompressed chunks by the file writer's copy (units of length 0 are stepped over)
    a.out_base = c.out;
    a.out_off = A.out_off;
    a.out_cap = A.out_cap;
    a.out_len = A.out_len;
    if ((e = launch_snappy(a, nullptr, s)) != hipSuccess) return e;
    if (n_stored && total) enqueue_copy(n, c.in, A.in_off, A.src_len, c.out, A.out_off, total, s);
    // 6. CRC-32C of every chunk's content where it now lies, compared with the stored value by one thread per chunk
    if (total) {
        if (chip_crc32c_batch(n, c.out, A.out_off, A.out_cap, A.crc, s) != CHIP_OK) return hipErrorUnknown;
    } else {
        if ((e = hipMemsetAsync(A.crc, 0, (size_t)n * 4, s)) != hipSuccess) return e;  // the CRC-32C of no bytes; out_base may be NULL
    }
    hipLaunchKernelGGL(snappypar_verify_kernel, grid, dim3(256), 0, s, chunks, n, A, d);
    if ((e = sl.fetch(s)) != hipSuccess) return e;
    if (sl.h_sum->n_bad) {
        serial = true;
        return hipSuccess;
    }
    c.sum->status = CHIP_FINISHED;
    c.sum->out_len = total;
    c.sum->in_used = c.len;
    return hipSuccess;
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_snappy_chunks_host(const uint8_t *in, uint64_t len, uint64_t max_chunks, chip_snappy_chunk *chunks, chip_snappy_chunks_summary *summary)
{
    if (!summary || (len && !in) || (max_chunks && !chunks)) return CHIP_E_INVALID;
    snappy::MemReader rd{in, len};
    *summary = snappy::walk_chunks(rd, len, max_chunks, chunks);
    return CHIP_OK;
}

int chip_snappy_chunks(const void *in_base, uint64_t len, uint64_t max_chunks, chip_snappy_chunk *chunks, chip_snappy_chunks_summary *summary,
                       void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (max_chunks && !chunks) || ((uintptr_t)in_base & 3u) || len > ((uint64_t)1 << 40)) return CHIP_E_INVALID;
    *summary = NO_STREAM;
    if (len < 4) return CHIP_OK;  // (what the walk says of it)
    return with_slot(
        g_snappychunks_cache, stream,
        [&](SnappyChunksSlot &sl, hipStream_t s) {
            hipError_t e = sl.summary();
            if (e != hipSuccess) return e;
            if ((e = hop((const uint8_t *)in_base, len, max_chunks, chunks, sl.d_sum, s)) != hipSuccess) return e;
            if ((e = sl.fetch(s)) != hipSuccess) return e;
            *summary = *sl.h_sum;
            return hipSuccess;
        },
        [&] { *summary = NO_STREAM; });
}

int chip_snappy_parallel(const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, uint32_t flags, chip_snappy_parallel_summary *summary,
                         void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (!summary || (len && !in_base) || (out_cap && !out_base) || ((uintptr_t)in_base & 3u) || flags || len > ((uint64_t)1 << 40))
        return CHIP_E_INVALID;
    const auto blank = [&] { *summary = chip_snappy_parallel_summary{0, 0, 0, 0, CHIP_NEED_INPUT, CHIP_SNAPPYPAR_SERIAL, 0, 0}; };
    blank();
    const SnappyParCall c{(const uint8_t *)in_base, len, (uint8_t *)out_base, out_cap, summary};
    return with_slot(
        g_snappypar_cache, stream,
        [&](SnappyParSlot &sl, hipStream_t s) {
            bool serial = true;
            hipError_t e = snappypar_parallel(sl, c, s, serial);
            if (e == hipSuccess && serial) e = snappypar_serial(sl, c, s);
            return e;
        },
        blank);
}

}  // extern "C"
