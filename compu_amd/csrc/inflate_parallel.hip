// ONE large deflate stream decoded by the whole GPU: chip_inflate_parallel.
//
// The stream is cut into chunks of chunk_bytes and every chunk in which the finder (inflate_find.hip) names a block start gets a wave
// of its own, before anybody knows whether the start is real or what stands in the 32 KiB in front of it.  In stream order:
//   wrapper   par_wrapper_kernel: the zlib / gzip header, for the bit of the first block (the finder looks only behind it)
//   find      chip_inflate_find_starts
//   sizes     inflate_spec_kernel: inflate_unit.h's size pass compiled with CHIP_INFLATE_SPEC, one unit per start plus unit 0 from the
//             stream's beginning.  A unit ends where it arrives at a later start (LINKED), at the final block, at an error.
//             -- the host follows the links from unit 0: the CHAIN.  Its members are real boundaries by induction; every other start
//             was a false one and cost its wave.  A 64-bit sum of the chain's lengths places every chunk (pt_out). --
//   markers   inflate_markers_kernel (inflate_parallel_markers.hip): every chain chunk decoded into 16-bit elements at 2 * pt_out[k]
//   windows   par_windows_kernel: ONE workgroup walks the chain and turns the markers of each chunk's last 32 KiB into bytes, window by
//             window; order comes from its own barriers
//   resolve   par_resolve_kernel: out[i] = element < 256 ? element : window of its chunk [marker]
//   checks    par_checks_kernel: CRC-32 / Adler-32 of every chunk with seed 0 / 1, one wave each
//             -- the host combines them along the chain (x^n mod P; Adler's closed form), compares the trailer and fills pt_check --
// No wave waits for another outside the one workgroup of the windows.  Whatever is not a clean stream of at least two chain chunks
// -- an error, a truncation, a wrong check value, a wave that gave up, no start at all -- is answered by the serial decode of the
// unit (chip_inflate_index_build), so that the answer is chip_decode_batch's.
// chip_inflate_parallel_next (sec. 4.18, below) runs the same passes over a SLAB of a stream of any length, from a cursor the caller
// carries: unit 0 begins at the cursor, the windows start from the carried one, and what did not end at a start is the next call's.
#define CHIP_INFLATE_SPEC 1
#include "inflate_unit.h"

#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "check_combine.h"
#include "launch_slots.h"
#include "plan_common.h"

namespace chip {

// the size pass over the starts: a persistent grid as inflate_sizes_kernel
__global__ __launch_bounds__(64, CHIP_WAVES_PER_SIMD) void inflate_spec_kernel(BatchArgs a, SpecRec sp, uint64_t *out_size, uint32_t *scratch, uint32_t *next_unit)
{
    __shared__ WaveLds L;
    uint32_t *grow = scratch + (size_t)blockIdx.x * SCRATCH_WORDS;
    for (;;) {
        uint32_t i = 0;
        if (lane_id() == 0) i = atomicAdd(next_unit, 1u);
        i = rdfirst(i);
        if (i >= a.n) break;
        inflate_unit<true>(a, i, L, grow, out_size, sp);
        WSYNC();  // the next unit reuses the LDS
    }
}

namespace {

static_assert(SPEC_PASS_MAX == CHIP_PAR_PASS_MAX, "the header names the number of starts a wave walks over");
constexpr uint32_t WINDOW = 32768;
constexpr uint32_t DEFAULT_CHUNK = 128u << 10;
constexpr uint32_t MAX_WAVES = 2048;  // waves of the two unit kernels (64 KiB of token rows each)
constexpr uint64_t CHUNK_OUT_MAX = 0xFFFFFFF0ull - WINDOW;  // chip_inflate_index_read's limit for a chunk

// what the kernels answer in the slot's summary
struct DevPar {
    int32_t w_status;  // the wrapper: ST_RUNNING, or the status that ends the unit
    uint32_t w_wrap, w_hdr, pad;
    // the one unit of the serial size pass
    uint64_t in_off, out_size;
    uint32_t in_len, in_used;
    int32_t status;
    uint32_t pad2;
};

__global__ __launch_bounds__(64) void par_wrapper_kernel(const uint8_t *in, uint32_t len, int32_t format, DevPar *d)
{
    __shared__ uint32_t tab[2048];
    uint32_t wrap = 0, hdr = 0;
    int32_t st = ST_RUNNING;
    if (format != CHIP_FMT_DEFLATE) st = parse_wrapper((LDS_AS uint32_t *)tab, in, len, format, wrap, hdr);
    if (lane_id() == 0) {
        d->w_status = (int32_t)rdfirst((uint32_t)st);
        d->w_wrap = rdfirst(wrap);
        d->w_hdr = rdfirst(hdr);
    }
}

// unit u of the size pass: from the byte that holds its start to the end of the stream
// (unit 0 from byte0: 0, or the byte a carried cursor stands in)
__global__ __launch_bounds__(256) void par_spec_units_kernel(const uint64_t *starts, uint32_t n_units, uint32_t len, uint32_t byte0, uint64_t *in_off,
                                                             uint32_t *in_len)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= n_units) return;
    const uint64_t byte = u ? starts[u - 1u] >> 3 : byte0;
    in_off[u] = byte < len ? byte : len;
    in_len[u] = byte < len ? len - (uint32_t)byte : 0u;
}

// window slot k: the caller's while it has room for it, else the scratch's
struct Windows {
    uint8_t *user, *scratch;
    uint64_t n_user;
    __device__ __forceinline__ uint8_t *slot(uint64_t k) const { return (k < n_user ? user : scratch) + (uint64_t)WINDOW * k; }
};

// element e of chunk k (pt_out[k] = o, window w of wl content bytes) as a byte; a marker outside the window's content (a reach the
// size pass would have refused) reads 0
__device__ __forceinline__ uint8_t resolved(uint32_t e, const uint8_t *w, uint32_t wl)
{
    if (e < 256u) return (uint8_t)e;
    const uint32_t j = (e & 0x7fffu) - (WINDOW - wl);
    return j < wl ? w[j] : (uint8_t)0;
}

// W_(k+1)[i] = content[pt_out[k + 1] - wl + i]: an element of chunk k resolved through W_k, or, in front of a chunk shorter than 32 KiB,
// a byte of W_k itself.  One workgroup, chunk after chunk; the window it reads and the one it writes stay in LDS (the slots in
// memory are for the resolve pass and the caller), so that a step is one round of element loads, LDS look-ups and a barrier.
// hist > 0 (chip_inflate_parallel_next): the content goes on from an earlier call, whose last hist bytes are carry[0 .. hist).  They
// are W_0, and every pt_out counts from the first of them on (element q of the call stands at img[q - hist]).
__global__ __launch_bounds__(1024) void par_windows_kernel(const uint16_t *__restrict__ img, const uint64_t *__restrict__ pt_out, uint32_t n, Windows W,
                                                           const uint8_t *__restrict__ carry, uint32_t hist)
{
    __shared__ uint8_t win[2][WINDOW];
    constexpr uint32_t PER = WINDOW / 1024u, COPY = 0x10000u;  // COPY | j: byte j of W_k as it stands
    // the elements of step k (they do not depend on any window: step k + 1's are loaded while step k works)
    auto load = [&](uint32_t k, uint32_t(&e)[PER]) {
        const uint64_t o0 = pt_out[k] + hist, o1 = pt_out[k + 1u] + hist;
        const uint32_t wl0 = o0 < WINDOW ? (uint32_t)o0 : WINDOW, wl1 = o1 < WINDOW ? (uint32_t)o1 : WINDOW;
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {  // every load of the step goes out before the first one is waited for
            const uint32_t i = threadIdx.x + 1024u * j;
            const uint64_t q = o1 - wl1 + i;
            e[j] = 0;
            if (i < wl1) e[j] = q >= o0 ? (uint32_t)img[q - hist] : COPY | (uint32_t)(q - (o0 - wl0));
        }
    };
    uint32_t e[PER] = {}, en[PER] = {};
    if (n >= 2) load(0, e);
    if (hist) {  // (uniform) W_0, in LDS and in its slot
        uint8_t *g0 = W.slot(0);
        for (uint32_t i = threadIdx.x; i < hist; i += 1024u) {
            const uint8_t v = carry[i];
            win[0][i] = v;
            g0[i] = v;
        }
        __syncthreads();
    }
    for (uint32_t k = 0; k + 1u < n; k++) {
        const uint64_t o0 = pt_out[k] + hist, o1 = pt_out[k + 1u] + hist;
        const uint32_t wl0 = o0 < WINDOW ? (uint32_t)o0 : WINDOW, wl1 = o1 < WINDOW ? (uint32_t)o1 : WINDOW;
        const uint8_t *w0 = win[k & 1u];
        uint8_t *w1 = win[(k + 1u) & 1u], *g1 = W.slot(k + 1u);
        if (k + 2u < n) load(k + 1u, en);
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {
            const uint32_t i = threadIdx.x + 1024u * j;
            if (i < wl1) {
                const uint8_t v = e[j] & COPY ? w0[e[j] & 0x7fffu] : resolved(e[j], w0, wl0);
                w1[i] = v;
                g1[i] = v;
            }
        }
        // W_(k+1) is whole in LDS before W_(k+2) reads it, and W_k is read no more before it is written again.  An LDS barrier only:
        // the slots in memory are read by later kernels, and waiting for their stores here would put a memory round trip into every step.
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) e[j] = en[j];
    }
}

// blockIdx.x = chunk, blockIdx.y = its share of the chunk's elements.  hist: content in front of out[0] that W_0 holds (above).
// first_bad (or nullptr): the least q whose element is a marker for a byte in front of the content -- a distance too far back that
// no size pass has vouched against (the one-wave path of chip_inflate_parallel_next); the caller sets it to ~0 before.
__global__ __launch_bounds__(256) void par_resolve_kernel(const uint16_t *img, const uint64_t *pt_out, uint32_t n, uint64_t total, Windows W, uint8_t *out,
                                                          uint32_t hist, unsigned long long *first_bad)
{
    const uint32_t k = blockIdx.x;
    const uint64_t o0 = pt_out[k], o1 = k + 1u < n ? pt_out[k + 1u] : total;
    const uint32_t wl0 = o0 + hist < WINDOW ? (uint32_t)o0 + hist : WINDOW;
    const uint8_t *w0 = W.slot(k);
    for (uint64_t q = o0 + blockIdx.y * 256u + threadIdx.x; q < o1; q += 256u * gridDim.y) {
        const uint32_t e = img[q];
        out[q] = resolved(e, w0, wl0);
        if (first_bad && e >= 256u && (e & 0x7fffu) < WINDOW - wl0) atomicMin(first_bad, (unsigned long long)q);
    }
}

// The window a later call starts from: the last min(hist + n, 32 768) bytes of (the hist bytes of `window`, then out[0 .. n)), written
// over `window`.  One workgroup: every thread holds its bytes before the first one is stored.
__global__ __launch_bounds__(1024) void par_carry_kernel(uint8_t *window, uint32_t hist, const uint8_t *out, uint64_t n)
{
    constexpr uint32_t PER = WINDOW / 1024u;
    const uint64_t all = hist + n;
    const uint32_t keep = all < WINDOW ? (uint32_t)all : WINDOW;
    const uint64_t first = all - keep;  // of the joined bytes
    uint8_t v[PER];
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint32_t i = threadIdx.x + 1024u * j;
        const uint64_t q = first + i;
        v[j] = 0;
        if (i < keep) v[j] = q < hist ? window[q] : out[q - hist];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint32_t i = threadIdx.x + 1024u * j;
        if (i < keep) window[i] = v[j];
    }
}

// chk[k] = the check of chunk k's bytes alone
__global__ __launch_bounds__(64) void par_checks_kernel(const uint8_t *out, const uint64_t *pt_out, uint32_t n, uint64_t total, uint32_t wrap, uint32_t *chk)
{
    __shared__ uint32_t tab[2048];
    const uint32_t k = blockIdx.x;
    const uint64_t o0 = pt_out[k], o1 = k + 1u < n ? pt_out[k + 1u] : total;
    const uint32_t len = (uint32_t)(o1 - o0);
    const uint32_t v = wrap == 1 ? wave_adler32(out + o0, len, 1u) : wave_crc32((LDS_AS uint32_t *)tab, out + o0, len, 0u);
    if (lane_id() == 0) chk[k] = rdfirst(v);
}

// CHIP_PAR_TIMING in the environment: the device time between the phases of every call, on stderr (events on the call's stream;
// a phase's figure holds the host's wait or work that stands between its two events)
struct PhaseClock {
    hipStream_t stream;
    const char *what = "inflate_parallel";
    bool on = getenv("CHIP_PAR_TIMING") != nullptr;
    std::vector<std::pair<const char *, hipEvent_t>> ev;
    void mark(const char *name)
    {
        hipEvent_t e;
        if (!on || hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, stream);
        ev.push_back({name, e});
    }
    ~PhaseClock()
    {
        for (size_t i = 1; i < ev.size(); i++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[i - 1].second, ev[i].second) == hipSuccess) fprintf(stderr, "[chip] %s %-8s %9.3f ms\n", what, ev[i].first, ms);
        }
        for (auto &e : ev) (void)hipEventDestroy(e.second);
    }
};

using ParSlot = SummarySlot<DevPar>;
SlotCache<ParSlot> g_par_cache;

struct ParCall {
    int format;
    const uint8_t *in;
    uint32_t len;
    uint8_t *out;
    uint64_t out_cap;
    uint32_t chunk_bytes;
    uint64_t max_points;
    uint64_t *pt_bit, *pt_out;
    uint32_t *pt_check;
    uint8_t *windows;
    chip_inflate_parallel_summary *summary;
};

// The serial path: the index build with a spacing no stream reaches, which is chip_decode_batch's answer, the first block as the
// one point, wrap, check and end_bit.  Room short: the one-unit size pass says how much to come back with.
hipError_t serial_locked(ParSlot &sl, const ParCall &c, hipStream_t stream)
{
    chip_inflate_parallel_summary &s = *c.summary;
    chip_inflate_index_summary is{0, 0, 0, 0, CHIP_NEED_OUTPUT, 0, 0, 0};
    if (c.out) {
        const int rc = chip_inflate_index_build(c.format, c.in, c.len, c.out, c.out_cap, 0xFFFFFFFFu, c.max_points, c.pt_bit, c.pt_out, c.pt_check,
                                                c.windows, &is, stream);
        if (rc != CHIP_OK) return rc == CHIP_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;
    }
    s.n_points = is.n_points, s.out_len = is.out_len, s.in_used = is.in_used, s.end_bit = is.end_bit;
    s.total_out = is.status == CHIP_FINISHED ? is.out_len : 0;
    s.status = is.status, s.wrap = is.wrap, s.check = is.check, s.path = CHIP_PAR_SERIAL;
    if (is.status != CHIP_NEED_OUTPUT) return hipSuccess;
    DevPar *d = sl.d_sum;
    *sl.h_sum = DevPar{0, 0, 0, 0, 0, 0, c.len, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(d, sl.h_sum, sizeof(DevPar), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    BatchArgs a{};
    a.in_base = c.in, a.in_off = &d->in_off, a.in_len = &d->in_len, a.in_used = &d->in_used, a.status = &d->status;
    a.n = 1, a.format = c.format;
    if ((e = launch_inflate(a, &d->out_size, stream)) != hipSuccess) return e;
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    const DevPar &h = *sl.h_sum;
    if (h.status == CHIP_FINISHED && h.out_size > c.out_cap) {
        s.out_len = 0, s.in_used = 0, s.end_bit = 0, s.check = 0;
        s.total_out = h.out_size;
        s.status = CHIP_NEED_OUTPUT;
    } else if (!c.out) {  // no room and no buffer, and no size to name: the size pass's verdict on the unit
        s.status = h.status;
        s.in_used = h.in_used;
        s.total_out = h.status == CHIP_FINISHED ? h.out_size : 0;
    }
    return hipSuccess;
}

// The parallel path.  serial = true on return: the stream is not one for it (or not clean) and nothing the caller sees was decided.
hipError_t parallel_locked(ParSlot &sl, const ParCall &c, hipStream_t stream, bool &serial)
{
    serial = true;
    chip_inflate_parallel_summary &s = *c.summary;
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    DevPar *d = sl.d_sum;
    if (c.len == 0) return hipSuccess;
    PhaseClock clock{stream};
    clock.mark("start");
    hipLaunchKernelGGL(par_wrapper_kernel, dim3(1), dim3(64), 0, stream, c.in, c.len, (int32_t)c.format, d);
    if ((e = sl.fetch(stream)) != hipSuccess) return e;
    if (sl.h_sum->w_status != ST_RUNNING) return hipSuccess;
    clock.mark("wrapper");
    const uint32_t wrap = sl.h_sum->w_wrap;
    const uint64_t first_bit = 8ull * sl.h_sum->w_hdr;
    const uint32_t B = c.chunk_bytes ? c.chunk_bytes : DEFAULT_CHUNK;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)c.len + B - 1) / B);
    if (n_chunks < 2 || first_bit >= 8ull * c.len) return hipSuccess;

    // the per-chunk words (buffer 0): no list is longer than the chunks are many
    const size_t N = n_chunks;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up16(bytes); return o; };
    const size_t o_counter = take(16), o_starts = take(N * 8), o_in_off = take(N * 8), o_in_len = take(N * 4), o_in_used = take(N * 4),
                 o_status = take(N * 4), o_size = take(N * 8), o_spec = take(N * sizeof(SpecOut)), o_bit0 = take(N * 4), o_out_off = take(N * 8),
                 o_out_cap = take(N * 4), o_out_len = take(N * 4), o_pt_out = take(N * 8), o_chk = take(N * 4);
    if ((e = sl.grow(0, at)) != hipSuccess) return e;
    uint8_t *w = sl.buf[0];
    uint32_t *counter = (uint32_t *)(w + o_counter);
    uint64_t *starts = (uint64_t *)(w + o_starts), *in_off = (uint64_t *)(w + o_in_off), *out_size = (uint64_t *)(w + o_size);
    uint32_t *in_len = (uint32_t *)(w + o_in_len), *in_used = (uint32_t *)(w + o_in_used);
    int32_t *status = (int32_t *)(w + o_status);
    SpecOut *spec = (SpecOut *)(w + o_spec);

    uint64_t n_starts = 0;
    const int rc = chip_inflate_find_starts(c.in, c.len, first_bit, B, n_chunks - 1, starts, &n_starts, stream);
    if (rc != CHIP_OK) return rc == CHIP_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;
    s.n_starts = n_starts;
    clock.mark("find");
    if (n_starts == 0 || n_starts > n_chunks - 1) return hipSuccess;

    // ---- the speculative size pass
    const uint32_t U = (uint32_t)n_starts + 1u;
    const size_t rows_bytes = (size_t)(U < MAX_WAVES ? U : MAX_WAVES) * SCRATCH_WORDS * 4;
    if ((e = sl.grow(1, rows_bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL(par_spec_units_kernel, dim3((U + 255u) / 256u), dim3(256), 0, stream, (const uint64_t *)starts, U, c.len, 0u, in_off, in_len);
    if ((e = hipMemsetAsync(counter, 0, 4, stream)) != hipSuccess) return e;
    {
        BatchArgs a{};
        a.in_base = c.in, a.in_off = in_off, a.in_len = in_len, a.in_used = in_used, a.status = status;
        a.n = U, a.format = c.format;
        const SpecRec sp{starts, (uint32_t)n_starts, spec};
        hipLaunchKernelGGL(inflate_spec_kernel, dim3(U < MAX_WAVES ? U : MAX_WAVES), dim3(64), 0, stream, a, sp, out_size, (uint32_t *)sl.buf[1], counter);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    std::vector<SpecOut> so(U);
    if ((e = hipMemcpyAsync(so.data(), spec, (size_t)U * sizeof(SpecOut), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    clock.mark("sizes");

    // ---- the chain
    std::vector<uint32_t> chain;  // the units on it
    std::vector<uint64_t> pt_out, size;
    bool clean = true;
    uint64_t total = 0;
    for (uint32_t u = 0;;) {
        const SpecOut &o = so[u];
        chain.push_back(u);
        pt_out.push_back(total);
        size.push_back(o.size);
        if (o.reach > total || o.size > CHUNK_OUT_MAX) clean = false;  // a match in front of stream byte 0; a chunk beyond a unit's room
        total += o.size;
        if (o.kind != SPEC_LINKED) {
            if (o.kind != SPEC_RAN || o.status != CHIP_FINISHED) clean = false;
            break;
        }
        if (o.link <= u || o.link >= U) return hipErrorUnknown;  // (the input changed under the kernels)
        u = o.link;
    }
    if (!clean || chain.size() < 2 || total > 0xFFFFFFF0ull) return hipSuccess;
    const uint32_t C = (uint32_t)chain.size();
    // chunk k begins where the chunk in front of it linked; chunk 0 at the first block
    std::vector<uint64_t> pt_bit(C);
    pt_bit[0] = so[0].first_bit;
    for (uint32_t k = 1; k < C; k++) pt_bit[k] = so[chain[k - 1u]].end_bit;
    const uint64_t end_bit = so[chain[C - 1u]].end_bit;
    for (uint32_t k = 0; k + 1u < C; k++)
        if (pt_bit[k + 1u] <= pt_bit[k]) return hipErrorUnknown;
    if (end_bit > 8ull * c.len) return hipErrorUnknown;

    // ---- the trailer's bytes
    const uint32_t tk = (uint32_t)((end_bit + 7) >> 3), need = wrap == 2 ? 8u : wrap == 1 ? 4u : 0u;
    uint8_t trailer[8] = {0};
    if (c.len - tk < need) return hipSuccess;
    if (need && (e = hipMemcpyAsync(trailer, c.in + tk, need, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if (need && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if (wrap == 2 && (trailer[4] | ((uint32_t)trailer[5] << 8) | ((uint32_t)trailer[6] << 16) | ((uint32_t)trailer[7] << 24)) != (uint32_t)total)
        return hipSuccess;

    const uint64_t n_false = n_starts - (C - 1u);
    if (total > c.out_cap) {  // room short: the size to come back with (chip_pack_units' convention)
        s = chip_inflate_parallel_summary{C, 0, 0, 0, total, n_starts, n_false, CHIP_NEED_OUTPUT, wrap, 0, CHIP_PAR_PARALLEL};
        serial = false;
        return hipSuccess;
    }

    // ---- the marker decode: chunk k's input ends with the byte that holds the next chunk's first bit
    const uint32_t q = (uint32_t)(C < c.max_points ? C : c.max_points);
    const size_t img_off = up16(rows_bytes), win_off = img_off + up16(2 * (size_t)total);
    if ((e = sl.grow(1, win_off + (q < C ? (size_t)WINDOW * C : 0) + 16)) != hipSuccess) return e;
    uint16_t *img = (uint16_t *)(sl.buf[1] + img_off);
    const Windows W{c.windows, sl.buf[1] + win_off, q};
    std::vector<uint64_t> m_in_off(C), m_out_off(C);
    std::vector<uint32_t> m_in_len(C), m_bit0(C), m_out_cap(C);
    for (uint32_t k = 0; k < C; k++) {
        m_in_off[k] = pt_bit[k] >> 3;
        m_in_len[k] = (uint32_t)((k + 1u < C ? (pt_bit[k + 1u] + 7) >> 3 : (uint64_t)c.len) - m_in_off[k]);
        m_bit0[k] = (uint32_t)(pt_bit[k] & 7u);
        m_out_off[k] = 2 * pt_out[k];
        m_out_cap[k] = (uint32_t)size[k];
    }
    uint32_t *bit0 = (uint32_t *)(w + o_bit0), *out_cap = (uint32_t *)(w + o_out_cap), *out_len = (uint32_t *)(w + o_out_len), *chk = (uint32_t *)(w + o_chk);
    uint64_t *out_off = (uint64_t *)(w + o_out_off), *d_pt_out = (uint64_t *)(w + o_pt_out);
    auto up = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };
    if ((e = up(in_off, m_in_off.data(), (size_t)C * 8)) != hipSuccess || (e = up(in_len, m_in_len.data(), (size_t)C * 4)) != hipSuccess ||
        (e = up(bit0, m_bit0.data(), (size_t)C * 4)) != hipSuccess || (e = up(out_off, m_out_off.data(), (size_t)C * 8)) != hipSuccess ||
        (e = up(out_cap, m_out_cap.data(), (size_t)C * 4)) != hipSuccess || (e = up(d_pt_out, pt_out.data(), (size_t)C * 8)) != hipSuccess ||
        (e = up(c.pt_bit, pt_bit.data(), (size_t)q * 8)) != hipSuccess || (e = up(c.pt_out, pt_out.data(), (size_t)q * 8)) != hipSuccess)
        return e;
    if ((e = hipMemsetAsync(counter, 0, 4, stream)) != hipSuccess) return e;
    clock.mark("chain");
    {
        BatchArgs a{};
        a.in_base = c.in, a.in_off = in_off, a.in_len = in_len;
        a.out_base = (uint8_t *)img, a.out_off = out_off, a.out_cap = out_cap;
        a.out_len = out_len, a.in_used = in_used, a.status = status;
        a.n = C, a.format = CHIP_FMT_DEFLATE;
        if ((e = enqueue_inflate_markers(a, bit0, (uint32_t *)sl.buf[1], counter, C < MAX_WAVES ? C : MAX_WAVES, stream)) != hipSuccess) return e;
    }
    clock.mark("markers");
    hipLaunchKernelGGL(par_windows_kernel, dim3(1), dim3(1024), 0, stream, (const uint16_t *)img, (const uint64_t *)d_pt_out, C, W, (const uint8_t *)nullptr, 0u);
    clock.mark("windows");
    hipLaunchKernelGGL(par_resolve_kernel, dim3(C, 8), dim3(256), 0, stream, (const uint16_t *)img, (const uint64_t *)d_pt_out, C, total, W, c.out, 0u,
                       (unsigned long long *)nullptr);
    clock.mark("resolve");
    if (wrap)
        hipLaunchKernelGGL(par_checks_kernel, dim3(C), dim3(64), 0, stream, (const uint8_t *)c.out, (const uint64_t *)d_pt_out, C, total, wrap, chk);
    clock.mark("checks");
    if ((e = hipGetLastError()) != hipSuccess) return e;
    std::vector<uint32_t> h_len(C), h_chk(C, 0);
    std::vector<int32_t> h_status(C);
    if ((e = hipMemcpyAsync(h_len.data(), out_len, (size_t)C * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h_status.data(), status, (size_t)C * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if (wrap && (e = hipMemcpyAsync(h_chk.data(), chk, (size_t)C * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;

    // ---- what the marker decode has to confirm, the checks along the chain, the trailer
    for (uint32_t k = 0; k < C; k++) {
        const bool ended = k + 1u < C ? (h_status[k] == CHIP_NEED_INPUT || h_status[k] == CHIP_NEED_OUTPUT) : h_status[k] == CHIP_FINISHED;
        if (!ended || h_len[k] != m_out_cap[k]) return hipSuccess;
    }
    std::vector<uint32_t> pt_check(C);
    uint32_t run = wrap == 1 ? 1u : 0u;
    for (uint32_t k = 0; k < C; k++) {
        pt_check[k] = run;
        if (wrap == 1) run = adler32_append(run, h_chk[k], size[k]);
        else if (wrap == 2) run = crc32_append(run, h_chk[k], size[k]);
    }
    const uint32_t want = wrap == 1 ? ((uint32_t)trailer[0] << 24) | ((uint32_t)trailer[1] << 16) | ((uint32_t)trailer[2] << 8) | trailer[3]
                                    : trailer[0] | ((uint32_t)trailer[1] << 8) | ((uint32_t)trailer[2] << 16) | ((uint32_t)trailer[3] << 24);
    if (wrap && want != run) return hipSuccess;  // the serial decode answers a wrong check value
    if ((e = up(c.pt_check, pt_check.data(), (size_t)q * 4)) != hipSuccess) return e;
    clock.mark("combine");
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    s = chip_inflate_parallel_summary{C, total, (uint64_t)tk + need, end_bit, total, n_starts, n_false, CHIP_FINISHED, wrap, run, CHIP_PAR_PARALLEL};
    serial = false;
    return hipSuccess;
}


// ---- chip_inflate_parallel_next: the same passes over a SLAB of a stream, from a carried cursor ---------------

// One step through the blocks of the slab, from the block boundary at bit `fb` of it.
struct BlocksOut {
    uint64_t end_bit = 0;  // the boundary reached (behind the final block when finished)
    uint64_t out_len = 0, need_out = 0, n_chunks = 0, n_starts = 0, n_false = 0;
    bool finished = false;  // the final block was delivered
    int32_t status = CHIP_NEED_INPUT;  // NEED_INPUT / NEED_OUTPUT: why the blocks stopped; an error: sticky
    uint32_t path = CHIP_PAR_SERIAL;
};

struct NextCall {
    const uint8_t *in;
    uint32_t len;
    uint8_t *out;
    uint64_t out_cap;
    uint32_t chunk_bytes;
    uint8_t *window;
    chip_inflate_cursor *cur;
};

hipError_t blocks_locked(ParSlot &sl, const NextCall &c, uint64_t fb, hipStream_t stream, PhaseClock &clock, BlocksOut &r)
{
    chip_inflate_cursor &cur = *c.cur;
    const uint32_t hist = cur.hist;
    hipError_t e = hipSuccess;
    if (fb + 3 > 8ull * c.len) return hipSuccess;  // not even a block's first three bits
    const uint32_t B = c.chunk_bytes ? c.chunk_bytes : DEFAULT_CHUNK;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)c.len + B - 1) / B);
    r.n_chunks = n_chunks;

    const size_t N = n_chunks;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up16(bytes); return o; };
    const size_t o_counter = take(16), o_bad = take(16), o_starts = take(N * 8), o_in_off = take(N * 8), o_in_len = take(N * 4), o_in_used = take(N * 4),
                 o_status = take(N * 4), o_size = take(N * 8), o_spec = take(N * sizeof(SpecOut)), o_bit0 = take(N * 4), o_out_off = take(N * 8),
                 o_out_cap = take(N * 4), o_out_len = take(N * 4), o_pt_out = take((N + 1) * 8), o_chk = take(N * 4), o_resume = take(RESUME_WORDS * 4);
    if ((e = sl.grow(0, at)) != hipSuccess) return e;
    uint8_t *w = sl.buf[0];
    uint32_t *counter = (uint32_t *)(w + o_counter);
    unsigned long long *first_bad = (unsigned long long *)(w + o_bad);
    uint64_t *starts = (uint64_t *)(w + o_starts), *in_off = (uint64_t *)(w + o_in_off), *out_size = (uint64_t *)(w + o_size);
    uint32_t *in_len = (uint32_t *)(w + o_in_len), *in_used = (uint32_t *)(w + o_in_used);
    int32_t *status = (int32_t *)(w + o_status);
    SpecOut *spec = (SpecOut *)(w + o_spec);
    uint32_t *bit0 = (uint32_t *)(w + o_bit0), *out_cap = (uint32_t *)(w + o_out_cap), *out_len = (uint32_t *)(w + o_out_len), *chk = (uint32_t *)(w + o_chk);
    uint64_t *out_off = (uint64_t *)(w + o_out_off), *d_pt_out = (uint64_t *)(w + o_pt_out);
    uint32_t *resume = (uint32_t *)(w + o_resume);
    auto up = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };

    uint64_t n_starts = 0;
    if (n_chunks >= 2) {
        const int rc = chip_inflate_find_starts(c.in, c.len, fb, B, n_chunks - 1, starts, &n_starts, stream);
        if (rc != CHIP_OK) return rc == CHIP_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;
        if (n_starts > n_chunks - 1) return hipErrorUnknown;
    }
    r.n_starts = n_starts;
    clock.mark("find");

    // ---- the speculative size pass; unit 0 begins at the cursor
    const uint32_t U = (uint32_t)n_starts + 1u;
    const size_t rows_bytes = (size_t)(U < MAX_WAVES ? U : MAX_WAVES) * SCRATCH_WORDS * 4;
    if ((e = sl.grow(1, rows_bytes)) != hipSuccess) return e;
    hipLaunchKernelGGL(par_spec_units_kernel, dim3((U + 255u) / 256u), dim3(256), 0, stream, (const uint64_t *)starts, U, c.len, (uint32_t)(fb >> 3), in_off,
                       in_len);
    if ((e = hipMemsetAsync(counter, 0, 4, stream)) != hipSuccess) return e;
    {
        BatchArgs a{};
        a.in_base = c.in, a.in_off = in_off, a.in_len = in_len, a.in_used = in_used, a.status = status;
        a.n = U, a.format = CHIP_FMT_DEFLATE;
        const SpecRec sp{starts, (uint32_t)n_starts, spec, (uint32_t)(fb & 7u)};
        hipLaunchKernelGGL(inflate_spec_kernel, dim3(U < MAX_WAVES ? U : MAX_WAVES), dim3(64), 0, stream, a, sp, out_size, (uint32_t *)sl.buf[1], counter);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    std::vector<SpecOut> so(U);
    if ((e = hipMemcpyAsync(so.data(), spec, (size_t)U * sizeof(SpecOut), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    clock.mark("sizes");

    // ---- the chain: its members that ended LINKED, or in the final block, and are clean; what follows is the next call's
    std::vector<uint64_t> pt_bit, pt_out, size;  // per kept member; pt_bit has the end of the last one behind them
    bool finished = false;
    uint64_t total = 0, links = 0;  // links: the starts the chain arrived at (the dropped member's too)
    pt_bit.push_back(fb);
    for (uint32_t u = 0;;) {
        const SpecOut &o = so[u];
        const bool fin = o.kind == SPEC_RAN && o.status == CHIP_FINISHED;
        if (o.kind != SPEC_LINKED && !fin) break;
        if (o.reach > total + hist || o.size > CHUNK_OUT_MAX) break;  // a match in front of stream byte 0: the one-wave path names it
        if (o.end_bit <= pt_bit.back() && !fin) return hipErrorUnknown;
        if (o.end_bit > 8ull * c.len || o.end_bit < pt_bit.back()) return hipErrorUnknown;
        pt_out.push_back(total);
        size.push_back(o.size);
        pt_bit.push_back(o.end_bit);
        total += o.size;
        if (fin) {
            finished = true;
            break;
        }
        if (o.link <= u || o.link >= U) return hipErrorUnknown;  // (the input changed under the kernels)
        u = o.link;
        links++;
    }
    const uint32_t K = (uint32_t)size.size();

    if (K >= 1 && so[0].kind == SPEC_LINKED) {
        // ---- the parallel path: the members that fit the room
        uint32_t D = 0;
        uint64_t give = 0;
        while (D < K && give + size[D] <= c.out_cap) give += size[D++];
        r.path = CHIP_PAR_PARALLEL;
        r.n_false = n_starts - links;
        if (D < K) r.status = CHIP_NEED_OUTPUT, r.need_out = size[D];
        if (D == 0) {
            r.end_bit = fb;
            return hipSuccess;
        }
        const size_t img_off = up16(rows_bytes), win_off = img_off + up16(2 * (size_t)give + 64);
        if ((e = sl.grow(1, win_off + (size_t)WINDOW * D + 16)) != hipSuccess) return e;
        uint16_t *img = (uint16_t *)(sl.buf[1] + img_off);
        const Windows W{nullptr, sl.buf[1] + win_off, 0};
        std::vector<uint64_t> m_in_off(D), m_out_off(D);
        std::vector<uint32_t> m_in_len(D), m_bit0(D), m_out_cap(D);
        for (uint32_t k = 0; k < D; k++) {
            m_in_off[k] = pt_bit[k] >> 3;
            const uint64_t end = k + 1u == K && finished ? (uint64_t)c.len : (pt_bit[k + 1u] + 7) >> 3;
            m_in_len[k] = (uint32_t)(end - m_in_off[k]);
            m_bit0[k] = (uint32_t)(pt_bit[k] & 7u);
            m_out_off[k] = 2 * pt_out[k];
            m_out_cap[k] = (uint32_t)size[k];
        }
        if ((e = up(in_off, m_in_off.data(), (size_t)D * 8)) != hipSuccess || (e = up(in_len, m_in_len.data(), (size_t)D * 4)) != hipSuccess ||
            (e = up(bit0, m_bit0.data(), (size_t)D * 4)) != hipSuccess || (e = up(out_off, m_out_off.data(), (size_t)D * 8)) != hipSuccess ||
            (e = up(out_cap, m_out_cap.data(), (size_t)D * 4)) != hipSuccess || (e = up(d_pt_out, pt_out.data(), (size_t)D * 8)) != hipSuccess)
            return e;
        if ((e = hipMemsetAsync(counter, 0, 4, stream)) != hipSuccess) return e;
        clock.mark("chain");
        {
            BatchArgs a{};
            a.in_base = c.in, a.in_off = in_off, a.in_len = in_len;
            a.out_base = (uint8_t *)img, a.out_off = out_off, a.out_cap = out_cap;
            a.out_len = out_len, a.in_used = in_used, a.status = status;
            a.n = D, a.format = CHIP_FMT_DEFLATE;
            if ((e = enqueue_inflate_markers(a, bit0, (uint32_t *)sl.buf[1], counter, D < MAX_WAVES ? D : MAX_WAVES, stream)) != hipSuccess) return e;
        }
        clock.mark("markers");
        hipLaunchKernelGGL(par_windows_kernel, dim3(1), dim3(1024), 0, stream, (const uint16_t *)img, (const uint64_t *)d_pt_out, D, W, (const uint8_t *)c.window,
                           hist);
        clock.mark("windows");
        hipLaunchKernelGGL(par_resolve_kernel, dim3(D, 8), dim3(256), 0, stream, (const uint16_t *)img, (const uint64_t *)d_pt_out, D, give, W, c.out, hist,
                           (unsigned long long *)nullptr);
        clock.mark("resolve");
        if (cur.wrap)
            hipLaunchKernelGGL(par_checks_kernel, dim3(D), dim3(64), 0, stream, (const uint8_t *)c.out, (const uint64_t *)d_pt_out, D, give, cur.wrap, chk);
        clock.mark("checks");
        if ((e = hipGetLastError()) != hipSuccess) return e;
        std::vector<uint32_t> h_len(D), h_chk(D, 0);
        std::vector<int32_t> h_status(D);
        if ((e = hipMemcpyAsync(h_len.data(), out_len, (size_t)D * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(h_status.data(), status, (size_t)D * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if (cur.wrap && (e = hipMemcpyAsync(h_chk.data(), chk, (size_t)D * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        bool confirmed = true;
        for (uint32_t k = 0; k < D; k++) {
            const bool ended = k + 1u == K && finished ? h_status[k] == CHIP_FINISHED : (h_status[k] == CHIP_NEED_INPUT || h_status[k] == CHIP_NEED_OUTPUT);
            if (!ended || h_len[k] != m_out_cap[k]) confirmed = false;
        }
        if (confirmed) {
            hipLaunchKernelGGL(par_carry_kernel, dim3(1), dim3(1024), 0, stream, c.window, hist, (const uint8_t *)c.out, give);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            append_checks(cur, h_chk.data(), size.data(), D);
            clock.mark("combine");
            r.out_len = give;
            r.end_bit = pt_bit[D];
            r.finished = finished && D == K;
            return hipSuccess;
        }
        // (the marker decode did not confirm the size pass: the one-wave path decides, and the bytes written so far are rewritten)
        r = BlocksOut{};
        r.n_chunks = n_chunks, r.n_starts = n_starts;
    }

    // ---- the one-wave path: unit 0 again, as a marker decode that ends at a boundary -- where it linked, else the last one it
    // reaches in slab and room (the resume record names it)
    const SpecOut &o0 = so[0];
    // an error: what stands in front of the block it is in is true content and is delivered first (the input ends with that
    // boundary's byte); with the cursor at that block the error is the answer
    const bool bad = o0.kind == SPEC_RAN && o0.status < 0;
    if (bad && o0.end_bit <= fb) {
        r.end_bit = fb;
        r.status = o0.status;
        return hipSuccess;
    }
    const uint64_t room = o0.size < c.out_cap ? o0.size : c.out_cap;
    const uint64_t in_end = o0.kind == SPEC_LINKED || bad ? (o0.end_bit + 7) >> 3 : (uint64_t)c.len;
    const size_t img_off = up16(SCRATCH_WORDS * 4);
    if ((e = sl.grow(1, img_off + up16(2 * (size_t)room + 64))) != hipSuccess) return e;
    uint16_t *img = (uint16_t *)(sl.buf[1] + img_off);
    {
        const uint64_t h_in_off = fb >> 3, h_out_off = 0, h_pt_out = 0;
        const uint32_t h_in_len = (uint32_t)(in_end - h_in_off), h_bit0 = (uint32_t)(fb & 7u), h_cap = (uint32_t)room;
        if ((e = up(in_off, &h_in_off, 8)) != hipSuccess || (e = up(in_len, &h_in_len, 4)) != hipSuccess || (e = up(bit0, &h_bit0, 4)) != hipSuccess ||
            (e = up(out_off, &h_out_off, 8)) != hipSuccess || (e = up(out_cap, &h_cap, 4)) != hipSuccess || (e = up(d_pt_out, &h_pt_out, 8)) != hipSuccess)
            return e;
        if ((e = hipMemsetAsync(counter, 0, 4, stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(resume, 0, RESUME_WORDS * 4, stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(first_bad, 0xFF, 8, stream)) != hipSuccess) return e;
        BatchArgs a{};
        a.in_base = c.in, a.in_off = in_off, a.in_len = in_len;
        a.out_base = (uint8_t *)img, a.out_off = out_off, a.out_cap = out_cap;
        a.out_len = out_len, a.in_used = in_used, a.status = status;
        a.n = 1, a.format = CHIP_FMT_DEFLATE, a.resume = resume;
        if ((e = enqueue_inflate_markers(a, bit0, (uint32_t *)sl.buf[1], counter, 1, stream)) != hipSuccess) return e;
    }
    uint32_t h_res[RESUME_WORDS], h_len = 0, h_used = 0;
    int32_t h_status = 0;
    if ((e = hipMemcpyAsync(h_res, resume, sizeof h_res, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&h_len, out_len, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&h_used, in_used, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&h_status, status, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    clock.mark("wave");
    const uint64_t bit_base = 8ull * (fb >> 3);
    uint64_t give = 0;
    if (h_status == CHIP_FINISHED) {
        give = h_len;
        r.finished = true;
        r.end_bit = bit_base + 8ull * h_used;  // (the bits behind the final block up to the byte's end belong to it)
    } else if (h_status == CHIP_NEED_INPUT || h_status == CHIP_NEED_OUTPUT) {
        give = h_res[1];
        r.end_bit = h_res[0] ? bit_base + h_res[0] : fb;
        if (r.end_bit < fb || r.end_bit > 8ull * c.len || give > h_len) return hipErrorUnknown;
        // the room was cut to what the size pass counted: only a caller's room below that is a reason to ask for more
        r.status = c.out_cap < o0.size ? CHIP_NEED_OUTPUT : CHIP_NEED_INPUT;
    } else {
        give = h_len;  // what decoded in front of the error
        r.end_bit = fb;
        r.status = h_status;
    }
    if (give > room) return hipErrorUnknown;
    if (give) {
        const Windows W{c.window, nullptr, 1};  // W_0 is the carried window as it stands
        hipLaunchKernelGGL(par_resolve_kernel, dim3(1, 64), dim3(256), 0, stream, (const uint16_t *)img, (const uint64_t *)d_pt_out, 1u, give, W, c.out, hist,
                           first_bad);
        unsigned long long bad = 0;
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&bad, first_bad, 8, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        if (bad < give) {  // invalid distance too far back, at content byte `bad` of the call
            give = bad;
            r.finished = false;
            r.end_bit = fb;
            r.status = Z_DATA_ERROR;
        }
    }
    if (give) {
        uint32_t h_chk = 0;
        if (cur.wrap) {
            hipLaunchKernelGGL(par_checks_kernel, dim3(1), dim3(64), 0, stream, (const uint8_t *)c.out, (const uint64_t *)d_pt_out, 1u, give, cur.wrap, chk);
            if ((e = hipMemcpyAsync(&h_chk, chk, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(par_carry_kernel, dim3(1), dim3(1024), 0, stream, c.window, hist, (const uint8_t *)c.out, give);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        append_checks(cur, &h_chk, &give, 1);
    }
    r.out_len = give;
    return hipSuccess;
}

hipError_t next_locked(ParSlot &sl, int format, const NextCall &c, chip_inflate_next_summary &s, hipStream_t stream)
{
    chip_inflate_cursor &cur = *c.cur;
    if (cur.phase == CHIP_CUR_DONE) {
        s.status = CHIP_FINISHED;
        return hipSuccess;
    }
    if (cur.phase >= CHIP_CUR_ERROR) {
        s.status = cur.phase == CHIP_CUR_ERROR && cur.error != CHIP_OK ? cur.error : (int32_t)CHIP_E_INVALID;
        return hipSuccess;
    }
    hipError_t e = sl.summary();
    if (e != hipSuccess) return e;
    PhaseClock clock{stream, "inflate_next"};
    clock.mark("start");
    auto fail = [&](int32_t st) {  // sticky
        cur.phase = CHIP_CUR_ERROR;
        cur.error = st;
        s.status = st;
    };
    uint64_t at_bit = cur.bit;  // of the slab: where the cursor stands
    if (cur.phase == CHIP_CUR_HEADER) {
        uint32_t wrap = 0, hdr = 0;
        if (format != CHIP_FMT_DEFLATE) {
            hipLaunchKernelGGL(par_wrapper_kernel, dim3(1), dim3(64), 0, stream, c.in, c.len, (int32_t)format, sl.d_sum);
            if ((e = sl.fetch(stream)) != hipSuccess) return e;
            const int32_t st = sl.h_sum->w_status;
            if (st == CHIP_NEED_INPUT) return hipSuccess;
            if (st != ST_RUNNING) {
                fail(st);
                return hipSuccess;
            }
            wrap = sl.h_sum->w_wrap, hdr = sl.h_sum->w_hdr;
        }
        clock.mark("wrapper");
        cur.wrap = wrap;
        cur.check = wrap == 1 ? 1u : 0u;
        cur.phase = CHIP_CUR_BLOCKS;
        at_bit = 8ull * hdr;
    }
    if (cur.phase == CHIP_CUR_BLOCKS) {
        BlocksOut r;
        r.end_bit = at_bit;
        if ((e = blocks_locked(sl, c, at_bit, stream, clock, r)) != hipSuccess) return e;
        s.out_len = r.out_len, s.need_out = r.need_out, s.n_chunks = r.n_chunks, s.n_starts = r.n_starts, s.n_false = r.n_false, s.path = r.path;
        cursor_delivered(cur, r.out_len);
        at_bit = r.end_bit;
        if (r.status != CHIP_NEED_INPUT && r.status != CHIP_NEED_OUTPUT) fail(r.status);
        else if (r.finished) {
            cur.phase = CHIP_CUR_TRAILER;
            at_bit = (r.end_bit + 7) & ~7ull;
        } else s.status = r.status;
    }
    if (cur.phase == CHIP_CUR_TRAILER) {
        const uint64_t tk = at_bit >> 3;
        const uint32_t need = cur.wrap == 2 ? 8u : cur.wrap == 1 ? 4u : 0u;
        uint8_t t[8] = {0};
        if (c.len - tk < need) {
            s.status = CHIP_NEED_INPUT;
        } else {
            if (need && (e = hipMemcpyAsync(t, c.in + tk, need, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
            if (need && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
            at_bit += 8ull * need;
            if (!trailer_matches(cur, t)) {
                fail(Z_DATA_ERROR);  // incorrect data check / incorrect length check
            } else {
                cur.phase = CHIP_CUR_DONE;
                s.status = CHIP_FINISHED;
            }
        }
    }
    s.in_used = cursor_advance(cur, at_bit);
    return hipStreamSynchronize(stream);
}

}  // namespace

}  // namespace chip

using namespace chip;

extern "C" {

int chip_inflate_parallel(int format, const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, uint32_t chunk_bytes, uint64_t max_points,
                          uint64_t *pt_bit, uint64_t *pt_out, uint32_t *pt_check, void *windows, chip_inflate_parallel_summary *summary,
                          void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (format != CHIP_FMT_DEFLATE && format != CHIP_FMT_ZLIB && format != CHIP_FMT_GZIP && format != CHIP_FMT_AUTO) return CHIP_E_INVALID;
    if (!summary || !in_base || ((uintptr_t)in_base & 3u) || (!out_base && out_cap) || len > CHIP_GZPLAN_WINDOW || out_cap > 0xFFFFFFF0ull)
        return CHIP_E_INVALID;
    if (max_points && (!pt_bit || !pt_out || !pt_check || !windows)) return CHIP_E_INVALID;
    if (chunk_bytes && (chunk_bytes < 256 || chunk_bytes > CHIP_GZPLAN_WINDOW)) return CHIP_E_INVALID;
    const chip_inflate_parallel_summary none{0, 0, 0, 0, 0, 0, 0, CHIP_NEED_INPUT, 0, 0, CHIP_PAR_SERIAL};
    *summary = none;
    const ParCall c{format, (const uint8_t *)in_base, (uint32_t)len, (uint8_t *)out_base, out_cap, chunk_bytes, max_points, pt_bit, pt_out, pt_check,
                    (uint8_t *)windows, summary};
    return with_slot(
        g_par_cache, stream,
        [&](ParSlot &sl, hipStream_t s) {
            bool serial = true;
            hipError_t e = parallel_locked(sl, c, s, serial);
            if (e == hipSuccess && serial) {
                const uint64_t n_starts = summary->n_starts;
                e = serial_locked(sl, c, s);
                summary->n_starts = n_starts;
                summary->n_false = 0;
            }
            return e;
        },
        [&] { *summary = none; });
}

int chip_inflate_parallel_next(int format, chip_inflate_cursor *cur, void *window, const void *in_base, uint64_t len, void *out_base, uint64_t out_cap,
                               uint32_t chunk_bytes, chip_inflate_next_summary *summary, void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (format != CHIP_FMT_DEFLATE && format != CHIP_FMT_ZLIB && format != CHIP_FMT_GZIP && format != CHIP_FMT_AUTO) return CHIP_E_INVALID;
    if (!summary || !cur || !window || (!in_base && len) || (!out_base && out_cap) || len > CHIP_GZPLAN_WINDOW || out_cap > 0xFFFFFFF0ull)
        return CHIP_E_INVALID;
    if (chunk_bytes && (chunk_bytes < 256 || chunk_bytes > CHIP_GZPLAN_WINDOW)) return CHIP_E_INVALID;
    if (cur->bit > 7 || cur->phase > CHIP_CUR_ERROR || cur->wrap > 2 || cur->hist != (cur->out_total < WINDOW ? cur->out_total : WINDOW))
        return CHIP_E_INVALID;
    const chip_inflate_next_summary none{0, 0, 0, 0, 0, 0, CHIP_NEED_INPUT, CHIP_PAR_SERIAL};
    *summary = none;
    const chip_inflate_cursor before = *cur;
    const NextCall c{(const uint8_t *)in_base, (uint32_t)len, (uint8_t *)out_base, out_cap, chunk_bytes, (uint8_t *)window, cur};
    return with_slot(
        g_par_cache, stream, [&](ParSlot &sl, hipStream_t s) { return next_locked(sl, format, c, *summary, s); },
        [&] {
            *summary = none;
            *cur = before;  // (the window may hold a later state: a failed call ends the decode)
        });
}

}  // extern "C"
