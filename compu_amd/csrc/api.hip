// C ABI of libcompu_hip.so (include/compu_hip.h): device/buffer management, the batched entry
// points, and the streaming Decoder/Encoder objects that mirror compu's vtables
// (src/decoder/mod.rs:160-166, src/encoder/mod.rs:52-57) on top of the batched GPU kernels.
//
// The streaming objects keep compu's call contract (NeedInput / NeedOutput / Finished, borrowed
// host buffers) but do all codec work on the GPU: input is accumulated in pinned host memory,
// the whole stream seen so far is decoded by the batch kernel (a batch of one), and decoded bytes
// are handed out of a device buffer as the caller provides room -- the same shape as brotli's
// internally buffered decoder that tests/decoder.rs:38-39 already allows for.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "chip_internal.h"
#include "lz4_enc_core.h"

using namespace chip;

namespace {

// Host-state allocator hooks (src/mem.rs:52-57,74-76).  chip_set_allocator may be called from any thread; an object
// keeps the hooks that were installed when it was made, so it is freed by the allocator that allocated it whatever is
// installed later (separate decoders on separate threads must not share unsynchronised globals).
struct Hooks {
    chip_malloc_fn malloc_fn = nullptr;
    chip_free_fn free_fn = nullptr;
    void *opaque = nullptr;
    void *alloc(size_t n) const { return malloc_fn ? malloc_fn(opaque, n) : malloc(n); }
    void release(void *p) const
    {
        if (!p) return;
        if (free_fn) free_fn(opaque, p);
        else free(p);
    }
};
std::mutex g_hooks_mu;
Hooks g_hooks;
Hooks current_hooks()
{
    std::lock_guard<std::mutex> lk(g_hooks_mu);
    return g_hooks;
}

bool device_ok()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// small device+pinned block holding the per-unit descriptor and result words of a batch of one
struct Meta {
    uint64_t in_off, out_off;
    uint32_t in_len, out_cap, out_len, in_used;
    int32_t status;
    uint32_t resume[RESUME_WORDS];  // inflate streaming: see BatchArgs::resume
};

// The arguments of a batch launch over n units of device memory; callers set resume, flags and sel where they use them.
BatchArgs batch_args(int format, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, void *out_base,
                     const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, uint32_t *in_used, int32_t *status)
{
    BatchArgs a;
    a.in_base = (const uint8_t *)in_base;
    a.in_off = in_off;
    a.in_len = in_len;
    a.out_base = (uint8_t *)out_base;
    a.out_off = out_off;
    a.out_cap = out_cap;
    a.out_len = out_len;
    a.in_used = in_used;
    a.status = status;
    a.n = (uint32_t)n;
    a.format = format;
    a.stats = nullptr;
    a.resume = nullptr;
#ifdef CHIP_STATS
    a.stats = getenv("CHIP_STATS_PTR") ? (unsigned long long *)strtoull(getenv("CHIP_STATS_PTR"), nullptr, 0) : nullptr;
#endif
    return a;
}

void pipes_trim();  // defined with the host-batch pipelines below

}  // namespace

extern "C" {

int chip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int chip_set_device(int device) { return hipSetDevice(device) == hipSuccess ? CHIP_OK : CHIP_E_NO_DEVICE; }

const char *chip_version(void) { return "compu-hip 0.1 (gfx950)"; }

void chip_set_allocator(chip_malloc_fn malloc_fn, chip_free_fn free_fn, void *opaque)
{
    std::lock_guard<std::mutex> lk(g_hooks_mu);
    // both or neither: memory from one allocator must never reach the other's free
    g_hooks.malloc_fn = (malloc_fn && free_fn) ? malloc_fn : nullptr;
    g_hooks.free_fn = (malloc_fn && free_fn) ? free_fn : nullptr;
    g_hooks.opaque = (malloc_fn && free_fn) ? opaque : nullptr;
}

void *chip_device_alloc(size_t size)
{
    void *p = nullptr;
    if (hipMalloc(&p, size ? size : 4) != hipSuccess) return nullptr;
    return p;
}
void chip_device_free(void *ptr)
{
    if (ptr) (void)hipFree(ptr);
}
void *chip_pinned_alloc(size_t size)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, size ? size : 4, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void chip_pinned_free(void *ptr)
{
    if (ptr) (void)hipHostFree(ptr);
}
int chip_memcpy_h2d(void *dst, const void *src, size_t size, void *stream)
{
    return hipMemcpyAsync(dst, src, size, hipMemcpyHostToDevice, (hipStream_t)stream) == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}
int chip_memcpy_d2h(void *dst, const void *src, size_t size, void *stream)
{
    return hipMemcpyAsync(dst, src, size, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}
int chip_stream_sync(void *stream) { return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH; }
int chip_trim(void)
{
    pipes_trim();  // cached host-batch pipelines of the current device (streams, staging and device buffers)
    return chip::release_scratch() == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;  // the launch slots of every codec
}

// ---- batched decode ------------------------------------------------------------------------

int chip_decode_batch(int format, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                      void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                      uint32_t *in_used, int32_t *status, void *stream)
{
    return chip_decode_batch_ex(format, 0, n, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, in_used, status, stream);
}

// CHIP_F_MEMBERS goes with the formats that have a concatenation convention (RFC 1952 sec. 2.2, RFC 8878 sec. 3.1), and not with
// CHIP_F_COMPU_STATUS: compu has no multi-member decode whose return values could be mirrored
static bool members_flag_ok(int format, uint32_t flags)
{
    // LZ4 takes no flag at all: compu has no LZ4 whose return values could be mirrored, and concatenated frames are the caller's loop
    if ((format == CHIP_FMT_LZ4_BLOCK || format == CHIP_FMT_LZ4) && flags) return false;
    // Snappy likewise: concatenated streams are one stream of the framing format already
    if ((format == CHIP_FMT_SNAPPY_BLOCK || format == CHIP_FMT_SNAPPY) && flags) return false;
    if (!(flags & CHIP_F_MEMBERS)) return true;
    if (flags & CHIP_F_COMPU_STATUS) return false;
    return format == CHIP_FMT_GZIP || format == CHIP_FMT_AUTO || format == CHIP_FMT_ZSTD || format == CHIP_FMT_DETECT;
}

int chip_decode_batch_ex(int format, uint32_t flags, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                         void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                         uint32_t *in_used, int32_t *status, void *stream)
{
    if (flags & ~(uint32_t)(CHIP_F_COMPU_STATUS | CHIP_F_MEMBERS)) return CHIP_E_INVALID;
    if (!members_flag_ok(format, flags)) return CHIP_E_INVALID;
    if (n == 0) return CHIP_OK;
    if (n > 0x7fffffffull || !in_base || !in_off || !in_len || !out_base || !out_off || !out_cap || !out_len || !in_used ||
        !status || ((uintptr_t)in_base & 3u))
        return CHIP_E_INVALID;
    if (!device_ok()) return CHIP_E_NO_DEVICE;
    BatchArgs a = batch_args(format, n, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, in_used, status);
    a.flags = flags;
    hipError_t e;
    switch (format) {
    case CHIP_FMT_DEFLATE:
    case CHIP_FMT_ZLIB:
    case CHIP_FMT_GZIP:
    case CHIP_FMT_AUTO: e = launch_inflate(a, nullptr, (hipStream_t)stream); break;
    case CHIP_FMT_ZSTD: e = launch_zstd(a, nullptr, 0, (hipStream_t)stream); break;
    case CHIP_FMT_BROTLI: e = launch_brotli_decode(a, (hipStream_t)stream); break;  // CHIP_F_COMPU_STATUS changes nothing
    case CHIP_FMT_LZ4_BLOCK:
    case CHIP_FMT_LZ4: e = launch_lz4(a, nullptr, (hipStream_t)stream); break;
    case CHIP_FMT_SNAPPY_BLOCK:
    case CHIP_FMT_SNAPPY: e = launch_snappy(a, nullptr, (hipStream_t)stream); break;
    case CHIP_FMT_DETECT:
        // Detection::detect routes every unit: one pass buckets the batch by format, then each decoder runs over its own
        // (homogeneous) list of units -- all of it one critical section of the (device, stream) slot (inflate.hip)
        e = launch_routed(a, nullptr, (hipStream_t)stream);
        break;
    default: return CHIP_E_INVALID;
    }
    return e == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}

int chip_decode_batch_sizes(int format, uint32_t flags, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                            uint64_t *out_size, uint32_t *in_used, int32_t *status, void *stream)
{
    // arguments first, the device second (as chip_decode_batch_ex): a refusal needs no GPU
    if (flags & ~(uint32_t)CHIP_F_MEMBERS) return CHIP_E_INVALID;
    if (!members_flag_ok(format, flags)) return CHIP_E_INVALID;
    switch (format) {
    case CHIP_FMT_DEFLATE:
    case CHIP_FMT_ZLIB:
    case CHIP_FMT_GZIP:
    case CHIP_FMT_AUTO:
    case CHIP_FMT_ZSTD:
    case CHIP_FMT_LZ4_BLOCK:
    case CHIP_FMT_LZ4:
    case CHIP_FMT_SNAPPY_BLOCK:
    case CHIP_FMT_SNAPPY:
    case CHIP_FMT_DETECT: break;
    default: return CHIP_E_INVALID;  // brotli: a size pass would be a full decode (header)
    }
    if (n == 0) return CHIP_OK;
    if (n > 0x7fffffffull || !in_base || !in_off || !in_len || !out_size || !in_used || !status || ((uintptr_t)in_base & 3u))
        return CHIP_E_INVALID;
    if (!device_ok()) return CHIP_E_NO_DEVICE;
    BatchArgs a = batch_args(format, n, in_base, in_off, in_len, nullptr, nullptr, nullptr, nullptr, in_used, status);
    a.flags = flags;
    hipError_t e;
    if (format == CHIP_FMT_ZSTD) e = launch_zstd(a, out_size, 0, (hipStream_t)stream);
    else if (format == CHIP_FMT_LZ4_BLOCK || format == CHIP_FMT_LZ4) e = launch_lz4(a, out_size, (hipStream_t)stream);
    else if (format == CHIP_FMT_SNAPPY_BLOCK || format == CHIP_FMT_SNAPPY) e = launch_snappy(a, out_size, (hipStream_t)stream);
    else if (format == CHIP_FMT_DETECT) e = launch_routed(a, out_size, (hipStream_t)stream);  // routed as a decode batch is
    else e = launch_inflate(a, out_size, (hipStream_t)stream);
    return e == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}

}  // extern "C"

namespace {

// the calling thread's current device is put back when a library call that switches devices returns
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (device >= 0 && device != prev) ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// ---- host-memory batches ------------------------------------------------------------------------------------------
// Slices of units alternate between two pipelines (H2D -> kernel -> D2H on a stream each), so the copies of one slice
// overlap the kernel of the other.  A slice whose units lie back to back in index order (the usual layout) moves straight
// between the caller's memory and the device; any other layout (gaps, reverse order, overlaps, a selection of units) is
// packed through pinned staging buffers.  Only the bytes a unit produced (out_len) are ever written to the caller's
// output.  Pipelines (streams, device and pinned buffers) are kept per device between calls.
struct Pipe {
    int device = -1;
    hipStream_t stream = nullptr;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    size_t in_cap = 0, out_cap = 0;
    uint8_t *d_arr = nullptr, *h_arr = nullptr;  // per-unit arrays of the slice, device side and pinned host side
    size_t arr_units = 0;
    uint8_t *h_in = nullptr, *h_out = nullptr;   // pinned staging (packed layouts only)
    size_t h_in_cap = 0, h_out_cap = 0;
    // slice in flight
    size_t k0 = 0, k1 = 0;    // positions [k0, k1) of the unit list (k1 == k0: none)
    bool out_direct = false;
    uint64_t o_lo = 0;
};

std::mutex g_pipe_mu;
std::vector<Pipe *> g_pipe_pool;

Pipe *pipe_get(int device)
{
    {
        std::lock_guard<std::mutex> lk(g_pipe_mu);
        for (size_t i = 0; i < g_pipe_pool.size(); i++)
            if (g_pipe_pool[i]->device == device) {
                Pipe *p = g_pipe_pool[i];
                g_pipe_pool.erase(g_pipe_pool.begin() + (long)i);
                return p;
            }
    }
    Pipe *p = new (std::nothrow) Pipe;
    if (!p) return nullptr;
    p->device = device;
    if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) {
        delete p;
        return nullptr;
    }
    return p;
}

void pipe_put(Pipe *p)
{
    if (!p) return;
    p->k0 = p->k1 = 0;
    std::lock_guard<std::mutex> lk(g_pipe_mu);
    g_pipe_pool.push_back(p);
}

void pipe_destroy(Pipe *p)  // the caller has made p->device current
{
    if (p->stream) {
        (void)hipStreamSynchronize(p->stream);
        chip::release_scratch_of(p->stream);
        (void)hipStreamDestroy(p->stream);
    }
    chip_device_free(p->d_in);
    chip_device_free(p->d_out);
    chip_device_free(p->d_arr);
    chip_pinned_free(p->h_arr);
    chip_pinned_free(p->h_in);
    chip_pinned_free(p->h_out);
    delete p;
}

void pipes_trim()
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return;
    std::vector<Pipe *> mine;
    {
        std::lock_guard<std::mutex> lk(g_pipe_mu);
        for (size_t i = 0; i < g_pipe_pool.size();) {
            if (g_pipe_pool[i]->device == dev) {
                mine.push_back(g_pipe_pool[i]);
                g_pipe_pool.erase(g_pipe_pool.begin() + (long)i);
            } else {
                i++;
            }
        }
    }
    for (Pipe *p : mine) pipe_destroy(p);
}

bool grow_buf(uint8_t *&ptr, size_t &cap, size_t need, bool pinned)
{
    if (need <= cap) return true;
    if (pinned) chip_pinned_free(ptr);
    else chip_device_free(ptr);
    cap = need + (need >> 2) + 4096;
    ptr = (uint8_t *)(pinned ? chip_pinned_alloc(cap) : chip_device_alloc(cap));
    if (!ptr) cap = 0;
    return ptr != nullptr;
}
bool grow_dev(uint8_t *&ptr, size_t &cap, size_t need) { return grow_buf(ptr, cap, need, false); }
bool grow_pinned(uint8_t *&ptr, size_t &cap, size_t need) { return grow_buf(ptr, cap, need, true); }

// A pinned buffer that keeps its first `len` bytes when it grows (doubling, from 64 KiB): the streaming objects' input and output.
bool reserve_pinned(uint8_t **buf, size_t *cap, size_t len, size_t need)
{
    if (need <= *cap) return true;
    size_t c = *cap ? *cap : 65536;
    while (c < need) c *= 2;
    uint8_t *p = (uint8_t *)chip_pinned_alloc(c);
    if (!p) return false;
    if (len) memcpy(p, *buf, len);
    chip_pinned_free(*buf);
    *buf = p;
    *cap = c;
    return true;
}

struct HostBatch {
    const uint8_t *in_base;
    const uint64_t *in_off;
    const uint32_t *in_len;
    uint8_t *out_base;
    const uint64_t *out_off;
    const uint32_t *out_cap;
    uint32_t *out_len, *in_used;  // in_used may be null (encode)
    int32_t *status;
    const uint32_t *sel;  // unit indices to run, ascending (null: 0 .. count)
    size_t count;
    size_t unit(size_t k) const { return sel ? sel[k] : k; }
};

// Runs the units of `hb` on `device` (made current by the caller).  `launch` enqueues the device batch call of one slice.
template <class Launch>
int host_pipeline(const HostBatch &hb, int device, size_t slice_bytes, Launch launch)
{
    if (hb.count == 0) return CHIP_OK;
    if (slice_bytes == 0) slice_bytes = (size_t)256 << 20;
    Pipe *pipes[2] = {pipe_get(device), pipe_get(device)};
    if (!pipes[0] || !pipes[1]) {
        for (Pipe *p : pipes)
            if (p) pipe_put(p);
        return CHIP_E_NOMEM;
    }
    int rc = CHIP_OK;
    // per unit on the device: in_off u64, out_off u64, in_len u32, out_cap u32 | out_len u32, in_used u32, status i32
    auto arr_bytes = [](size_t units) { return units * 36 + 64; };
    // results and payload of the slice a pipeline has in flight -> the caller's memory
    auto collect = [&](Pipe &pp) -> bool {
        if (pp.k1 == pp.k0) return true;
        const size_t m = pp.k1 - pp.k0;
        if (hipStreamSynchronize(pp.stream) != hipSuccess) return false;  // kernel done, result words in h_arr
        const uint32_t *r_len = (const uint32_t *)(pp.h_arr + m * 24), *r_used = r_len + m;
        const int32_t *r_st = (const int32_t *)(r_len + 2 * m);
        const uint64_t *s_out_off = (const uint64_t *)pp.h_arr + m;  // the slice's device-side output offsets
        bool ok = true;
        if (pp.out_direct) {
            // runs of units whose produced bytes lie back to back go in one copy; nothing beyond out_len is written
            size_t u = 0;
            while (u < m && ok) {
                size_t v = u;
                uint64_t run_len = r_len[u];
                while (v + 1 < m && r_len[v] == hb.out_cap[hb.unit(pp.k0 + v)] &&
                       hb.out_off[hb.unit(pp.k0 + v)] + r_len[v] == hb.out_off[hb.unit(pp.k0 + v + 1)]) {
                    v++;
                    run_len += r_len[v];
                }
                if (run_len)
                    ok = hipMemcpyAsync(hb.out_base + hb.out_off[hb.unit(pp.k0 + u)], pp.d_out + s_out_off[u], (size_t)run_len,
                                        hipMemcpyDeviceToHost, pp.stream) == hipSuccess;
                u = v + 1;
            }
            ok = ok && hipStreamSynchronize(pp.stream) == hipSuccess;
        } else {
            uint64_t span = 0;
            for (size_t u = 0; u < m; u++)
                if (r_len[u]) span = s_out_off[u] + r_len[u] > span ? s_out_off[u] + r_len[u] : span;
            if (span) {
                ok = grow_pinned(pp.h_out, pp.h_out_cap, (size_t)span);
                ok = ok && hipMemcpyAsync(pp.h_out, pp.d_out, (size_t)span, hipMemcpyDeviceToHost, pp.stream) == hipSuccess;
                ok = ok && hipStreamSynchronize(pp.stream) == hipSuccess;
                for (size_t u = 0; u < m && ok; u++)
                    if (r_len[u]) memcpy(hb.out_base + hb.out_off[hb.unit(pp.k0 + u)], pp.h_out + s_out_off[u], r_len[u]);
            }
        }
        for (size_t u = 0; u < m; u++) {
            const size_t g = hb.unit(pp.k0 + u);
            hb.out_len[g] = r_len[u];
            if (hb.in_used) hb.in_used[g] = r_used[u];
            hb.status[g] = r_st[u];
        }
        pp.k1 = pp.k0;
        return ok;
    };
    size_t k = 0;
    int turn = 0;
    while (rc == CHIP_OK && k < hb.count) {
        // next slice: positions [k, j) until the byte budget is reached; is it one back-to-back run in memory?
        size_t j = k;
        uint64_t budget = 0, in_sum = 0, out_sum = 0;
        bool in_direct = true, out_direct = true;
        while (j < hb.count) {
            const size_t g = hb.unit(j);
            const uint64_t need = (uint64_t)hb.in_len[g] + hb.out_cap[g];
            if (j > k && budget + need > slice_bytes) break;
            if (j > k) {
                const size_t gp = hb.unit(j - 1);
                // the next unit starts at or (by at most 15 bytes of padding) behind the end of the previous one
                const uint64_t ie = hb.in_off[gp] + hb.in_len[gp], oe = hb.out_off[gp] + hb.out_cap[gp];
                if (hb.in_off[g] < ie || hb.in_off[g] - ie > 15) in_direct = false;
                if (hb.out_off[g] < oe || hb.out_off[g] - oe > 15) out_direct = false;
            }
            budget += need;
            in_sum += ((uint64_t)hb.in_len[g] + 3u) & ~3ull;
            out_sum += ((uint64_t)hb.out_cap[g] + 15u) & ~15ull;
            j++;
        }
        Pipe &pp = *pipes[turn];
        turn ^= 1;
        if (!collect(pp)) {
            rc = CHIP_E_LAUNCH;
            break;
        }
        const size_t m = j - k, g0 = hb.unit(k), gl = hb.unit(j - 1);
        const uint64_t in_lo = hb.in_off[g0] & ~3ull;  // a direct slice keeps the units' alignment relative to a dword-aligned base
        const uint64_t in_span = in_direct ? hb.in_off[gl] + hb.in_len[gl] - in_lo : in_sum;
        const uint64_t o_lo = hb.out_off[g0];
        const uint64_t out_span = out_direct ? hb.out_off[gl] + hb.out_cap[gl] - o_lo : out_sum;
        bool ok = grow_dev(pp.d_in, pp.in_cap, (size_t)((in_span + 3) & ~3ull) + 16) && grow_dev(pp.d_out, pp.out_cap, (size_t)out_span + 16);
        if (ok && m > pp.arr_units) {
            chip_device_free(pp.d_arr);
            chip_pinned_free(pp.h_arr);
            pp.arr_units = m + (m >> 2) + 64;
            pp.d_arr = (uint8_t *)chip_device_alloc(arr_bytes(pp.arr_units));
            pp.h_arr = (uint8_t *)chip_pinned_alloc(arr_bytes(pp.arr_units));
            ok = pp.d_arr && pp.h_arr;
            if (!ok) pp.arr_units = 0;
        }
        if (ok && !in_direct) ok = grow_pinned(pp.h_in, pp.h_in_cap, (size_t)in_span + 16);
        if (!ok) {
            rc = CHIP_E_NOMEM;
            break;
        }
        // per-unit arrays rebased to the slice (and, for a packed slice, the input bytes gathered)
        uint64_t *h_in_off = (uint64_t *)pp.h_arr, *h_out_off = h_in_off + m;
        uint32_t *h_in_len = (uint32_t *)(h_out_off + m), *h_out_cap = h_in_len + m;
        uint64_t ip = 0, op = 0;
        for (size_t u = 0; u < m; u++) {
            const size_t g = hb.unit(k + u);
            h_in_len[u] = hb.in_len[g];
            h_out_cap[u] = hb.out_cap[g];
            if (in_direct) {
                h_in_off[u] = hb.in_off[g] - in_lo;
            } else {
                h_in_off[u] = ip;
                memcpy(pp.h_in + ip, hb.in_base + hb.in_off[g], hb.in_len[g]);
                ip += ((uint64_t)hb.in_len[g] + 3u) & ~3ull;
            }
            if (out_direct) {
                h_out_off[u] = hb.out_off[g] - o_lo;
            } else {
                h_out_off[u] = op;
                op += ((uint64_t)hb.out_cap[g] + 15u) & ~15ull;
            }
        }
        uint64_t *d_in_off = (uint64_t *)pp.d_arr, *d_out_off = d_in_off + m;
        uint32_t *d_in_len = (uint32_t *)(d_out_off + m), *d_out_cap = d_in_len + m, *d_res = d_out_cap + m;
        ok = hipMemcpyAsync(pp.d_arr, pp.h_arr, m * 24, hipMemcpyHostToDevice, pp.stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(pp.d_in, in_direct ? hb.in_base + in_lo : pp.h_in, (size_t)in_span, hipMemcpyHostToDevice, pp.stream) == hipSuccess;
        ok = ok && launch(m, pp.d_in, d_in_off, d_in_len, pp.d_out, d_out_off, d_out_cap, d_res, d_res + m, (int32_t *)(d_res + 2 * m), pp.stream) == CHIP_OK;
        ok = ok && hipMemcpyAsync(pp.h_arr + m * 24, d_res, m * 12, hipMemcpyDeviceToHost, pp.stream) == hipSuccess;
        if (!ok) {
            rc = CHIP_E_LAUNCH;
            break;
        }
        pp.k0 = k;
        pp.k1 = j;
        pp.out_direct = out_direct;
        pp.o_lo = o_lo;
        k = j;
    }
    for (Pipe *p : pipes) {
        if (rc == CHIP_OK) {
            if (!collect(*p)) rc = CHIP_E_LAUNCH;
        } else {
            (void)hipStreamSynchronize(p->stream);
        }
        pipe_put(p);
    }
    return rc;
}

bool host_args_ok(size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, void *out_base, const uint64_t *out_off,
                  const uint32_t *out_cap, uint32_t *out_len, int32_t *status)
{
    return n <= 0x7fffffffull && in_base && in_off && in_len && out_base && out_off && out_cap && out_len && status;
}

}  // namespace

extern "C" {

int chip_decode_batch_host(int format, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                           void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                           uint32_t *in_used, int32_t *status, int device, size_t slice_bytes)
{
    const int dev1[1] = {device};
    return chip_decode_batch_multi(format, n, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, in_used, status, dev1, 1,
                                   slice_bytes);
}

// Contiguous ranges of `list` (unit indices; null = identity) for `parts` workers, balanced by input + output bytes.
static void balanced_cuts(const uint32_t *list, size_t count, const uint32_t *in_len, const uint32_t *out_cap, int parts, size_t *cuts)
{
    uint64_t total = 0;
    for (size_t k = 0; k < count; k++) {
        const size_t g = list ? list[k] : k;
        total += (uint64_t)in_len[g] + out_cap[g] + 64;
    }
    uint64_t acc = 0;
    int next = 1;
    cuts[0] = 0;
    for (size_t k = 0; k < count && next < parts; k++) {
        const size_t g = list ? list[k] : k;
        acc += (uint64_t)in_len[g] + out_cap[g] + 64;
        while (next < parts && acc * (uint64_t)parts >= total * (uint64_t)next) cuts[next++] = k + 1;
    }
    while (next <= parts) cuts[next++] = count;
}

int chip_partition_units(size_t n, const uint32_t *in_len, const uint32_t *out_cap, int parts, size_t *cuts)
{
    if (parts <= 0 || !cuts || (n && (!in_len || !out_cap))) return CHIP_E_INVALID;
    balanced_cuts(nullptr, n, in_len, out_cap, parts, cuts);
    return CHIP_OK;
}

int chip_decode_batch_multi(int format, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, void *out_base,
                            const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, uint32_t *in_used, int32_t *status,
                            const int *devices, int n_devices, size_t slice_bytes)
{
    if (n == 0) return CHIP_OK;
    if (!host_args_ok(n, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, status) || !in_used) return CHIP_E_INVALID;
    switch (format) {
    case CHIP_FMT_DEFLATE: case CHIP_FMT_ZLIB: case CHIP_FMT_GZIP: case CHIP_FMT_AUTO: case CHIP_FMT_ZSTD: case CHIP_FMT_BROTLI:
    case CHIP_FMT_LZ4_BLOCK: case CHIP_FMT_LZ4: case CHIP_FMT_SNAPPY_BLOCK: case CHIP_FMT_SNAPPY: case CHIP_FMT_DETECT: break;
    default: return CHIP_E_INVALID;
    }
    const int visible = chip_device_count();
    if (visible <= 0) return CHIP_E_NO_DEVICE;
    std::vector<int> devs;
    if (!devices || n_devices <= 0) {
        for (int d = 0; d < visible; d++) devs.push_back(d);
    } else {
        for (int k = 0; k < n_devices; k++) {
            int d = devices[k];
            if (d < 0 && hipGetDevice(&d) != hipSuccess) return CHIP_E_NO_DEVICE;
            if (d >= visible) return CHIP_E_INVALID;
            devs.push_back(d);
        }
    }
    const int parts = (int)devs.size();
    // per format one list of units (a mixed batch is bucketed by Detection::detect so that every launch is homogeneous)
    struct Bucket { int format; std::vector<uint32_t> list; bool all; };
    std::vector<Bucket> buckets;
    if (format == CHIP_FMT_DETECT) {
        Bucket bi{CHIP_FMT_AUTO, {}, false}, bz{CHIP_FMT_ZSTD, {}, false};
        for (size_t i = 0; i < n; i++) {
            const int kind = chip_detect((const uint8_t *)in_base + in_off[i], in_len[i]);
            if (kind == CHIP_DETECT_GZIP || kind == CHIP_DETECT_ZLIB) bi.list.push_back((uint32_t)i);
            else if (kind == CHIP_DETECT_ZSTD) bz.list.push_back((uint32_t)i);
            else {
                out_len[i] = 0;
                in_used[i] = 0;
                status[i] = kind == CHIP_DETECT_NONE ? CHIP_NEED_INPUT : CHIP_UNKNOWN_FORMAT;
            }
        }
        if (!bi.list.empty()) buckets.push_back(std::move(bi));
        if (!bz.list.empty()) buckets.push_back(std::move(bz));
    } else {
        buckets.push_back(Bucket{format, {}, true});
    }
    std::vector<std::vector<size_t>> cuts(buckets.size(), std::vector<size_t>((size_t)parts + 1));
    for (size_t b = 0; b < buckets.size(); b++)
        balanced_cuts(buckets[b].all ? nullptr : buckets[b].list.data(), buckets[b].all ? n : buckets[b].list.size(), in_len, out_cap, parts,
                      cuts[b].data());
    std::vector<int> rcs((size_t)parts, CHIP_OK);
    auto worker = [&](int w) {
        DeviceGuard g(devs[(size_t)w]);
        if (!g.ok) {
            rcs[(size_t)w] = CHIP_E_NO_DEVICE;
            return;
        }
        for (size_t b = 0; b < buckets.size() && rcs[(size_t)w] == CHIP_OK; b++) {
            const size_t lo = cuts[b][(size_t)w], hi = cuts[b][(size_t)w + 1];
            if (hi == lo) continue;
            const int fmt = buckets[b].format;
            // a worker's share of an unselected batch is the index range [lo, hi): express it by shifted array pointers
            HostBatch hb{(const uint8_t *)in_base, in_off, in_len, (uint8_t *)out_base, out_off, out_cap, out_len, in_used, status, nullptr, hi - lo};
            if (buckets[b].all) {
                hb.in_off += lo; hb.in_len += lo; hb.out_off += lo; hb.out_cap += lo; hb.out_len += lo; hb.in_used += lo; hb.status += lo;
            } else {
                hb.sel = buckets[b].list.data() + lo;
            }
            rcs[(size_t)w] = host_pipeline(hb, devs[(size_t)w], slice_bytes,
                                           [=](size_t m, const void *di, const uint64_t *dio, const uint32_t *dil, void *dout, const uint64_t *doo,
                                               const uint32_t *doc, uint32_t *dol, uint32_t *diu, int32_t *dst, void *st) {
                                               return chip_decode_batch(fmt, m, di, dio, dil, dout, doo, doc, dol, diu, dst, st);
                                           });
        }
    };
    if (parts == 1) {
        worker(0);
    } else {
        std::vector<std::thread> th;
        for (int w = 0; w < parts; w++) th.emplace_back(worker, w);  // one host thread per GPU: hipSetDevice is per thread
        for (auto &t : th) t.join();
    }
    for (int rc : rcs)
        if (rc != CHIP_OK) return rc;
    return CHIP_OK;
}

int chip_encode_batch_host(int format, int level, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                           void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int32_t *status,
                           int device, size_t slice_bytes)
{
    if (n == 0) return CHIP_OK;
    if (!host_args_ok(n, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, status)) return CHIP_E_INVALID;
    if (!device_ok()) return CHIP_E_NO_DEVICE;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return CHIP_E_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return CHIP_E_INVALID;
    HostBatch hb{(const uint8_t *)in_base, in_off, in_len, (uint8_t *)out_base, out_off, out_cap, out_len, nullptr, status, nullptr, n};
    return host_pipeline(hb, device, slice_bytes,
                         [=](size_t m, const void *di, const uint64_t *dio, const uint32_t *dil, void *dout, const uint64_t *doo,
                             const uint32_t *doc, uint32_t *dol, uint32_t *, int32_t *dst, void *st) {
                             return chip_encode_batch(format, level, m, di, dio, dil, dout, doo, doc, dol, dst, st);
                         });
}

// Detection::detect, src/decoder/mod.rs:28-114 (including the fall-through of the 0x68 arm,
// src/decoder/mod.rs:80-82, which makes `68 xx` zlib headers come out as Unknown).
int chip_detect(const uint8_t *b, size_t len)
{
    if (len < 2) return CHIP_DETECT_NONE;
    if (b[0] == 0x1f && b[1] == 0x8b) return CHIP_DETECT_GZIP;
    if ((((unsigned)b[0] << 8) | b[1]) % 31 == 0) {
        static const uint8_t flg[8][4] = {{0x1d, 0x5b, 0x99, 0xd7}, {0x19, 0x57, 0x95, 0xd3}, {0x15, 0x53, 0x91, 0xcf},
                                          {0x11, 0x4f, 0x8d, 0xcb}, {0x0d, 0x4b, 0x89, 0xc7}, {0x09, 0x47, 0x85, 0xc3},
                                          {0x05, 0x43, 0x81, 0xde}, {0x01, 0x5e, 0x9c, 0xda}};
        if ((b[0] & 0x8f) == 0x08 && b[0] != 0x68) {
            const uint8_t *row = flg[b[0] >> 4];
            for (int i = 0; i < 4; i++)
                if (b[1] == row[i]) return CHIP_DETECT_ZLIB;
        }
    }
    if (len < 4) return CHIP_DETECT_NONE;
    if (b[0] == 0x28 && b[1] == 0xb5 && b[2] == 0x2f && b[3] == 0xfd) return CHIP_DETECT_ZSTD;
    return CHIP_DETECT_UNKNOWN;
}

int chip_detect_batch(size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, int32_t *kind,
                      void *stream)
{
    if (n == 0) return CHIP_OK;
    if (!in_base || !in_off || !in_len || !kind) return CHIP_E_INVALID;
    if (!device_ok()) return CHIP_E_NO_DEVICE;
    return launch_detect(n, (const uint8_t *)in_base, in_off, in_len, kind, (hipStream_t)stream) == hipSuccess ? CHIP_OK
                                                                                                               : CHIP_E_LAUNCH;
}

// ---- error strings -------------------------------------------------------------------------

const char *chip_decoder_strerror(int format, int32_t code)
{
    if (format == CHIP_FMT_BROTLI) {
        // BrotliDecoderErrorString(code), src/decoder/brotli_c.rs (describe_error_fn)
        switch (code) {
        case 0: return "NO_ERROR";
        case 1: return "SUCCESS";
        case 2: return "NEEDS_MORE_INPUT";
        case 3: return "NEEDS_MORE_OUTPUT";
        case -1: return "EXUBERANT_NIBBLE";
        case -2: return "RESERVED";
        case -3: return "EXUBERANT_META_NIBBLE";
        case -4: return "SIMPLE_HUFFMAN_ALPHABET";
        case -5: return "SIMPLE_HUFFMAN_SAME";
        case -6: return "CL_SPACE";
        case -7: return "HUFFMAN_SPACE";
        case -8: return "CONTEXT_MAP_REPEAT";
        case -9: return "BLOCK_LENGTH_1";
        case -10: return "BLOCK_LENGTH_2";
        case -11: return "TRANSFORM";
        case -12: return "DICTIONARY";
        case -13: return "WINDOW_BITS";
        case -14: return "PADDING_1";
        case -15: return "PADDING_2";
        case -16: return "DISTANCE";
        case -19: return "DICTIONARY_NOT_SET";
        case -20: return "INVALID_ARGUMENTS";
        case -21: return "CONTEXT_MODES";
        case -22: return "TREE_GROUPS";
        case -25: return "CONTEXT_MAP";
        case -26: return "RING_BUFFER_1";
        case -27: return "RING_BUFFER_2";
        case -30: return "BLOCK_TYPE_TREES";
        case -31: return "UNREACHABLE";
        default: return "INVALID";
        }
    }
    if (format == CHIP_FMT_ZSTD) {
        // ZSTD_getErrorName(code as usize), src/decoder/zstd.rs:159-164
        switch (code < 0 ? -code : code) {
        case 0: return "No error detected";
        case 1: return "Error (generic)";
        case 10: return "Unknown frame descriptor";
        case 12: return "Version not supported";
        case 14: return "Unsupported frame parameter";
        case 16: return "Frame requires too much memory for decoding";
        case 20: return "Data corruption detected";
        case 22: return "Restored data doesn't match checksum";
        case 30: return "Dictionary is corrupted";
        case 32: return "Dictionary mismatch";
        case 64: return "Allocation error : not enough memory";
        case 70: return "Destination buffer is too small";
        case 72: return "Src size is incorrect";
        default: return "Unspecified error code";
        }
    }
    // zError, src/decoder/zlib_ng.rs:118-123
    static const char *const tab[] = {"need dictionary", "stream end", "", "file error", "stream error",
                                      "data error", "insufficient memory", "buffer error", "incompatible version", ""};
    int idx = 2 - code;
    if (idx < 0 || idx > 9) idx = 9;
    return tab[idx];
}

}  // extern "C"

// ---- streaming decoder -----------------------------------------------------------------------

struct chip_decoder {
    Hooks hooks;  // the allocator this object came from
    int format;
    int device;
    int window_log_max;
    hipStream_t stream;
    uint8_t *h_in;   // pinned: every input byte of the current stream
    size_t h_in_cap, h_in_len;
    uint8_t *d_in;
    size_t d_in_cap;
    uint8_t *d_out;
    size_t d_out_cap;
    Meta *d_meta;
    Meta *h_meta;    // pinned
    bool decoded;    // kernel results below describe h_in[0..h_in_len)
    uint32_t k_out_len, k_in_used;
    int32_t k_status;
    size_t delivered;  // decoded bytes already handed to the caller
    bool done;
    size_t d_in_len;      // input bytes already on the device (the stream only grows)
    uint32_t resume[RESUME_WORDS];  // inflate: last block boundary the kernel reached, running check (BatchArgs::resume); zeros = from the start
    size_t in_dropped;    // input bytes dropped in front of the buffer so far
    uint32_t last_ck;     // resume[0] + 8 * input bytes dropped so far: tells whether a run reached a new block boundary
    uint32_t *d_zres;     // zstd: device blob with the kernel's block checkpoint (header + decode tables), see zstd_unit.h
    uint32_t *h_zhdr;     // zstd: host copy of the checkpoint's ZRES_HDR header words (pinned, behind h_meta)
};

namespace {

// Limits of a streaming object: the kernels address a unit's input by 32-bit bit offsets and its output
// by 32-bit byte offsets.  What is BUFFERED stays far below them (input in front of the last block boundary and output
// that has been handed on are dropped), so only a single deflate block or zstd frame of that size can run into them.
constexpr size_t DEC_IN_LIMIT = (size_t)256 << 20;    // buffered compressed bytes
constexpr size_t DEC_OUT_LIMIT = 0xfffffff0ull;       // decoded bytes held on the device
constexpr size_t DEC_OUT_SOFT = (size_t)8 << 20;      // the device output is not grown past this while the stream makes progress
constexpr size_t DEC_DROP_IN = 65536, DEC_DROP_OUT = (size_t)1 << 20;  // housekeeping thresholds

// Decode what has accumulated.  Input is appended to the device copy (only the new bytes cross the link), an inflate
// stream continues from the last block boundary an earlier call reached (the window in front of it stays on the device,
// the trailer check is carried as a running value), so feeding a long stream in pieces costs O(stream) time and
// O(window + piece) memory.  The device output grows while a run reaches no new boundary without it.
bool dec_run(chip_decoder *d)
{
    const size_t in_len = d->h_in_len;
    const size_t need_in = ((in_len + 3) & ~(size_t)3) + 16;
    if (need_in > d->d_in_cap) {
        const size_t ncap = need_in * 2 + 4096;
        uint8_t *p = (uint8_t *)chip_device_alloc(ncap);
        if (!p) return false;
        chip_device_free(d->d_in);  // (stream-ordered work on it is complete: every call ends with a synchronise)
        d->d_in = p;
        d->d_in_cap = ncap;
        d->d_in_len = 0;  // upload again from the pinned copy
    }
    if (in_len > d->d_in_len) {
        const size_t from = d->d_in_len & ~(size_t)3;  // keep the copies dword aligned
        if (hipMemcpyAsync(d->d_in + from, d->h_in + from, in_len - from, hipMemcpyHostToDevice, d->stream) != hipSuccess) return false;
        d->d_in_len = in_len;
    }
    const bool inflate = d->format != CHIP_FMT_ZSTD && d->format != CHIP_FMT_BROTLI;
    const bool brotli = d->format == CHIP_FMT_BROTLI;
    if (!inflate && !d->d_zres) {
        d->d_zres = (uint32_t *)chip_device_alloc(brotli ? ZRES_HDR * 4 : ZRES_BYTES);  // brotli: the header only
        if (!d->d_zres || hipMemsetAsync(d->d_zres, 0, ZRES_HDR * 4, d->stream) != hipSuccess) return false;
    }
    size_t cap = d->d_out_cap;
    if (cap == 0) cap = in_len * 4 > 65536 ? in_len * 4 : 65536;
    if (cap > DEC_OUT_SOFT && d->d_out_cap == 0) cap = DEC_OUT_SOFT;
    for (;;) {
        if (cap > DEC_OUT_LIMIT) cap = DEC_OUT_LIMIT;
        if (cap > d->d_out_cap) {
            uint8_t *p = (uint8_t *)chip_device_alloc(cap);
            if (!p) return false;
            const size_t keep = d->k_out_len;  // the window of a stream that resumes and what has not been delivered yet
            if (keep && hipMemcpyAsync(p, d->d_out, keep, hipMemcpyDeviceToDevice, d->stream) != hipSuccess) return false;
            if (keep && hipStreamSynchronize(d->stream) != hipSuccess) return false;
            chip_device_free(d->d_out);
            d->d_out = p;
            d->d_out_cap = cap;
        }
        Meta m = {0, 0, (uint32_t)in_len, (uint32_t)d->d_out_cap, 0, 0, 0, {0}};
        for (uint32_t k = 0; k < RESUME_WORDS; k++) m.resume[k] = d->resume[k];
        *d->h_meta = m;
        if (hipMemcpyAsync(d->d_meta, d->h_meta, sizeof(Meta), hipMemcpyHostToDevice, d->stream) != hipSuccess) return false;
        Meta *dm = d->d_meta;
        BatchArgs a = batch_args(d->format, 1, d->d_in, &dm->in_off, &dm->in_len, d->d_out, &dm->out_off, &dm->out_cap, &dm->out_len, &dm->in_used, &dm->status);
        a.resume = inflate ? dm->resume : d->d_zres;
        hipError_t e = inflate  ? launch_inflate(a, nullptr, d->stream)
                       : brotli ? launch_brotli_decode(a, d->stream)
                                : launch_zstd(a, nullptr, d->window_log_max, d->stream);
        if (e != hipSuccess) return false;
        if (hipMemcpyAsync(d->h_meta, d->d_meta, sizeof(Meta), hipMemcpyDeviceToHost, d->stream) != hipSuccess) return false;
        if (!inflate && hipMemcpyAsync(d->h_zhdr, d->d_zres, ZRES_HDR * 4, hipMemcpyDeviceToHost, d->stream) != hipSuccess) return false;
        if (hipStreamSynchronize(d->stream) != hipSuccess) return false;
        uint32_t ck;
        if (inflate) {
            for (uint32_t k = 0; k < RESUME_WORDS; k++) d->resume[k] = d->h_meta->resume[k];
            ck = d->resume[0] + 8u * (uint32_t)d->in_dropped;
        } else if (brotli) {
            ck = d->h_zhdr[0] + 8u * (uint32_t)d->in_dropped;  // a bit offset
        } else {
            ck = d->h_zhdr[0] + (uint32_t)d->in_dropped;
        }
        const bool progress = ck != d->last_ck || d->h_meta->out_len > d->delivered;  // a new block boundary, or bytes to hand on
        d->last_ck = ck;
        d->k_out_len = d->h_meta->out_len;
        // out of device output: a stream that got somewhere hands on what it has and continues from its last boundary in a
        // buffer of the same size; one that did not (a block, or a zstd window, larger than the buffer) gets a larger one
        if (d->h_meta->status == CHIP_NEED_OUTPUT && d->d_out_cap < DEC_OUT_LIMIT && (!progress || d->d_out_cap < DEC_OUT_SOFT)) {
            cap = d->d_out_cap * 2;
            continue;
        }
        break;
    }
    d->k_in_used = d->h_meta->in_used;
    d->k_status = d->h_meta->status;
    d->decoded = true;
    return true;
}

// Forward move of d_out[from .. from + n) to d_out[0 .. n), in pieces no longer than the distance: source and destination of a
// piece never overlap.
bool dec_move_down(chip_decoder *d, size_t from, size_t n)
{
    for (size_t done = 0; done < n;) {
        const size_t c = n - done < from ? n - done : from;
        if (hipMemcpyAsync(d->d_out + done, d->d_out + from + done, c, hipMemcpyDeviceToDevice, d->stream) != hipSuccess) return false;
        done += c;
    }
    return hipStreamSynchronize(d->stream) == hipSuccess;
}

// Between calls of a stream that goes on: drop the input in front of the last block boundary and the output that has been
// handed on and that no later block can reach -- inflate: in front of the 32 KiB window of that boundary (BatchArgs::resume
// says how the kernel is told); zstd: in front of the frame's window, and never behind what the running XXH64 covers (the
// checkpoint header, zstd_unit.h).  A single-segment zstd frame's window is its content size: nothing is dropped for it, as libzstd
// keeps it whole (src/decoder/zstd.rs:98-136 sits on ZSTD_decompressStream).
bool dec_compact(chip_decoder *d)
{
    if (!d->decoded) return true;
    if (d->k_status != CHIP_NEED_INPUT && d->k_status != CHIP_NEED_OUTPUT) return true;
    if (d->format == CHIP_FMT_BROTLI || d->format == CHIP_FMT_ZSTD) {
        // the checkpoint header (zstd_unit.h; brotli's metablock checkpoint: chip_internal.h, BRES_WORDS): input in front of the
        // boundary's byte, output in front of the window of the boundary that has been handed on.  zh[0] is 1 + the boundary's
        // offset in the input, in bits for brotli and in bytes for zstd.
        const bool brotli = d->format == CHIP_FMT_BROTLI;
        const uint32_t in_unit = brotli ? 8u : 1u;
        uint32_t *zh = d->h_zhdr;
        if (zh[0] == 0) return true;  // no metablock / block done yet
        bool dirty = false;
        const size_t drop_in = (((size_t)zh[0] - 1u) / in_unit) & ~(size_t)3;  // the boundary's byte, dword aligned down
        if (drop_in >= DEC_DROP_IN) {
            memmove(d->h_in, d->h_in + drop_in, d->h_in_len - drop_in);
            d->h_in_len -= drop_in;
            d->d_in_len = 0;  // the (short) rest is uploaded again
            zh[0] -= in_unit * (uint32_t)drop_in;
            d->in_dropped += drop_in;
            d->k_in_used = d->k_in_used > drop_in ? d->k_in_used - (uint32_t)drop_in : 0;
            dirty = true;
        }
        const uint64_t window = (uint64_t)zh[8] | ((uint64_t)zh[9] << 32);
        const uint64_t dropped = (uint64_t)zh[12] | ((uint64_t)zh[13] << 32);
        const size_t r1 = zh[1];
        size_t keep_from = r1 > window ? r1 - (size_t)window : 0;
        if (keep_from > d->delivered) keep_from = d->delivered;
        if (!brotli && (zh[5] & 1u)) {  // zstd's content checksum: bytes the running hash has not taken yet stay
            const uint64_t hashed = (uint64_t)zh[14] | ((uint64_t)zh[15] << 32);
            const size_t hrel = (size_t)(hashed - dropped);
            if (keep_from > hrel) keep_from = hrel;
        }
        keep_from &= ~(size_t)15;
        if (keep_from >= DEC_DROP_OUT) {
            if (!dec_move_down(d, keep_from, d->k_out_len - keep_from)) return false;
            d->delivered -= keep_from;
            d->k_out_len -= (uint32_t)keep_from;
            zh[1] -= (uint32_t)keep_from;
            const uint64_t nd = dropped + keep_from;
            zh[12] = (uint32_t)nd;
            zh[13] = (uint32_t)(nd >> 32);
            dirty = true;
        }
        if (dirty) {
            if (hipMemcpyAsync(d->d_zres, zh, ZRES_HDR * 4, hipMemcpyHostToDevice, d->stream) != hipSuccess) return false;
            if (hipStreamSynchronize(d->stream) != hipSuccess) return false;
        }
        return true;
    }
    const uint32_t r0 = d->resume[0], r1 = d->resume[1];
    if (r0 == 0) return true;
    const size_t bnd = r0 >> 3;  // the boundary's byte; 8 bytes stay in front of it so that the offset never becomes 0
    const size_t drop_in = bnd > 8 ? ((bnd - 8) & ~(size_t)3) : 0;
    if (drop_in >= DEC_DROP_IN) {
        memmove(d->h_in, d->h_in + drop_in, d->h_in_len - drop_in);
        d->h_in_len -= drop_in;
        d->d_in_len = 0;  // the (short) rest is uploaded again
        d->resume[0] -= 8u * (uint32_t)drop_in;
        d->in_dropped += drop_in;
        d->k_in_used = d->k_in_used > drop_in ? d->k_in_used - (uint32_t)drop_in : 0;
    }
    size_t keep_from = d->delivered < r1 ? d->delivered : r1;
    keep_from = keep_from > 32768 ? ((keep_from - 32768) & ~(size_t)15) : 0;
    if (keep_from >= DEC_DROP_OUT) {
        if (!dec_move_down(d, keep_from, d->k_out_len - keep_from)) return false;
        d->delivered -= keep_from;
        d->k_out_len -= (uint32_t)keep_from;
        d->resume[1] -= (uint32_t)keep_from;
        d->resume[5] += (uint32_t)keep_from;
    }
    return true;
}

// Decoded bytes a call may hand on.  A brotli stream that ended in an error hands on what libbrotlidec would have flushed before
// reaching it: its ring buffer goes out whole (the checkpoint's [10] is its size where the run stopped), and what earlier calls
// handed on stays handed on.
size_t dec_out_limit(const chip_decoder *d)
{
    if (d->format != CHIP_FMT_BROTLI || d->k_status >= 0) return d->k_out_len;
    const uint64_t rsz = d->h_zhdr[10];
    const uint64_t dropped = (uint64_t)d->h_zhdr[12] | ((uint64_t)d->h_zhdr[13] << 32);
    const uint64_t flushed = rsz ? (dropped + d->k_out_len) / rsz * rsz : 0;
    size_t lim = flushed > dropped ? (size_t)(flushed - dropped) : 0;
    if (lim > d->k_out_len) lim = d->k_out_len;
    return lim > d->delivered ? lim : d->delivered;
}

void dec_clear(chip_decoder *d)
{
    d->h_in_len = 0;
    d->decoded = false;
    d->k_out_len = d->k_in_used = 0;
    d->k_status = CHIP_NEED_INPUT;
    d->delivered = 0;
    d->done = false;
    d->d_in_len = 0;
    for (uint32_t k = 0; k < RESUME_WORDS; k++) d->resume[k] = 0;
    d->last_ck = 0;
    d->in_dropped = 0;
    if (d->h_zhdr) memset(d->h_zhdr, 0, ZRES_HDR * 4);
    if (d->d_zres) {  // the next stream starts from its frame header
        (void)hipMemsetAsync(d->d_zres, 0, ZRES_HDR * 4, d->stream);
        (void)hipStreamSynchronize(d->stream);
    }
}

}  // namespace

extern "C" {

chip_decoder *chip_decoder_new(int format, const chip_decoder_opts *opts)
{
    if (format != CHIP_FMT_DEFLATE && format != CHIP_FMT_ZLIB && format != CHIP_FMT_GZIP && format != CHIP_FMT_AUTO &&
        format != CHIP_FMT_ZSTD && format != CHIP_FMT_BROTLI)
        return nullptr;
    if (!device_ok()) return nullptr;  // no CPU codec behind this backend
    int device = opts ? opts->device : -1;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return nullptr;
    DeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    const Hooks hooks = current_hooks();
    chip_decoder *d = (chip_decoder *)hooks.alloc(sizeof(chip_decoder));
    if (!d) return nullptr;
    memset(d, 0, sizeof *d);
    d->hooks = hooks;
    d->format = format;
    d->device = device;
    d->window_log_max = opts ? opts->window_log_max : 0;
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
        hooks.release(d);
        return nullptr;
    }
    d->d_meta = (Meta *)chip_device_alloc(sizeof(Meta));
    d->h_meta = (Meta *)chip_pinned_alloc(sizeof(Meta) + ZRES_HDR * 4);
    d->h_zhdr = d->h_meta ? (uint32_t *)(d->h_meta + 1) : nullptr;
    if (!d->d_meta || !d->h_meta || !reserve_pinned(&d->h_in, &d->h_in_cap, 0, 65536)) {
        chip_decoder_free(d);
        return nullptr;
    }
    dec_clear(d);
    return d;
}

chip_decode_result chip_decode(chip_decoder *d, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len)
{
    chip_decode_result r = {in_len, out_len, CHIP_NEED_INPUT, 0};
    if (!d) {
        r.status = -1;
        r.err = -2;  // Z_STREAM_ERROR
        return r;
    }
    if (d->done) {
        // like zlib in its DONE state: Finished again, nothing consumed
        r.status = CHIP_FINISHED;
        return r;
    }
    DeviceGuard guard(d->device);  // the caller's current device is put back on return
    auto fail = [&](int32_t err) {
        r.status = -1;
        r.err = err;
        return r;
    };
    if (!guard.ok) return fail(-2);
    const bool stream_end_known = d->decoded && (d->k_status == CHIP_FINISHED || d->k_status < 0 || d->k_status == CHIP_NEED_DICT);
    size_t taken = 0;
    if (!stream_end_known && in_len) {
        if (!dec_compact(d)) return fail(-4);
        if (d->h_in_len + in_len > DEC_IN_LIMIT) return fail(-4);  // Z_MEM_ERROR: more buffered input than a unit can address
        if (!reserve_pinned(&d->h_in, &d->h_in_cap, d->h_in_len, d->h_in_len + in_len)) return fail(-4);
        memcpy(d->h_in + d->h_in_len, in, in_len);
        d->h_in_len += in_len;
        taken = in_len;
        d->decoded = false;
    }
    size_t n_total = 0;
    for (;;) {
        if (!d->decoded && !dec_run(d)) return fail(-4);
        const size_t avail = dec_out_limit(d) - d->delivered;
        const size_t n = avail < out_len - n_total ? avail : out_len - n_total;
        if (n) {
            if (hipMemcpyAsync(out + n_total, d->d_out + d->delivered, n, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
                hipStreamSynchronize(d->stream) != hipSuccess)
                return fail(-4);
            d->delivered += n;
            n_total += n;
        }
        // everything decoded so far is handed on but the device buffer was the limit: make room and decode on
        if (d->delivered == d->k_out_len && d->k_status == CHIP_NEED_OUTPUT && n_total < out_len) {
            const bool zs = d->format == CHIP_FMT_ZSTD || d->format == CHIP_FMT_BROTLI;
            const uint32_t before = zs ? d->h_zhdr[1] : d->resume[1];
            if (!dec_compact(d)) return fail(-4);
            if ((zs ? d->h_zhdr[1] : d->resume[1]) == before && d->d_out_cap >= DEC_OUT_LIMIT) break;  // nothing could be dropped and nothing can grow
            d->decoded = false;
            continue;
        }
        break;
    }
    const size_t n = n_total;
    r.output_remain = out_len - n;
    // bytes of this call that lie behind the end of the stream go back to the caller
    size_t giveback = 0;
    if (d->k_status == CHIP_FINISHED || d->k_status < 0 || d->k_status == CHIP_NEED_DICT) {
        size_t trailing = d->h_in_len - d->k_in_used;
        giveback = trailing < taken ? trailing : taken;
        d->h_in_len -= giveback;
    }
    r.input_remain = (in_len - taken) + giveback;
    if (d->format == CHIP_FMT_BROTLI) {
        // BrotliDecoderDecompressStream's result, src/decoder/brotli_c.rs:43-60: Success once the stream is done and its output
        // handed on, NeedsMoreOutput while decoded bytes wait, an error once what libbrotlidec flushes in front of it
        // (dec_out_limit) is handed on -- in the call that hands on its last byte -- else NeedsMoreInput
        if (d->k_status < 0) {
            if (d->delivered < dec_out_limit(d)) {
                r.status = CHIP_NEED_OUTPUT;
            } else {
                r.status = -1;
                r.err = d->k_status;
            }
        } else if (d->k_status == CHIP_FINISHED && d->delivered == d->k_out_len) {
            d->done = true;
            r.status = CHIP_FINISHED;
        } else if (d->delivered < d->k_out_len || d->k_status == CHIP_NEED_OUTPUT) {
            r.status = CHIP_NEED_OUTPUT;
        } else {
            r.status = CHIP_NEED_INPUT;
        }
        return r;
    }
    if (d->format == CHIP_FMT_ZSTD) {
        // src/decoder/zstd.rs:113-135: 0 -> Finished (frame done AND flushed); else a full output buffer -> NeedOutput,
        // whatever else happened; else no error -> NeedInput; else the error
        // A call that returns an error leaves input.pos where the caller set it (compu's decode_fn reports input.size - input.pos,
        // src/decoder/zstd.rs): the whole input of the call is reported as remaining, also when an empty output range turns the
        // error into NeedOutput.
        if (d->k_status < 0 && d->delivered == d->k_out_len) r.input_remain = in_len;
        if (d->k_status == CHIP_FINISHED && d->delivered == d->k_out_len) {
            d->done = true;
            r.status = CHIP_FINISHED;
        } else if (d->k_status < 0 && d->delivered == d->k_out_len && out_len != 0) {
            // The call that gets to the damage: ZSTD_decompressStream returns the error before it writes output.pos, so compu sees 0 and
            // reports the error -- with none of the bytes this call could have handed on (the oracle states the rule; pinned against
            // the system's libzstd in tests/test_oracle_zstd.py).  Only an empty output range (0 == 0) reads as NeedOutput.
            r.status = -1;
            r.err = d->k_status;
            r.output_remain = out_len;
        } else if (r.output_remain == 0 || d->delivered < d->k_out_len || d->k_status == CHIP_NEED_OUTPUT) {
            r.status = CHIP_NEED_OUTPUT;
        } else if (d->k_status == CHIP_NEED_INPUT || d->k_status == CHIP_FINISHED) {
            r.status = CHIP_NEED_INPUT;
        } else {
            r.status = -1;
            r.err = d->k_status;
        }
        return r;
    }
    if (d->delivered < d->k_out_len || d->k_status == CHIP_NEED_OUTPUT) {
        r.status = CHIP_NEED_OUTPUT;
        return r;
    }
    if (d->k_status == CHIP_FINISHED) {
        d->done = true;
        r.status = CHIP_FINISHED;
    } else if (d->k_status == CHIP_NEED_INPUT) {
        // Z_OK with avail_in == 0 -> NeedInput; a call that made no progress at all is zlib's
        // Z_BUF_ERROR, which compu maps to NeedOutput (src/decoder/mod.rs:476-481)
        r.status = (in_len == 0 && n == 0) ? CHIP_NEED_OUTPUT : CHIP_NEED_INPUT;
    } else {
        r.status = -1;
        r.err = d->k_status == CHIP_NEED_DICT ? Z_NEED_DICT : d->k_status;
    }
    return r;
}

void chip_decoder_footprint(const chip_decoder *d, size_t *pinned_bytes, size_t *device_bytes)
{
    if (pinned_bytes) *pinned_bytes = d ? d->h_in_cap + sizeof(Meta) + ZRES_HDR * 4 : 0;
    if (!device_bytes) return;
    *device_bytes = 0;
    if (!d) return;
    const bool brotli = d->format == CHIP_FMT_BROTLI;
    *device_bytes = d->d_in_cap + d->d_out_cap + sizeof(Meta) + (d->d_zres ? (brotli ? ZRES_HDR * 4 : ZRES_BYTES) : 0);
    if (brotli) {  // the kernel's table slots for this decoder's stream (one 128 KiB slot, one worst-case slot)
        DeviceGuard guard(d->device);
        *device_bytes += chip::brotli_scratch_bytes_of(d->stream);
    }
}

chip_decoder *chip_decoder_reset(chip_decoder *d)
{
    if (d) {
        DeviceGuard guard(d->device);
        dec_clear(d);
    }
    return d;
}

void chip_decoder_free(chip_decoder *d)
{
    if (!d) return;
    DeviceGuard guard(d->device);
    if (d->stream) {
        chip::release_scratch_of(d->stream);  // the stream's launch slots go with it
        (void)hipStreamDestroy(d->stream);
    }
    chip_pinned_free(d->h_in);
    chip_pinned_free(d->h_meta);
    chip_device_free(d->d_in);
    chip_device_free(d->d_out);
    chip_device_free(d->d_meta);
    chip_device_free(d->d_zres);
    const Hooks hooks = d->hooks;
    hooks.release(d);
}

}  // extern "C"

// ---- batched encode --------------------------------------------------------------------------------

extern "C" {

size_t chip_encode_bound(int format, size_t in_len)
{
    // zstd: raw blocks of 128 KiB (3-byte headers), the largest frame header (18 bytes) and the checksum
    if (format == CHIP_FMT_ZSTD) return in_len + 3 * (in_len ? (in_len + (128u << 10) - 1) / (128u << 10) : 1) + 18 + 4;
    // brotli: uncompressed metablocks of 128 KiB (the first header shares its bytes with the WBITS field: at most 4 bytes, then 3
    // each), the closing empty last metablock (1 byte) -- 4 bytes per metablock and 2 more are a safe margin
    if (format == CHIP_FMT_BROTLI) return in_len + 4 * (in_len ? (in_len + (128u << 10) - 1) / (128u << 10) : 1) + 2;
    // LZ4: the block format's own worst case; a frame of stored 64 KiB blocks with every checksum
    if (format == CHIP_FMT_LZ4_BLOCK) return (size_t)lz4enc::block_bound(in_len);
    if (format == CHIP_FMT_LZ4) return (size_t)lz4enc::frame_bound(in_len);
    size_t blocks = in_len ? (in_len + 65534) / 65535 : 1;
    size_t wrap = format == CHIP_FMT_BGZF ? 26 : format == CHIP_FMT_GZIP ? 18 : format == CHIP_FMT_ZLIB ? 6 : 0;  // header + trailer
    // dynamic levels: a block holds at least 65472 tokens and costs at most 6 bytes more than its stored form
    return in_len + 5 * blocks + 6 * (in_len / 65472 + 1) + 5 + wrap;
}

int chip_encode_batch(int format, int level, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                      void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int32_t *status,
                      void *stream)
{
    return chip_encode_batch_ex(format, level, CHIP_STRATEGY_DEFAULT, n, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, status, stream);
}

int chip_encode_batch_ex(int format, int level, int strategy, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                         void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int32_t *status,
                         void *stream)
{
    // arguments first, the device second: a refusal needs no GPU
    if (n == 0) return CHIP_OK;
    if (!host_args_ok(n, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, status)) return CHIP_E_INVALID;
    switch (format) {
    case CHIP_FMT_ZSTD:
        if (level < -131072 || level > 131072 || strategy < CHIP_ZSTD_STRATEGY_DEFAULT || strategy > CHIP_ZSTD_STRATEGY_BTULTRA2) return CHIP_E_INVALID;
        break;
    case CHIP_FMT_BROTLI:  // level = quality 0..11 (0 = libbrotlienc's default 11), strategy = compu's mode byte 0..3 (recorded only)
        if (level < 0 || level > 11 || strategy < 0 || strategy > 3) return CHIP_E_INVALID;
        break;
    case CHIP_FMT_LZ4_BLOCK:
    case CHIP_FMT_LZ4:  // level -1 .. 12 (the lz4 command's range), strategy = CHIP_LZ4_S_* bits (frames only)
        if (!lz4_encode_args_ok(format, level, strategy)) return CHIP_E_INVALID;
        break;
    case CHIP_FMT_DEFLATE:
    case CHIP_FMT_ZLIB:
    case CHIP_FMT_GZIP:
    case CHIP_FMT_BGZF:  // one BGZF block per unit (deflate.hip's wrapper branch); units above 65280 bytes are CHIP_ENC_ERROR
        if (level == -1) level = 6;  // zlib's Z_DEFAULT_COMPRESSION
        if (level < 0 || level > 9 || strategy < CHIP_STRATEGY_DEFAULT || strategy > CHIP_STRATEGY_FIXED) return CHIP_E_INVALID;
        break;
    default: return CHIP_E_INVALID;
    }
    if (!device_ok()) return CHIP_E_NO_DEVICE;
    const BatchArgs a = batch_args(format, n, in_base, in_off, in_len, out_base, out_off, out_cap, out_len, nullptr, status);
    const uint32_t wl = zenc::MAX_DIST_LOG;  // the batch frames use zstd's default window_log (27)
    hipError_t e;
    if (format == CHIP_FMT_ZSTD) e = launch_zstd_encode(a, level, strategy, wl, wl, ZF_FIRST | ZF_LAST | ZF_ONESHOT, nullptr, (hipStream_t)stream);
    else if (format == CHIP_FMT_BROTLI) e = launch_brotli_encode(a, level, 22, ZF_FIRST | ZF_LAST, nullptr, (hipStream_t)stream);
    else if (format == CHIP_FMT_LZ4_BLOCK || format == CHIP_FMT_LZ4) e = launch_lz4_encode(a, level, strategy, (hipStream_t)stream);
    else e = launch_deflate_l1(a, level, 7u | ((uint32_t)strategy << 8), format == CHIP_FMT_ZLIB ? 1u : 0u, 0, nullptr, (hipStream_t)stream);
    return e == hipSuccess ? CHIP_OK : CHIP_E_LAUNCH;
}

}  // extern "C"

// ---- streaming encoder -----------------------------------------------------------------------------
// Same contract as internal_zlib_impl_encode! (src/encoder/mod.rs:334-370): Process buffers input,
// Flush / Finish compress what is buffered as one byte-aligned deflate segment on the GPU (a sync
// marker or the final-block flag closes it), and compressed bytes are handed out as the caller
// provides room.

struct chip_encoder {
    Hooks hooks;  // the allocator this object came from
    int mode, level, device, strategy;
    hipStream_t stream;
    uint8_t *h_in;  // pinned: input not yet compressed
    size_t h_in_cap, h_in_len;
    uint8_t *d_in, *d_out;
    size_t d_in_cap, d_out_cap;
    uint8_t *h_out;  // pinned: compressed bytes not yet delivered
    size_t h_out_cap, h_out_len, delivered;
    struct EMeta {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len;
        int32_t status;
        uint32_t check, pad;
    } *d_meta, *h_meta;
    bool started, finished;
    uint32_t check;
    uint64_t total_in;
    // zstd (mode == CHIP_FMT_ZSTD): window_log of the options, and the repeat offsets + XXH64 state carried between segments;
    // brotli (mode == CHIP_FMT_BROTLI): lgwin of the options (level = quality, strategy = mode), and the distance ring
    int wlog;
    ZEncStream *d_zs;
    BEncStream *d_bs;
};

namespace {

void enc_clear(chip_encoder *e)
{
    e->h_in_len = 0;
    e->h_out_len = e->delivered = 0;
    e->started = e->finished = false;
    e->check = e->mode == CHIP_FMT_ZLIB ? 1u : 0u;
    e->total_in = 0;
}

// compress the buffered input as one segment and append it to h_out
bool enc_segment(chip_encoder *e, bool final)
{
    const size_t n = e->h_in_len;
    const bool zstd = e->mode == CHIP_FMT_ZSTD, brotli = e->mode == CHIP_FMT_BROTLI;
    // zstd: with a small window_log the blocks are smaller than the 128 KiB chip_encode_bound counts with
    const size_t zblock = e->wlog < 17 ? (size_t)1 << e->wlog : (size_t)128 << 10;
    const size_t bound = zstd ? n + 3 * (n / zblock + 1) + 22 + 16 : chip_encode_bound(e->mode, n) + 16;
    if (n + 16 > e->d_in_cap) {
        chip_device_free(e->d_in);
        e->d_in_cap = (n + 16) * 2;
        e->d_in = (uint8_t *)chip_device_alloc(e->d_in_cap);
        if (!e->d_in) return false;
    }
    if (bound > e->d_out_cap) {
        chip_device_free(e->d_out);
        e->d_out_cap = bound * 2;
        e->d_out = (uint8_t *)chip_device_alloc(e->d_out_cap);
        if (!e->d_out) return false;
    }
    if (n && hipMemcpyAsync(e->d_in, e->h_in, n, hipMemcpyHostToDevice, e->stream) != hipSuccess) return false;
    chip_encoder::EMeta m = {0, 0, (uint32_t)n, (uint32_t)bound, 0, 0, 0, 0};
    *e->h_meta = m;
    if (hipMemcpyAsync(e->d_meta, e->h_meta, sizeof m, hipMemcpyHostToDevice, e->stream) != hipSuccess) return false;
    chip_encoder::EMeta *dm = e->d_meta;
    const BatchArgs a = batch_args(e->mode, 1, e->d_in, &dm->in_off, &dm->in_len, e->d_out, &dm->out_off, &dm->out_cap, &dm->out_len, nullptr, &dm->status);
    if (zstd) {
        // a frame compressed in one call (Finish with the whole input buffered) is single-segment with Frame_Content_Size, as
        // libzstd's one-call ZSTD_e_end; otherwise the header declares a window: the segments are at most 1 MiB and no match
        // crosses them, so 2^20 (or the option's smaller window_log) covers every distance
        const uint32_t flags = (e->started ? 0u : ZF_FIRST) | (final ? ZF_LAST : 0u) | (!e->started && final ? ZF_ONESHOT : 0u);
        const uint32_t wl_single = e->wlog < 27 ? (uint32_t)e->wlog : 27u, wl_window = e->wlog < 20 ? (uint32_t)e->wlog : 20u;
        if (launch_zstd_encode(a, e->level, e->strategy, wl_single, wl_window, flags, e->d_zs, e->stream) != hipSuccess) return false;
    } else if (brotli) {
        // every segment but the last ends byte-aligned (Flush's empty metadata metablock); the ring goes on to the next one
        const uint32_t flags = (e->started ? 0u : ZF_FIRST) | (final ? ZF_LAST : 0u);
        if (launch_brotli_encode(a, e->level, e->wlog, flags, e->d_bs, e->stream) != hipSuccess) return false;
    } else {
        const uint32_t flags = (e->started ? 0u : 1u) | (final ? 2u | 4u : 0u) | ((uint32_t)e->strategy << 8);
        if (launch_deflate_l1(a, e->level, flags, e->check, e->total_in, &e->d_meta->check, e->stream) != hipSuccess) return false;
    }
    if (hipMemcpyAsync(e->h_meta, e->d_meta, sizeof m, hipMemcpyDeviceToHost, e->stream) != hipSuccess) return false;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return false;
    if (e->h_meta->status != CHIP_ENC_FINISHED) return false;
    const size_t got = e->h_meta->out_len;
    if (!reserve_pinned(&e->h_out, &e->h_out_cap, e->h_out_len, e->h_out_len + got)) return false;
    if (got && (hipMemcpyAsync(e->h_out + e->h_out_len, e->d_out, got, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
                hipStreamSynchronize(e->stream) != hipSuccess))
        return false;
    e->h_out_len += got;
    e->check = e->h_meta->check;
    e->total_in += n;
    e->h_in_len = 0;
    e->started = true;
    if (final) e->finished = true;
    return true;
}

// What the three public constructors share once the options are parsed and found valid.  state_bytes: the device block a
// zstd or brotli encoder carries from one segment to the next (d_zs / d_bs), 0 for none.
chip_encoder *encoder_new_common(int mode, int level, int strategy, int wlog, int device, size_t state_bytes)
{
    if (!device_ok()) return nullptr;  // no CPU codec behind this backend
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return nullptr;
    DeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    const Hooks hooks = current_hooks();
    chip_encoder *e = (chip_encoder *)hooks.alloc(sizeof(chip_encoder));
    if (!e) return nullptr;
    memset(e, 0, sizeof *e);
    e->hooks = hooks;
    e->mode = mode;
    e->level = level;
    e->strategy = strategy;
    e->wlog = wlog;
    e->device = device;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
        hooks.release(e);
        return nullptr;
    }
    e->d_meta = (chip_encoder::EMeta *)chip_device_alloc(sizeof(chip_encoder::EMeta));
    e->h_meta = (chip_encoder::EMeta *)chip_pinned_alloc(sizeof(chip_encoder::EMeta));
    void *state = state_bytes ? chip_device_alloc(state_bytes) : nullptr;
    if (mode == CHIP_FMT_ZSTD) e->d_zs = (ZEncStream *)state;
    else e->d_bs = (BEncStream *)state;
    if (!e->d_meta || !e->h_meta || (state_bytes && !state) || !reserve_pinned(&e->h_in, &e->h_in_cap, 0, 65536) ||
        !reserve_pinned(&e->h_out, &e->h_out_cap, 0, 65536)) {
        chip_encoder_free(e);
        return nullptr;
    }
    enc_clear(e);
    return e;
}

}  // namespace

extern "C" {

chip_encoder *chip_encoder_new(const chip_encoder_opts *opts)
{
    // defaults of ZlibOptions::new(), src/encoder/zlib_common.rs:59-66
    int mode = opts ? opts->mode : CHIP_FMT_GZIP, level = opts ? opts->compression : 9;
    const int strategy = opts ? opts->strategy : CHIP_STRATEGY_DEFAULT, mem_level = opts ? opts->mem_level : 0;
    if (level == -1) level = 6;  // "Use -1 for zlib default" (zlib_common.rs:96-103): Z_DEFAULT_COMPRESSION
    if ((mode != CHIP_FMT_DEFLATE && mode != CHIP_FMT_ZLIB && mode != CHIP_FMT_GZIP) || level < 0 || level > 9) return nullptr;
    // what deflateInit2_ refuses (Z_STREAM_ERROR -> None, src/encoder/zlib_ng.rs:81-86): memLevel outside 1..9, unknown strategy
    if (strategy < CHIP_STRATEGY_DEFAULT || strategy > CHIP_STRATEGY_FIXED || mem_level < 0 || mem_level > 9) return nullptr;
    return encoder_new_common(mode, level, strategy, 0, opts ? opts->device : -1, 0);
}

chip_encoder *chip_encoder_new_zstd(const chip_zstd_encoder_opts *opts)
{
    // ZstdOptions::new(), src/encoder/zstd.rs:70-77: level 3 (ZSTD_CLEVEL_DEFAULT), strategy Default, window_log 27
    int level = opts ? opts->level : 3;
    const int strategy = opts ? opts->strategy : CHIP_ZSTD_STRATEGY_DEFAULT, wlog = opts ? opts->window_log : 27;
    // what ZSTD_CCtx_setParameter refuses (apply() -> None, src/encoder/zstd.rs:107-124)
    if (level < -131072 || level > 131072 || strategy < CHIP_ZSTD_STRATEGY_DEFAULT || strategy > CHIP_ZSTD_STRATEGY_BTULTRA2 ||
        wlog < 10 || wlog > 31)
        return nullptr;
    if (level == 0) level = 3;
    if (level > 22) level = 22;
    return encoder_new_common(CHIP_FMT_ZSTD, level, strategy, wlog, opts ? opts->device : -1, sizeof(ZEncStream));
}

chip_encoder *chip_encoder_new_brotli(const chip_brotli_encoder_opts *opts)
{
    // BrotliOptions::new(), src/encoder/brotli_common.rs: quality and mode unset (libbrotlienc's quality 11), lgwin 22
    const int quality = opts ? opts->quality : 0, mode = opts ? opts->mode : 0, lgwin = opts ? opts->lgwin : 22;
    if (quality < 0 || quality > 11 || mode < 0 || mode > 3 || lgwin < 10 || lgwin > 24) return nullptr;
    return encoder_new_common(CHIP_FMT_BROTLI, quality ? quality : 11, mode, lgwin, opts ? opts->device : -1, sizeof(BEncStream));
}

chip_encode_result chip_encode(chip_encoder *e, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, int op)
{
    chip_encode_result r = {in_len, out_len, CHIP_ENC_ERROR};
    if (!e || op < CHIP_OP_PROCESS || op > CHIP_OP_FINISH) return r;
    DeviceGuard guard(e->device);
    if (!guard.ok) return r;
    // Memory stays bounded: buffered input is compressed as a (byte-aligned, non-final) segment once ENC_SEGMENT bytes have
    // gathered, and no more input is taken while more than ENC_BACKLOG compressed bytes wait for the caller -- as zlib's
    // deflate() stops consuming when avail_out is 0.
    constexpr size_t ENC_SEGMENT = (size_t)1 << 20, ENC_BACKLOG = (size_t)4 << 20;
    size_t taken = 0;
    while (!e->finished && taken < in_len && e->h_out_len - e->delivered <= ENC_BACKLOG) {
        const size_t room = ENC_SEGMENT - (e->h_in_len < ENC_SEGMENT ? e->h_in_len : ENC_SEGMENT);
        const size_t k = in_len - taken < room ? in_len - taken : room;
        if (!reserve_pinned(&e->h_in, &e->h_in_cap, e->h_in_len, e->h_in_len + k)) return r;
        memcpy(e->h_in + e->h_in_len, in + taken, k);
        e->h_in_len += k;
        taken += k;
        if (e->h_in_len >= ENC_SEGMENT && taken < in_len && !enc_segment(e, false)) return r;  // the rest of this call's input follows
    }
    if (!e->finished && e->h_in_len >= ENC_SEGMENT && op == CHIP_OP_PROCESS && !enc_segment(e, false)) return r;
    if (!e->finished && taken == in_len && (op == CHIP_OP_FLUSH || op == CHIP_OP_FINISH) &&
        (e->h_in_len || op == CHIP_OP_FINISH || !e->started)) {
        if (!enc_segment(e, op == CHIP_OP_FINISH)) return r;
    }
    size_t avail = e->h_out_len - e->delivered, k = avail < out_len ? avail : out_len;
    if (k) memcpy(out, e->h_out + e->delivered, k);
    e->delivered += k;
    if (e->delivered == e->h_out_len) e->h_out_len = e->delivered = 0;
    r.input_remain = in_len - taken;
    r.output_remain = out_len - k;
    if (e->mode == CHIP_FMT_BROTLI) {
        // src/encoder/brotli_c.rs:63-84: NeedOutput while compressed bytes wait (BrotliEncoderHasMoreOutput), otherwise Finished
        // for Finish and Continue for Process and Flush (a failure returned Error above)
        if (e->h_out_len != 0) r.status = CHIP_ENC_NEED_OUTPUT;
        else r.status = op == CHIP_OP_FINISH ? CHIP_ENC_FINISHED : CHIP_ENC_CONTINUE;
        return r;
    }
    if (e->mode == CHIP_FMT_ZSTD) {
        // ZSTD_compressStream2's return value -> EncodeStatus, src/encoder/zstd.rs:174-197.  It is 0 when no compressed byte
        // waits for delivery, and for Flush also nothing is buffered, for Finish also the frame is closed; 0 is Finished for
        // Finish and Continue otherwise, anything else NeedOutput when the output was filled to its last byte.
        const bool waiting = e->h_out_len != 0;
        const bool zero = !waiting && (op == CHIP_OP_PROCESS || (e->h_in_len == 0 && taken == in_len)) &&
                          (op != CHIP_OP_FINISH || e->finished);
        if (zero) r.status = op == CHIP_OP_FINISH ? CHIP_ENC_FINISHED : CHIP_ENC_CONTINUE;
        else r.status = k == out_len ? CHIP_ENC_NEED_OUTPUT : CHIP_ENC_CONTINUE;
        return r;
    }
    // deflate() return code -> EncodeStatus, src/encoder/mod.rs:357-367: with Finish, anything short of
    // Z_STREAM_END is NeedOutput; otherwise Z_OK is Continue and a call without progress (Z_BUF_ERROR) NeedOutput
    if (op == CHIP_OP_FINISH) r.status = (e->finished && e->h_out_len == 0) ? CHIP_ENC_FINISHED : CHIP_ENC_NEED_OUTPUT;
    else r.status = (taken || k) ? CHIP_ENC_CONTINUE : CHIP_ENC_NEED_OUTPUT;
    return r;
}

chip_encoder *chip_encoder_reset(chip_encoder *e)
{
    if (e) enc_clear(e);
    return e;
}

void chip_encoder_free(chip_encoder *e)
{
    if (!e) return;
    DeviceGuard guard(e->device);
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
        chip::release_scratch_of(e->stream);  // the stream's launch slots go with it
        (void)hipStreamDestroy(e->stream);
    }
    chip_pinned_free(e->h_in);
    chip_pinned_free(e->h_out);
    chip_pinned_free(e->h_meta);
    chip_device_free(e->d_in);
    chip_device_free(e->d_out);
    chip_device_free(e->d_meta);
    chip_device_free(e->d_zs);
    chip_device_free(e->d_bs);
    const Hooks hooks = e->hooks;
    hooks.release(e);
}

}  // extern "C"
