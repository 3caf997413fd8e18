// Internal declarations shared by the HIP translation units of libcompu_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/compu_hip.h"
#include "zstd_enc_core.h"

namespace chip {

// Per-unit running state codes used inside kernels (never exported).
constexpr int32_t ST_RUNNING = 0x7fffffff;

// zlib return codes carried in DecodeError (src/decoder/mod.rs:482)
constexpr int32_t Z_NEED_DICT = 2;
constexpr int32_t Z_DATA_ERROR = -3;

// ZSTD_ErrorCode values carried (negated) in DecodeError (src/decoder/zstd.rs:131)
constexpr int32_t ZSTD_E_GENERIC = 1;
constexpr int32_t ZSTD_E_PREFIX_UNKNOWN = 10;
constexpr int32_t ZSTD_E_FRAMEPARAM_UNSUPPORTED = 14;
constexpr int32_t ZSTD_E_WINDOW_TOO_LARGE = 16;
constexpr int32_t ZSTD_E_CORRUPTION = 20;
constexpr int32_t ZSTD_E_CHECKSUM_WRONG = 22;
constexpr int32_t ZSTD_E_DICT_WRONG = 32;

constexpr uint32_t RESUME_WORDS = 6;

// The streaming zstd decoder's checkpoint in device memory (written by zstd_kernel, sized by api.hip): a header of ZRES_HDR words, then the
// first ZSAVE_WORDS words of the kernel's LDS state (its decode tables; zstd_unit.h asserts that this is where `weights` starts), then slack.
constexpr uint32_t ZRES_HDR = 24;
constexpr uint32_t ZSAVE_WORDS = 2312;
constexpr size_t ZRES_BYTES = (size_t)(ZRES_HDR + ZSAVE_WORDS) * 4 + 64;

struct BatchArgs {
    const uint8_t *in_base;
    const uint64_t *in_off;
    const uint32_t *in_len;
    uint8_t *out_base;
    const uint64_t *out_off;
    const uint32_t *out_cap;
    uint32_t *out_len;
    uint32_t *in_used;
    int32_t *status;
    uint32_t n;
    int32_t format;
    unsigned long long *stats;  // diagnostic builds only (-DCHIP_STATS): 16 words per unit, else nullptr
    // inflate, streaming decoder only (else nullptr): RESUME_WORDS words per unit, in and out --
    //  [0] bit offset (in the unit's input as it is handed over) of the last block boundary reached, 0 = start from the beginning
    //  [1] output bytes produced up to there, as an offset into the unit's output range
    //  [2] wrapper kind (0 raw, 1 zlib, 2 gzip)
    //  [3] running check value (Adler-32 / CRC-32) over the first [4] bytes of the stream's output
    //  [4] output bytes the running check covers, counted from the start of the stream
    //  [5] output bytes the caller has dropped in front of the output range (offset 0 = stream byte [5]), low 32 bits of
    //      the stream's output count = [5] + offset
    // A later call over the unconsumed input (the caller may drop input in front of the boundary and output in front of the
    // 32 KiB window, adjusting [0], [1] and [5]) continues from that boundary.
    uint32_t *resume;
    // Routed batches (CHIP_FMT_DETECT): the kernel works on units sel[0 .. *sel_n) instead of 0 .. n (both device
    // pointers, written by route_kernel earlier on the same stream); nullptr = all n units in index order.
    const uint32_t *sel = nullptr;
    const uint32_t *sel_n = nullptr;
    uint32_t flags = 0;  // CHIP_F_* of chip_decode_batch_ex (include/compu_hip.h)
};
// What zstd_tokens_kernel (zstd_unit.h compiled with CHIP_ZSTD_TOKENS; zstd_tokens.hip) takes beside a BatchArgs whose units are the blocks
// of ONE frame: in_off 0 and in_len the frame's for every unit, out_off / out_cap the block's literal slot in scratch.
struct ZTokArgs {
    const chip_zstd_block *blocks;  // chip_zstd_blocks' records
    const uint32_t *seq_base;       // sequences in front of each block
    uint32_t *tok;                  // 3 words per sequence: literal length, match length, offset (bit 31: symbolic)
    uint32_t *res;                  // 8 words per block: rep0..2 handed on, literal mode (0 input, 1 RLE, 2 slot), its place / byte, Regenerated_Size
    uint64_t window;
};
constexpr uint32_t ZTOK_SLOT_SLACK = 8736;  // a literal slot is Regenerated_Size + this: the Huffman walk's scratch rows (zstd_unit.h asserts it)
hipError_t launch_zstd_tokens(const BatchArgs &a, const ZTokArgs &tk, hipStream_t stream);
// (zstd_tokens.hip) XXH64 of n bytes on one wave, its low 32 bits to *got
hipError_t launch_zstd_xxh(const uint8_t *p, uint32_t n, uint32_t *got, hipStream_t stream);
// (zstd_tokens.hip) the running XXH64 `st` brought forward over n bytes on one wave, the new state to *out (device memory)
hipError_t launch_zstd_xxh_update(const uint8_t *p, uint32_t n, const chip_xxh64_state &st, chip_xxh64_state *out, hipStream_t stream);
constexpr uint32_t F_COMPU_STATUS = 1u;  // = CHIP_F_COMPU_STATUS
constexpr uint32_t F_MEMBERS = 2u;       // = CHIP_F_MEMBERS

// launchers (each only enqueues on `stream`)
// inflate.hip: out_size == nullptr decodes the batch.  Else the size pass (chip_decode_batch_sizes): a.out_base / out_off / out_cap /
// out_len are not read; the decoded length of unit i goes to out_size[i].  Both share one (device, stream) slot.
hipError_t launch_inflate(const BatchArgs &a, uint64_t *out_size, hipStream_t stream);
// (inflate_sizes.hip: the size pass's launch itself, for launch_inflate, which holds the slot)
hipError_t enqueue_inflate_sizes(const BatchArgs &a, uint64_t *out_size, uint32_t *scratch, uint32_t *counter, uint32_t blocks, hipStream_t stream);
// (inflate_members.hip: the same for a CHIP_F_MEMBERS batch; out_size != nullptr launches the size pass, else the decoder)
hipError_t enqueue_inflate_members(const BatchArgs &a, uint64_t *out_size, uint32_t *scratch, uint32_t *counter, uint32_t blocks, hipStream_t stream);
// (inflate_parallel_markers.hip: the marker decode of chip_inflate_parallel, for inflate_parallel.hip, which holds the slot: a.n units
// that begin at bit bit0[u] of their first input byte and write 16-bit elements; a.out_off counts bytes, a.out_cap and a.out_len
// elements; `blocks` waves with SCRATCH_WORDS of token rows each)
hipError_t enqueue_inflate_markers(const BatchArgs &a, const uint32_t *bit0, uint32_t *scratch, uint32_t *counter, uint32_t blocks, hipStream_t stream);
// zstd.hip: out_size == nullptr decodes the batch, else the size pass, as launch_inflate; window_log_max 0 = 27
hipError_t launch_zstd(const BatchArgs &a, uint64_t *out_size, int window_log_max, hipStream_t stream);
// (zstd_sizes.hip: the size pass's launch itself, for launch_zstd; wlog_max is the limit itself, never 0)
hipError_t enqueue_zstd_sizes(const BatchArgs &a, uint64_t *out_size, int wlog_max, hipStream_t stream);
// (zstd_members.hip, zstd_members_sizes.hip: the same for a CHIP_F_MEMBERS batch, decoder and size pass)
hipError_t enqueue_zstd_members(const BatchArgs &a, int wlog_max, hipStream_t stream);
hipError_t enqueue_zstd_members_sizes(const BatchArgs &a, uint64_t *out_size, int wlog_max, hipStream_t stream);
// lz4.hip: CHIP_FMT_LZ4_BLOCK / CHIP_FMT_LZ4 (a.format), out_size == nullptr decodes the batch, else the size pass; no scratch
hipError_t launch_lz4(const BatchArgs &a, uint64_t *out_size, hipStream_t stream);
// (lz4.hip) XXH32, seed 0, of n bytes on one wave, to *got (device memory)
hipError_t launch_lz4_xxh(const uint8_t *p, uint64_t n, uint32_t *got, hipStream_t stream);
// snappy.hip: CHIP_FMT_SNAPPY_BLOCK / CHIP_FMT_SNAPPY (a.format), out_size == nullptr decodes the batch, else the size pass; no scratch
hipError_t launch_snappy(const BatchArgs &a, uint64_t *out_size, hipStream_t stream);
// lz4_enc.hip: the batch encoder of CHIP_FMT_LZ4_BLOCK / CHIP_FMT_LZ4 (a.format); lz4_encode_args_ok is the refusal that needs no
// device: level -1 .. 12, strategy 0 for blocks and CHIP_LZ4_S_* bits for frames
bool lz4_encode_args_ok(int format, int level, int strategy);
hipError_t launch_lz4_encode(const BatchArgs &a, int level, int strategy, hipStream_t stream);
// launch_slots.hip: the cached launch scratch of every codec ("Launch slots")
hipError_t release_scratch();                 // every slot of the current device, after a device sync
void release_scratch_of(hipStream_t stream);  // the slots of one (drained) stream of the current device
// Detection-driven router of a mixed batch: appends the index of every gzip / zlib unit to sel_inflate and of every zstd
// frame to sel_zstd (counts[0], counts[1], zeroed by the call) and answers units that are neither at once (their length to
// out_size, the size pass's array, when that is given).
hipError_t launch_route(const BatchArgs &a, uint64_t *out_size, uint32_t *sel_inflate, uint32_t *sel_zstd, uint32_t *counts, hipStream_t stream);
// a whole CHIP_FMT_DETECT batch (router + both decoders over their lists, or with out_size both size kernels) under one lock of the
// (device, stream) slot, with which the router's scratch is cached
hipError_t launch_routed(const BatchArgs &a, uint64_t *out_size, hipStream_t stream);
hipError_t launch_detect(size_t n, const uint8_t *in_base, const uint64_t *in_off, const uint32_t *in_len, int32_t *kind,
                         hipStream_t stream);
hipError_t launch_deflate_l1(const BatchArgs &a, int level, uint32_t flags, uint32_t check_seed, uint64_t total_before,
                             uint32_t *check_out, hipStream_t stream);

// zstd encoder (zstd_enc.hip).  Flags: ZF_FIRST writes the frame header (and starts the repeat offsets and the XXH64 state),
// ZF_LAST ends the frame (last block, checksum), ZF_ONESHOT allows the single-segment header with Frame_Content_Size.
constexpr uint32_t ZF_FIRST = 1u, ZF_LAST = 2u, ZF_ONESHOT = 4u;
// what a streaming zstd encoder carries on the device from one segment to the next
struct ZEncStream {
    uint32_t rep[3], pad;
    zenc::Xxh xxh;
};
hipError_t launch_zstd_encode(const BatchArgs &a, int level, int strategy, uint32_t wlog_single, uint32_t wlog_window, uint32_t flags,
                              ZEncStream *stream_state, hipStream_t stream);

// brotli encoder (brotli_enc.hip).  Flags: ZF_FIRST writes the WBITS field and starts the distance ring, ZF_LAST closes the stream
// (otherwise the segment ends byte-aligned).  quality 0..11 (0 = 11), lgwin 10..24.
struct BEncStream {
    uint32_t ring[4];  // the distance ring carried from one segment to the next, last distance first
};
hipError_t launch_brotli_encode(const BatchArgs &a, int quality, int lgwin, uint32_t flags, BEncStream *stream_state, hipStream_t stream);

// brotli decoder (brotli.hip): a persistent launch with a 128 KiB table slot per wave, then an always-enqueued launch on 64 waves
// with worst-case slots for the units whose metablock tables did not fit (an overflow list on the device).
// BatchArgs::resume (streaming only): the checkpoint written at every metablock boundary -- [0] 1 + bit offset of the boundary in
// the unit's input (0 = start of the stream), [1] output bytes up to it, [2..5] the distance ring, oldest first, [6] WBITS,
// [7] libbrotlidec's ring buffer size at the boundary, [8,9] the window (2^WBITS bytes), [10] the ring buffer size where the run
// stopped, [12,13] output bytes the HOST has dropped in front of the output range (host-written).  The host allocates
// ZRES_HDR words for it (the header size the streaming code copies for zstd as well).
constexpr uint32_t BRES_WORDS = 16;
static_assert(BRES_WORDS <= ZRES_HDR, "the brotli checkpoint fits the header the streaming code copies");
hipError_t launch_brotli_decode(const BatchArgs &a, hipStream_t stream);
size_t brotli_scratch_bytes_of(hipStream_t stream);  // device bytes its per-wave table slots hold for `stream` (streaming footprint)

// Detection::detect (src/decoder/mod.rs:28-114) on device: first 2-4 bytes of a unit -> CHIP_DETECT_*.
// The FLG table of mod.rs:44-55 is packed one word per CINFO; the 0x68 row never matches in the
// reference (mod.rs:80-82 lacks the `return`) and is kept that way.
__device__ __forceinline__ int32_t detect_kind(const uint8_t *b, uint32_t len)
{
    if (len < 2) return CHIP_DETECT_NONE;
    const uint32_t b0 = b[0], b1 = b[1];
    if (b0 == 0x1f && b1 == 0x8b) return CHIP_DETECT_GZIP;
    if (((b0 << 8) | b1) % 31 == 0 && (b0 & 0x8f) == 0x08 && b0 != 0x68) {
        const uint32_t rows[8] = {0x1d5b99d7u, 0x195795d3u, 0x155391cfu, 0x114f8dcbu, 0x0d4b89c7u, 0x094785c3u, 0x054381deu, 0x015e9cdau};
        const uint32_t r = rows[b0 >> 4];
        if (b1 == (r >> 24) || b1 == ((r >> 16) & 0xff) || b1 == ((r >> 8) & 0xff) || b1 == (r & 0xff)) return CHIP_DETECT_ZLIB;
    }
    if (len < 4) return CHIP_DETECT_NONE;
    return (b0 == 0x28 && b1 == 0xb5 && b[2] == 0x2f && b[3] == 0xfd) ? CHIP_DETECT_ZSTD : CHIP_DETECT_UNKNOWN;
}

// address spaces: LDS pointers keep theirs through calls and selects (a generic pointer to LDS becomes flat accesses), pointers
// into HBM keep theirs through scalar round trips
#define LDS_AS __attribute__((address_space(3)))
#define GAS __attribute__((address_space(1)))

// ---- wavefront helpers (wave = 64 lanes, one wave per workgroup in the codec kernels) ----------
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << lane_id()) - 1ull; }
__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t l)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}
__device__ __forceinline__ uint32_t rdfirst(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// The same for a pointer: tells the compiler that a value every lane holds alike is wave-uniform, so that it lives in
// scalar registers and loops over it become scalar branches instead of exec-mask loops.
template <typename T>
__device__ __forceinline__ T *rdfirst_ptr(T *p)
{
    const uint64_t v = (uint64_t)(uintptr_t)p;
    return (T *)(uintptr_t)(((uint64_t)rdfirst((uint32_t)(v >> 32)) << 32) | rdfirst((uint32_t)v));
}

// DPP lane moves within the wave (gfx9 controls): lanes without a source keep 0
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}

// inclusive prefix sum across the wave: Hillis-Steele inside each row of 16 lanes (row_shr:1,2,4,8),
// then the row totals are carried over with row_bcast:15 (rows 1,3) and row_bcast:31 (rows 2,3)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += dpp_or_zero<0x111>(v);
    v += dpp_or_zero<0x112>(v);
    v += dpp_or_zero<0x114>(v);
    v += dpp_or_zero<0x118>(v);
    v += dpp_or_zero<0x142, 0xa>(v);
    v += dpp_or_zero<0x143, 0xc>(v);
    return v;
}

// inclusive running maximum across the wave (same DPP ladder; 0 is the identity for unsigned max)
__device__ __forceinline__ uint32_t wave_incl_max_scan(uint32_t v)
{
    uint32_t t;
    t = dpp_or_zero<0x111>(v); v = v > t ? v : t;
    t = dpp_or_zero<0x112>(v); v = v > t ? v : t;
    t = dpp_or_zero<0x114>(v); v = v > t ? v : t;
    t = dpp_or_zero<0x118>(v); v = v > t ? v : t;
    t = dpp_or_zero<0x142, 0xa>(v); v = v > t ? v : t;
    t = dpp_or_zero<0x143, 0xc>(v); v = v > t ? v : t;
    return v;
}

// value of the previous lane (lane 0 gets 0): DPP wave_shr:1
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) { return dpp_or_zero<0x138>(v); }

// LDS written by some lanes of the (single) wave, read by others: order + visibility
#define WSYNC() __syncthreads()
// The same for LDS only: leaves global loads and stores in flight (a one-wave workgroup needs no s_barrier, LDS
// operations of a wave complete in order; the memory clobber keeps the compiler from moving or forwarding LDS accesses)
#define LSYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

}  // namespace chip
