/*
 * compu_hip.h -- C ABI of the MI355X (gfx950) batched compression backend for compu.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / C++ types.  Each entry point
 * names the reference interface it replaces (paths relative to the compu crate root).  A Rust
 * `hip` Interface variant binds these 1:1 (INTEGRATION.md shows the glue).
 *
 * Everything here runs on the GPU.  There is no CPU codec behind this library: if no HIP device
 * is usable the constructors return NULL / the batch calls return CHIP_E_NO_DEVICE.
 */
#ifndef COMPU_HIP_H
#define COMPU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- shared enums -------------------------------------------------------------------------- */

/* decoder::DecodeStatus, src/decoder/mod.rs:139-146 (same order) */
enum { CHIP_NEED_INPUT = 0, CHIP_NEED_OUTPUT = 1, CHIP_FINISHED = 2 };
/* Batch status only: the zlib header asks for a preset dictionary.  zlib answers Z_NEED_DICT (+2),
 * which compu passes through as Err(DecodeError(2)) (src/decoder/mod.rs:482); the value 2 is taken
 * by CHIP_FINISHED in the per-unit status array, hence a code of its own.  chip_decode() reports
 * it as err = 2 like the reference. */
enum { CHIP_NEED_DICT = 3 };
/* Batch status only, CHIP_FMT_DETECT: the unit is neither gzip, zlib nor zstd (Detection::Unknown);
 * a unit too short to classify (detect() == None) reports CHIP_NEED_INPUT. */
enum { CHIP_UNKNOWN_FORMAT = 4 };

/* encoder::EncodeOp src/encoder/mod.rs:12-23, encoder::EncodeStatus src/encoder/mod.rs:27-38 */
enum { CHIP_OP_PROCESS = 0, CHIP_OP_FLUSH = 1, CHIP_OP_FINISH = 2 };
enum { CHIP_ENC_CONTINUE = 0, CHIP_ENC_NEED_OUTPUT = 1, CHIP_ENC_FINISHED = 2, CHIP_ENC_ERROR = 3 };

/* decoder::ZlibMode src/decoder/zlib_common.rs:4-15 and encoder ZlibMode
 * src/encoder/zlib_common.rs:28-37 use zlib's windowBits values; zstd gets its own tag. */
enum {
    CHIP_FMT_DEFLATE = -15,
    CHIP_FMT_ZLIB = 15,
    CHIP_FMT_GZIP = 31,
    CHIP_FMT_AUTO = 47, /* decoder only: zlib or gzip, src/decoder/zlib_common.rs:11-14 */
    CHIP_FMT_ZSTD = 100,
    /* RFC 7932 brotli (decoder: Interface::brotli_c, src/decoder/brotli_c.rs; encoder: chip_encoder_new_brotli and the batch
     * calls) -- no large-window streams (a WINDOW_BITS error, as for compu, which never sets
     * BROTLI_DECODER_PARAM_LARGE_WINDOW), no shared dictionaries; not part of CHIP_FMT_DETECT routing (compu cannot detect
     * brotli) */
    CHIP_FMT_BROTLI = 101,
    /* LZ4 ("LZ4: blocks and frames" and "LZ4: encoding" below): one raw block of the LZ4 block format, delimited by in_len[i], and one
     * frame of the LZ4 frame format.  The batch calls only (device, host and multi); not part of CHIP_FMT_DETECT routing, not with
     * CHIP_F_COMPU_STATUS or CHIP_F_MEMBERS, and the streaming chip_decoder_new does not take them (compu has no LZ4). */
    CHIP_FMT_LZ4_BLOCK = 102,
    CHIP_FMT_LZ4 = 103,
    /* Snappy ("Snappy: blocks and framed streams" below): one raw block (a varint preamble and elements: what snappy::RawCompress
     * writes and a Parquet page holds), delimited by in_len[i], and one stream of the framing format (a .sz file).  Decoding only,
     * the batch calls only (device, host and multi); not part of CHIP_FMT_DETECT routing, not with CHIP_F_COMPU_STATUS or
     * CHIP_F_MEMBERS, not taken by the streaming objects or by any encode entry point (compu has no Snappy). */
    CHIP_FMT_SNAPPY_BLOCK = 104,
    CHIP_FMT_SNAPPY = 105,
    /* chip_encode_batch / _ex / _host and chip_encode_bound only: every unit becomes one BGZF block (below).  Decoding takes
     * CHIP_FMT_GZIP with the arrays of chip_bgzf_plan; the streaming chip_encoder_new does not take this tag. */
    CHIP_FMT_BGZF = 131,
    /* chip_decode_batch only: route every unit by Detection::detect (src/decoder/mod.rs:28-114) to the
     * zlib/gzip or the zstd decoder -- the mixed gzip+zstd batch of BASELINE.json configs[4] */
    CHIP_FMT_DETECT = 0
};

/* decoder::Detection src/decoder/mod.rs:9-21; CHIP_DETECT_NONE is Rust's `None` (too few bytes) */
enum { CHIP_DETECT_NONE = -1, CHIP_DETECT_ZSTD = 0, CHIP_DETECT_GZIP = 1, CHIP_DETECT_ZLIB = 2, CHIP_DETECT_UNKNOWN = 3 };

/* library-level failures of the batch calls (not codec errors) */
enum { CHIP_OK = 0, CHIP_E_NO_DEVICE = -100, CHIP_E_INVALID = -101, CHIP_E_LAUNCH = -102, CHIP_E_NOMEM = -103 };

/* decoder::Decode src/decoder/mod.rs:150-157.  status is Ok(DecodeStatus) when err == 0 and
 * Err(DecodeError(err)) otherwise (err = zlib's negative code, or -(ZSTD_ErrorCode)). */
typedef struct {
    size_t input_remain;
    size_t output_remain;
    int32_t status;
    int32_t err;
} chip_decode_result;

/* encoder::Encode src/encoder/mod.rs:42-49 */
typedef struct {
    size_t input_remain;
    size_t output_remain;
    int32_t status;
} chip_encode_result;

/* ---- device / library ---------------------------------------------------------------------- */

/* Number of usable gfx950 devices (0 if none); never initialises more than the HIP runtime. */
int chip_device_count(void);
/* Select the device used by subsequent calls of this thread (hipSetDevice semantics). */
int chip_set_device(int device);
const char *chip_version(void);

/* src/mem.rs:27-76 routes every codec allocation through compu_malloc/compu_free.  Host-side
 * state of this backend goes through the same hooks when installed (signatures of
 * compu_malloc_with_state / compu_free_with_state, src/mem.rs:52-57,74-76); device memory comes
 * from hipMalloc and staging memory from hipHostMalloc. */
typedef void *(*chip_malloc_fn)(void *opaque, size_t size);
typedef void (*chip_free_fn)(void *opaque, void *ptr);
void chip_set_allocator(chip_malloc_fn malloc_fn, chip_free_fn free_fn, void *opaque);

/* Device and pinned-host buffers (north star: src/buffer.rs grows pinned-host + device types). */
void *chip_device_alloc(size_t size);
void chip_device_free(void *ptr);
void *chip_pinned_alloc(size_t size);
void chip_pinned_free(void *ptr);
int chip_memcpy_h2d(void *dst_dev, const void *src_host, size_t size, void *stream);
int chip_memcpy_d2h(void *dst_host, const void *src_dev, size_t size, void *stream);
int chip_stream_sync(void *stream);
/* The inflate kernel keeps a token scratch per (device, stream) it has been launched on: one 64 KiB slot per
 * resident wave, about 270 MB on an MI355X, allocated at the first launch and reused.  chip_trim() waits for the
 * current device and gives that memory back (the next launch allocates again).  The brotli decoder keeps a table slot per wave in
 * the same way: 128 KiB per resident wave (at most 16 per CU, about 512 MiB on an MI355X) plus 64 worst-case slots of about
 * 1.4 MB for the units whose metablock tables do not fit the small one (min(n, 64) of them; a streaming decoder keeps one of
 * each, freed with it); chip_trim() releases them too.  No reference counterpart:
 * zlib-ng's inflate state is ~40 KiB of host memory per decoder (src/decoder/zlib_ng.rs:29-55). */
int chip_trim(void);

/* ---- streaming decoder: mirrors decoder::Interface, src/decoder/mod.rs:160-166 --------------- */

typedef struct chip_decoder chip_decoder;

typedef struct {
    int32_t window_log_max; /* ZstdOptions::window_log, src/decoder/zstd.rs:22-47; 0 = default */
    int32_t device;         /* HIP device ordinal, -1 = current */
} chip_decoder_opts;

/* Interface::zlib_ng(mode) src/decoder/zlib_ng.rs:61-90 / Interface::zstd(opts)
 * src/decoder/zstd.rs:81-94.  NULL on failure (the Rust side maps NULL to None). */
chip_decoder *chip_decoder_new(int format, const chip_decoder_opts *opts);
/* decode_fn: src/decoder/zlib_ng.rs:94-96 (+ macro src/decoder/mod.rs:459-486),
 * src/decoder/zstd.rs:98-136.  `in`/`out` are host pointers borrowed for the call only.
 * Limits: at most 256 MiB of compressed input may be BUFFERED (input behind the last deflate block boundary, or of
 * one zstd frame) and 4 GiB - 16 of decoded output held; a call that would cross them fails with err = -4
 * (Z_MEM_ERROR) instead of looping.  The calling thread's current HIP device is left as it was. */
chip_decode_result chip_decode(chip_decoder *d, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len);
/* reset_fn: src/decoder/zlib_ng.rs:99-108, src/decoder/zstd.rs:139-148.  Returns the instance
 * to keep using (compu replaces its pointer with the returned one, src/decoder/mod.rs:433-441). */
chip_decoder *chip_decoder_reset(chip_decoder *d);
/* drop_fn: src/decoder/zlib_ng.rs:111-115, src/decoder/zstd.rs:151-156 */
void chip_decoder_free(chip_decoder *d);
/* Memory a streaming decoder holds right now: pinned host bytes (buffered input) and device bytes (input copy, decoded
 * output not yet handed on + the 32 KiB window, checkpoint).  An inflate stream keeps O(window + piece) whatever its
 * length: input in front of the last block boundary and output that has been handed on are dropped between calls (the
 * reference's state is ~40 KiB per decoder, src/decoder/zlib_ng.rs:29-55).  A zstd stream keeps O(frame window + piece)
 * the same way (ZSTD_decompressStream's own buffers, src/decoder/zstd.rs:98-136): the block checkpoint carries the running
 * XXH64, output behind the window is dropped; a single-segment frame's window is its content size.  The inflate kernel's
 * token scratch (64 KiB per streaming decoder) is not included.  A brotli stream keeps O(window + piece) the same way (checkpoint
 * at every metablock boundary); its count includes the kernel's table slots of the decoder's stream, one 128 KiB slot and one
 * worst-case slot of about 1.4 MB, which chip_decoder_free() releases. */
void chip_decoder_footprint(const chip_decoder *d, size_t *pinned_bytes, size_t *device_bytes);
/* describe_error_fn: src/decoder/zlib_ng.rs:118-123 (zError), src/decoder/zstd.rs:159-164
 * (ZSTD_getErrorName).  Never NULL for code 0 (tests/decoder.rs:74-76). */
const char *chip_decoder_strerror(int format, int32_t code);

/* ---- batched decode: the hot path (additive API) -------------------------- */

/*
 * Decode n independent units in one launch, one wavefront per unit.  Every pointer is a DEVICE
 * pointer.  Unit i reads in_base[in_off[i] .. +in_len[i]) and writes out_base[out_off[i] ..
 * +out_cap[i]).  Results per unit:
 *   out_len[i]  bytes written
 *   in_used[i]  bytes of input consumed (trailing bytes after the stream are not counted)
 *   status[i]   CHIP_FINISHED / CHIP_NEED_INPUT (stream truncated) / CHIP_NEED_OUTPUT (out_cap too
 *               small) / CHIP_NEED_DICT, or a negative codec error with the meaning of DecodeError
 *               (zlib: -3 data error; zstd: -(ZSTD_ErrorCode), e.g. -20 corruption, -22 checksum)
 * For CHIP_FMT_ZSTD: on CHIP_NEED_OUTPUT out_len counts whole blocks only, and the unit's range up to
 * out_cap[i] may be used as scratch (regenerated literals are parked at its end while a block decodes).
 * A block is decoded in the unit's own range, so one that does not fit is CHIP_NEED_OUTPUT at the point
 * where the room ends -- also when damage lies further on in that block, which libzstd (decoding in a buffer of
 * its own) would report instead; with room for the frame the verdicts are the same.  A match offset beyond the
 * frame's Window_Size is -20 even where the bytes exist (RFC 8878 3.1.1.1.2): the verdict never depends on
 * how much history a streaming caller's decoder still holds.
 * For CHIP_FMT_BROTLI: status[i] is CHIP_FINISHED, CHIP_NEED_INPUT (truncated), CHIP_NEED_OUTPUT, or a negative
 * BrotliDecoderErrorCode (compu's DecodeError(code), src/decoder/brotli_c.rs:50-59).  On CHIP_NEED_OUTPUT out_len[i] ==
 * out_cap[i] and those are the stream's first out_cap[i] bytes.  With room for the output the verdict, the output and the code
 * are libbrotlidec's; on an error out_len[i] counts the bytes decoded in front of it (libbrotlidec flushes fewer).  Exceptions:
 * a unit that runs 2^24 commands of a single block type in one metablock without output is -31 (UNREACHABLE) where
 * libbrotlidec keeps going; a unit longer than 512 MiB - 64 reads as truncated.  CHIP_F_COMPU_STATUS changes nothing for brotli.
 * in_base must be 4-byte aligned and its allocation padded to a multiple of 4 bytes.
 * `format` is one CHIP_FMT_* for the whole batch.  `stream` is a hipStream_t (NULL = default
 * stream); the call only enqueues work.  Returns CHIP_OK or a CHIP_E_* code.
 * Replaces, per unit, the loop  Interface::zlib_ng(mode) -> decode -> reset
 * (src/decoder/zlib_ng.rs:61-108, src/decoder/mod.rs:459-486).
 */
int chip_decode_batch(int format, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                      void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                      uint32_t *in_used, int32_t *status, void *stream);

/*
 * The same with options.  CHIP_F_COMPU_STATUS: status[i] is what compu's decode_fn would have returned for the unit, to the
 * letter, where the default names the cause instead --
 *   deflate / zlib / gzip (src/decoder/mod.rs:475-483): zlib's Z_OK with avail_in == 0 is NeedInput even when it was the
 *     output that filled (in_used[i] is then zlib's count: every bit of the token during which the room ran out, rounded up
 *     to a byte), and a unit without any input is NeedOutput (zlib's Z_BUF_ERROR);
 *   zstd (src/decoder/zstd.rs:121-133): compu compares output.pos with output.size before it looks at the return value -- a
 *     truncated frame whose bytes so far fill out_cap[i] exactly is NeedOutput; an error stays the error, also behind blocks
 *     that fill out_cap[i] exactly (ZSTD_decompressStream returns an error before it writes output.pos, so compu sees 0),
 *     except for an empty output range (0 == 0: NeedOutput).
 * Everything else is identical.  Unknown flag bits: CHIP_E_INVALID.
 *
 * CHIP_F_MEMBERS: a unit is a SERIES of gzip members (RFC 1952 sec. 2.2: WARC / Common Crawl records, `cat a.gz b.gz`) or of
 * zstd frames and skippable frames (RFC 8878 sec. 3.1: pzstd output, seekable files), decoded one behind the other by the wave
 * that owns the unit, as gzip -d and ZSTD_decompress do.  For CHIP_FMT_GZIP, CHIP_FMT_AUTO, CHIP_FMT_ZSTD and CHIP_FMT_DETECT (routed:
 * gzip / zlib units and zstd units each go to their member kernel, units that are neither are answered as without the flag).
 * CHIP_E_INVALID, before the device is looked for, with CHIP_FMT_DEFLATE, CHIP_FMT_ZLIB and CHIP_FMT_BROTLI (no concatenation
 * convention), with the LZ4 tags (concatenated frames are the caller's loop), with the Snappy tags and together with CHIP_F_COMPU_STATUS (compu has
 * no multi-member decode to mirror).  No reference counterpart, and
 * batch only: the streaming decoders do not take it (compu's caller sees Finished, calls reset and goes on), nor do
 * chip_decode_batch_host / _multi, which have no flags word.
 * The contract.  decode1(p, room) is what a unit without the flag answers for the input in[p .. len) and `room` bytes of output:
 * (st, out_len, in_used).  With the flag a unit of `len` bytes and out_cap `cap` answers
 *
 *   p = 0; total = 0
 *   loop:
 *     (st, ol, iu) = decode1(p, cap - total)          # size pass: no room limit, 64-bit total
 *     total += ol
 *     if st != CHIP_FINISHED:
 *         status = st; out_len = total
 *         in_used = (st == CHIP_NEED_INPUT) ? len : p + iu
 *         stop
 *     p += iu
 *     if another member starts at p: continue
 *     status = CHIP_FINISHED; out_len = total; in_used = p; stop
 *
 * "Another member starts at p", only behind a unit of the same family --
 *   gzip: the member just finished was gzip (not zlib under CHIP_FMT_AUTO / CHIP_FMT_DETECT), len - p >= 2 and the bytes at p
 *     are 1f 8b;
 *   zstd: len - p >= 4 and the LE32 at p is 0xFD2FB528 or 0x184D2A50 .. 0x184D2A5F.
 * Anything else behind a finished member is trailing bytes, not counted in in_used, as without the flag: zero padding, a lone
 * 1f, fewer than 4 bytes behind a zstd frame.  Once a member is started its verdict is the unit's: 1f 8b followed by nothing is
 * CHIP_NEED_INPUT, 1f 8b 07 ... is -3, a wrong CRC in member 3 is -3 with out_len = members 1 and 2 plus what member 3 decoded
 * (out_len counts the bytes in front of the error, as ever).  It follows that
 *   - a match distance never reaches in front of its own member's first byte: gzip -3 ("invalid distance too far back"), zstd
 *     -20, although the previous member's bytes lie right there in the output;
 *   - CRC-32 / ISIZE and XXH64 / Frame_Content_Size are checked per member, over that member's bytes only;
 *   - zstd's "on CHIP_NEED_OUTPUT out_len counts whole blocks only" applies to the frame that ran out of room; earlier frames
 *     count in full;
 *   - a unit made only of skippable frames is CHIP_FINISHED with out_len 0;
 *   - in_len == 0 answers as without the flag, and a single-member unit answers the same with and without it.
 * The loop ends: a started gzip member consumes at least 18 bytes, a started zstd frame at least 8, or the unit ends.
 */
enum { CHIP_F_COMPU_STATUS = 1 };
enum { CHIP_F_MEMBERS = 2 };
int chip_decode_batch_ex(int format, uint32_t flags, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                         void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                         uint32_t *in_used, int32_t *status, void *stream);

/*
 * The size pass: the decoded length of every unit, without decoding it.  chip_decode_batch wants an out_cap[i] and an output
 * range per unit, and the formats do not say how much a unit decodes to (raw deflate and zlib carry no length, gzip's ISIZE is
 * modulo 2^32 and sits behind the data).  This call takes the same input description (DEVICE pointers, in_base 4-byte aligned
 * and padded as for chip_decode_batch, enqueue-only on `stream`), no output buffer at all, and answers per unit
 *   out_size[i]  decoded length in bytes, 64-bit: a unit may decode to more than an out_cap can express
 *   in_used[i]   bytes of input consumed, as chip_decode_batch
 *   status[i]    as chip_decode_batch; never CHIP_NEED_OUTPUT
 * `flags` is 0 or CHIP_F_MEMBERS (anything else, CHIP_F_COMPU_STATUS included: CHIP_E_INVALID).  With CHIP_F_MEMBERS (formats as
 * for chip_decode_batch_ex) a unit is a series of members and the four rules below hold per unit, measured against the decode
 * with the same flag; out_size[i] is the series' total and may exceed 2^32.
 * `format`: CHIP_FMT_DEFLATE, CHIP_FMT_ZLIB, CHIP_FMT_GZIP, CHIP_FMT_AUTO, CHIP_FMT_ZSTD (window_log_max: the default, as
 * chip_decode_batch), and CHIP_FMT_DETECT, routed exactly as a CHIP_FMT_DETECT decode batch is (units that are neither get
 * CHIP_UNKNOWN_FORMAT / CHIP_NEED_INPUT), and CHIP_FMT_LZ4_BLOCK / CHIP_FMT_LZ4 and CHIP_FMT_SNAPPY_BLOCK / CHIP_FMT_SNAPPY (flags 0 only; "LZ4: blocks and frames" and
 * "Snappy: blocks and framed streams" below say what the pass checks).  CHIP_FMT_BROTLI is CHIP_E_INVALID: brotli's literal context is the two previous
 * BYTES, so a brotli size pass is a full decode (it would decode into a ring) -- a different design.  Arguments are checked
 * before the device is looked for (as chip_decode_batch_ex does).
 * The contract:
 *  1. Exact on valid streams.  If chip_decode_batch with enough room answers CHIP_FINISHED for a unit, so does the size pass,
 *     with out_size[i] = that decode's out_len[i] and in_used[i] = its in_used[i].
 *  2. The same verdict wherever the verdict does not need decoded bytes.  Every check the decoder makes is made -- wrapper header
 *     fields, code-length verdicts in zlib's order, invalid codes, "invalid distance too far back" (positions in front of the
 *     unit's first byte included), stored LEN / NLEN, CHIP_NEED_DICT, truncation (CHIP_NEED_INPUT), gzip's ISIZE against the
 *     counted length -- except the Adler-32 / CRC-32 comparison (a gzip unit whose CRC is wrong AND whose ISIZE is cut or wrong
 *     therefore reads CHIP_NEED_INPUT / a length error here, where the decoder meets the CRC first).  zstd: frame and block
 *     headers, literals and sequence section headers, Huffman tree and FSE table descriptions, the sequence bitstream, offsets
 *     against window and position, Frame_Content_Size against the counted length, window_log_max -- except the CONTENTS of
 *     Huffman-coded literal streams (skipped by their stated size; a stream of stated size 0 or with a zero last byte is
 *     content too, and not seen) and the XXH64 comparison.  A frame with Frame_Content_Size
 *     is still walked: the header is not trusted.  On an error or CHIP_NEED_INPUT out_size[i] is the length
 *     counted in front of it (as out_len is) and in_used[i] is what chip_decode_batch (flags 0) reports with ample room.
 *  3. Enough room.  Decoding a unit with out_cap[i] = out_size[i] never answers CHIP_NEED_OUTPUT when the size pass said
 *     CHIP_FINISHED, damaged payload or not.
 *  4. A unit whose only fault is one the size pass cannot see (a wrong check value, a damaged Huffman literal stream) is CHIP_FINISHED here and an error
 *     in the decode that follows: the price of not producing the bytes.
 * No per-unit device memory: the pass uses the inflate kernel's token scratch of (device, stream) -- one slot per resident wave,
 * shared with chip_decode_batch on that stream, released by chip_trim() -- and, routed, that slot's index lists; zstd needs none.
 * No reference counterpart: compu's decode_vec grows a Vec as it goes (src/decoder/mod.rs:323-335); this replaces the
 * guess / CHIP_NEED_OUTPUT / decode-again loop a batch caller would write around it.
 */
int chip_decode_batch_sizes(int format, uint32_t flags, size_t n, const void *in_base, const uint64_t *in_off,
                            const uint32_t *in_len, uint64_t *out_size, uint32_t *in_used, int32_t *status, void *stream);

/*
 * The same for data that starts and ends in HOST memory (SURVEY.md sec. 8b "pinned-host variant", 8e): every
 * pointer is a host pointer (hipHostMalloc / chip_pinned_alloc memory lets the copies run asynchronously; pageable
 * memory works but serialises them).  The units are cut into slices (about `slice_bytes` of input + output each,
 * 0 = 256 MiB); slices alternate between two HIP streams, each running H2D -> kernel -> D2H for its slice, so the
 * copies of one slice overlap the kernel of the other.  Offsets are relative to in_base / out_base as in
 * chip_decode_batch.  A slice whose units lie back to back in index order (the usual layout; up to 15 bytes of
 * padding between units) moves straight between the caller's memory and the device; any other layout (gaps, reverse
 * order, overlapping ranges) is packed through pinned staging buffers.  Exactly out_len[i] bytes are written at
 * out_off[i]; nothing else in out_base is touched.  Returns when everything has arrived in host memory; the
 * calling thread's current device is left as it was.  Streams and buffers are kept per device between calls
 * (chip_trim() releases them).
 * No reference counterpart: compu's decode loop is the host-memory path (src/decoder/mod.rs:323-335).
 */
int chip_decode_batch_host(int format, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                           void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                           uint32_t *in_used, int32_t *status, int device, size_t slice_bytes);

/*
 * chip_decode_batch_host over several GPUs of the node (independent units, no exchange step, no
 * collective).  `devices[0 .. n_devices)` are HIP device ordinals (NULL / 0 = every visible device).  The units are
 * partitioned on the host into one contiguous index range per device, balanced by input + output bytes; a
 * CHIP_FMT_DETECT batch is first bucketed by Detection::detect (src/decoder/mod.rs:28-114) so that every launch is
 * homogeneous (gzip/zlib units to the inflate kernel, zstd frames to the zstd kernel; units that are neither are
 * answered on the host).  Each device is driven by a host thread of its own (hipSetDevice is per thread) with two
 * streams, as above; results land in the caller's per-unit arrays.  Returns the first failure of any device.
 */
int chip_decode_batch_multi(int format, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                            void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                            uint32_t *in_used, int32_t *status, const int *devices, int n_devices, size_t slice_bytes);

/* The host-side partition chip_decode_batch_multi uses: cuts[0 .. parts] with cuts[0] = 0 and
 * cuts[parts] = n; worker w owns units [cuts[w], cuts[w+1]), contiguous and balanced by in_len + out_cap bytes.
 * Pure host arithmetic (no device needed). */
int chip_partition_units(size_t n, const uint32_t *in_len, const uint32_t *out_cap, int parts, size_t *cuts);

/* Detection::detect src/decoder/mod.rs:28-114 on the first bytes of each unit; kind[i] gets a
 * CHIP_DETECT_* value.  Host form and batched device form. */
int chip_detect(const uint8_t *bytes, size_t len);
int chip_detect_batch(size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, int32_t *kind,
                      void *stream);

/* ---- BGZF: from a file to a batch (additive API) ------------------------- */

/*
 * BGZF (the blocked gzip of BAM, BCF, tabix-indexed VCF and bgzip; SAM specification sec. 4.1) is a concatenation of gzip
 * members of at most 64 KiB, compressed and decoded, each stating its own compressed size: exactly the batch of independent
 * units chip_decode_batch wants.  These calls turn a BGZF buffer into that call's four arrays.
 * A block at byte p has the 18-byte header htslib writes:  1f 8b 08 04 | MTIME (4) XFL OS, any value | 06 00 (XLEN 6) |
 * 42 43 02 00 ('B' 'C', SLEN 2) | BSIZE (u16 LE).  It is BSIZE + 1 bytes long and ISIZE is the u32 LE in its last 4 bytes.
 * LIMIT: the BC subfield must be the only one.  A block whose extra field holds other subfields as well is valid by the SAM
 * specification and CHIP_BGZF_BAD_HEADER here (no known writer emits one).  Such a file still decodes: its blocks are gzip
 * members, which chip_gzip_plan (below) plans by the size pass instead of BSIZE, or as ONE CHIP_FMT_GZIP unit with CHIP_F_MEMBERS
 * (chip_decode_batch_ex), one wave walking its members, within the 512 MiB limit of a unit's input.
 * The plan of `len` bytes is defined by this walk:
 *   p = 0, n = 0, total = 0
 *   loop: p == len -> OK;  len - p < 18 -> TRUNCATED;  header bytes wrong -> BAD_HEADER;
 *         bs = BSIZE + 1;  bs < 28 -> BAD_HEADER (18 + the 2-byte empty deflate stream + 8);  p + bs > len -> TRUNCATED;
 *         isize = LE32(p + bs - 4);  isize > 65536 -> BAD_HEADER;
 *         block n: in_off = p, in_len = bs, out_off = total, out_cap = isize;  n++, total += isize, p += bs
 * summary: n_blocks = n and total_out = total of the WHOLE walk, in_used = p where it stopped, status why, eof = 1 when the last
 * block has ISIZE 0 (htslib's EOF marker is such a block).  Blocks with ISIZE 0 are units like any other (out_cap 0): indices
 * are the file's block numbers.  The arrays receive the first min(n_blocks, max_blocks) blocks and nothing behind them is
 * written: max_blocks = 0 with null arrays counts, a second call fills.  in_off is relative to the buffer and out_off starts at
 * 0, so the arrays go unchanged to chip_decode_batch(CHIP_FMT_GZIP, n_blocks, in_base, in_off, in_len, out, out_off, out_cap, ..).
 * CHIP_E_INVALID, checked before the device is looked for: summary NULL, a NULL buffer with len > 0, NULL arrays with
 * max_blocks > 0 (chip_bgzf_plan: in_base not 4-byte aligned, len > 2^40).  len == 0 is CHIP_OK with an all-zero summary.
 * No reference counterpart: compu has no container formats.
 */
enum { CHIP_BGZF_OK = 0, CHIP_BGZF_TRUNCATED = 1, CHIP_BGZF_BAD_HEADER = 2 };
typedef struct {
    uint64_t n_blocks, total_out, in_used;
    int32_t status;
    uint32_t eof;
} chip_bgzf_summary;

/* The walk itself on HOST memory: pure host arithmetic, no device needed (as chip_partition_units).  Its arrays are what
 * chip_decode_batch_host / chip_decode_batch_multi take. */
int chip_bgzf_plan_host(const uint8_t *in, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                        uint32_t *out_cap, chip_bgzf_summary *summary);

/* The same answer for a buffer in DEVICE memory, without one dependent memory round trip per block: in_base and the four arrays
 * are DEVICE pointers, summary is a HOST pointer.  in_base as for chip_decode_batch (4-byte aligned, allocation padded to a
 * multiple of 4 bytes); len is arbitrary.  SYNCHRONOUS on `stream` (n_blocks is a host argument of the decode that follows): it
 * returns when the arrays are in device memory and *summary is filled, and waits once in between to size its scratch by the
 * number of header candidates.  Scratch per (device, stream), kept between calls and released by chip_trim(): 16 bytes per
 * 16 KiB of input and 36 + 4 * ceil(log2(candidates + 1)) bytes per candidate (about 7 MB for 65 536 blocks).  More than 2^31 - 1
 * candidates: CHIP_E_NOMEM.  The calling thread's current device is left as it was. */
int chip_bgzf_plan(const void *in_base, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                   uint32_t *out_cap, chip_bgzf_summary *summary, void *stream);

/* htslib's 28-byte EOF marker (an empty BGZF block); *len gets 28 (len may be NULL).  Static storage. */
const uint8_t *chip_bgzf_eof_block(size_t *len);

/* ---- zstd frames: from a file to a batch (additive API) ------------------- */

/*
 * A zstd file may hold many frames (RFC 8878 sec. 3.1: pzstd output, the seekable format, one frame per chunk, `cat a.zst b.zst`),
 * with skippable frames among them.  Where a frame ends is found without decoding anything: from its header and the 3-byte header
 * of each block; with Frame_Content_Size the frame also states how much room it needs.  These calls turn such a buffer into the
 * four arrays of chip_decode_batch(CHIP_FMT_ZSTD, ..), one unit and so one wave per frame, where the same buffer as ONE unit with
 * CHIP_F_MEMBERS is decoded by a single wave.  All integers are little endian.
 * The plan of `len` bytes is defined by this walk:
 *   p = 0; n = 0; skipped = 0; unsized = 0; total = 0
 *   loop:
 *     p == len            -> OK
 *     len - p < 4         -> TRUNCATED
 *     m = LE32(p)
 *     m in 0x184D2A50 .. 0x184D2A5F (skippable frame):
 *         len - p < 8 -> TRUNCATED;  s = LE32(p + 4);  s > len - p - 8 -> TRUNCATED
 *         skipped++;  p += 8 + s;  continue                 (no unit: indices count data frames only)
 *     m != 0xFD2FB528     -> BAD_HEADER
 *     len - p < 5         -> TRUNCATED
 *     fhd = byte(p + 4);  f = fhd >> 6;  ss = (fhd >> 5) & 1;  d = fhd & 3
 *     hs = 5 + (ss ? 0 : 1) + {0,1,2,4}[d] + (f == 0 ? ss : {-,2,4,8}[f])
 *     len - p < hs        -> TRUNCATED
 *     fcs = absent when f == 0 and ss == 0, else the field's value (the 2-byte form + 256)
 *     q = p + hs;  blocks = 0
 *     per block:  len - q < 3 -> TRUNCATED;  h = LE24(q);  type = (h >> 1) & 3;  type == 3 -> BAD_HEADER
 *                 ++blocks > CHIP_ZPLAN_MAX_BLOCKS -> TOO_LARGE
 *                 body = (type == 1) ? 1 : h >> 3;  body > len - q - 3 -> TRUNCATED
 *                 q += 3 + body;  stop after the block with h & 1
 *     fhd & 4 (checksum):  len - q < 4 -> TRUNCATED;  q += 4
 *     q - p > 2^32 - 1, or fcs present and fcs >= 0xFFFFFFFF  -> TOO_LARGE
 *     frame n:  in_off = p, in_len = q - p, out_off = total,
 *               out_cap = fcs, or CHIP_ZPLAN_UNSIZED (adds 0 to total, unsized++)
 *     n++;  total += fcs or 0;  p = q
 * summary: n_frames = n, n_skippable = skipped, n_unsized = unsized and total_out = total of the WHOLE walk, status why it
 * stopped, in_used = the p of the frame (or skippable frame) where it stopped -- not q: a frame that is cut or refused is not
 * consumed.  The plan judges only what it needs to find lengths.  The reserved bit of the frame header descriptor, the window
 * descriptor, the dictionary ID, Block_Maximum_Size, the content of the blocks and Frame_Content_Size against what the blocks
 * decode to are the business of the decode that follows, as they are today.  The block cap belongs to the definition (host and
 * device): a frame of legal empty raw blocks would otherwise keep a single GPU lane hopping for minutes, and at the block sizes
 * libzstd writes 2^20 blocks are far beyond the 4 GiB in_len can express.
 * The arrays receive the first min(n_frames, max_frames) frames and nothing behind them is written: max_frames = 0 with null
 * arrays counts, a second call fills.  in_off is relative to the buffer and out_off starts at 0, so with n_unsized == 0 the
 * arrays go unchanged to chip_decode_batch(CHIP_FMT_ZSTD, n_frames, in_base, in_off, in_len, out, out_off, out_cap, ..).  With
 * unsized frames: chip_decode_batch_sizes over in_off / in_len, then chip_layout_units, then the decode.
 * CHIP_E_INVALID, checked before the device is looked for: summary NULL, a NULL buffer with len > 0, NULL arrays with
 * max_frames > 0 (chip_zstd_plan: in_base not 4-byte aligned, len > 2^40).  len == 0 is CHIP_OK with an all-zero summary.
 * No reference counterpart: compu has no container formats.
 */
enum { CHIP_ZPLAN_OK = 0, CHIP_ZPLAN_TRUNCATED = 1, CHIP_ZPLAN_BAD_HEADER = 2, CHIP_ZPLAN_TOO_LARGE = 3 };
#define CHIP_ZPLAN_UNSIZED 0xFFFFFFFFu   /* out_cap of a frame without Frame_Content_Size */
#define CHIP_ZPLAN_MAX_BLOCKS (1u << 20) /* blocks per frame the walk follows */
typedef struct {
    uint64_t n_frames, n_skippable, n_unsized, total_out, in_used;
    int32_t status;
    uint32_t pad;
} chip_zstd_plan_summary;

/* The walk itself on HOST memory: pure host arithmetic, no device needed.  Its arrays are what chip_decode_batch_host /
 * chip_decode_batch_multi take. */
int chip_zstd_plan_host(const uint8_t *in, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                        uint32_t *out_cap, chip_zstd_plan_summary *summary);

/* The same answer for a buffer in DEVICE memory, with the conventions of chip_bgzf_plan: in_base and the four arrays are DEVICE
 * pointers, summary is a HOST pointer; in_base 4-byte aligned, its allocation padded to a multiple of 4 bytes; len is arbitrary.
 * SYNCHRONOUS on `stream`: it returns when the arrays are in device memory and *summary is filled, and waits once in between to
 * size its scratch by the number of magic-number candidates.  Scratch per (device, stream), a launch slot of its own, kept between
 * calls and released by chip_trim(): 16 bytes per 16 KiB of input and 60 + 4 * ceil(log2(candidates + 1)) bytes per candidate.
 * More than 2^31 - 1 candidates: CHIP_E_NOMEM.  Input that changes during the call: CHIP_E_LAUNCH, nothing is written out of
 * range.  The calling thread's current device is left as it was. */
int chip_zstd_plan(const void *in_base, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                   uint32_t *out_cap, chip_zstd_plan_summary *summary, void *stream);

/* The step between chip_decode_batch_sizes and chip_decode_batch, on the device: out_size (the size pass's answer), out_off and
 * out_cap are DEVICE arrays of n entries; out_off[i] = the exclusive 64-bit sum of out_size[0 .. i), out_cap[i] =
 * min(out_size[i], 0xFFFFFFFF).  total and n_over are HOST pointers: the sum of all sizes, and the number of units with
 * out_size > 0xFFFFFFFF (too large for one unit; their out_cap is clipped).  SYNCHRONOUS on `stream` (the caller allocates
 * `total` bytes next).  out_size and out_off must not be the same array.  n == 0 writes *total = *n_over = 0 without touching the
 * device.  CHIP_E_INVALID before the device is looked for: total or n_over NULL, a NULL array with n > 0, n > 2^32 - 1.  Scratch:
 * 8 bytes per 1024 units in the slot of chip_zstd_plan.  Without it a caller holding frames with no Frame_Content_Size, or gzip
 * units after a size pass, copies n sizes to the host and n offsets back.  No reference counterpart. */
int chip_layout_units(size_t n, const uint64_t *out_size, uint64_t *out_off, uint32_t *out_cap, uint64_t *total, uint64_t *n_over,
                      void *stream);

/* ---- one zstd frame: its blocks and their table sources (additive API) ----- */

/*
 * The plain `big.zst` is ONE frame of many blocks.  A block states its size in its 3-byte header, so where every block lies is
 * found by the hop chip_zstd_plan makes, and what a block needs from the blocks in front of it -- the Huffman literal table a
 * Treeless_Literals_Block reuses, the FSE tables Repeat_Mode reuses -- is stated in its section headers.  These calls describe the
 * blocks of the FIRST frame of a buffer from headers alone: nothing is decoded.  It is the first pass of decoding one frame with a
 * wave per block (sec. 4.19), and a cheap answer to "which blocks stand alone".  All integers are little endian.
 * The walk of `len` bytes:
 *     len < 4             -> TRUNCATED
 *     LE32(0) != 0xFD2FB528 -> BAD_HEADER           (a skippable frame in front is not stepped over)
 *     len < 5             -> TRUNCATED
 *     fhd = byte(4);  f = fhd >> 6;  ss = (fhd >> 5) & 1;  d = fhd & 3
 *     hs = 5 + (ss ? 0 : 1) + {0,1,2,4}[d] + (f == 0 ? ss : {-,2,4,8}[f])
 *     len < hs            -> TRUNCATED
 *     content_size = CHIP_ZBLOCKS_UNSIZED when f == 0 and ss == 0, else the field's value (the 2-byte form + 256)
 *     window_size  = ss ? content_size : (1 << wl) + ((1 << wl) >> 3) * (wd & 7), wd = byte(5), wl = 10 + (wd >> 3)
 *     q = hs;  n = 0
 *     per block:  len - q < 3 -> TRUNCATED;  h = LE24(q);  type = (h >> 1) & 3;  type == 3 -> BAD_HEADER
 *                 n + 1 > CHIP_ZPLAN_MAX_BLOCKS -> TOO_LARGE
 *                 body = (type == 1) ? 1 : h >> 3;  body > len - q - 3 -> TRUNCATED
 *                 block n:  offset = q, size = h >> 3, type, flags = h & 1 (CHIP_ZBLOCK_LAST)
 *                 n++;  q += 3 + body;  stop after the block with h & 1
 *     fhd & 4 (checksum):  len - q < 4 -> TRUNCATED;  q += 4
 *     in_used = q, status OK
 * A walk that stops early keeps the blocks it has counted (header and body present), with in_used = 0: the frame is not
 * consumed.  The reserved bit, the dictionary ID and the window against a limit are for the decode to judge; `descriptor` is fhd
 * and header_bytes is hs, so it can.
 * A compressed block (type 2) is described from its literals section header and its sequences section header (RFC 8878
 * 3.1.1.3.1.1, 3.1.1.3.2.1): lit_type (0 raw, 1 RLE, 2 compressed, 3 treeless), lit_regen (Regenerated_Size), lit_comp (the bytes
 * the literals take behind their header: lit_regen, 1, or Compressed_Size), n_seq (Number_of_Sequences) and mode[3], the
 * compression modes of LL, OF and ML (0 predefined, 1 RLE, 2 FSE, 3 repeat; all 0 when n_seq == 0, which has no modes byte).
 * Where one of these headers reaches beyond the block's body, the block gets CHIP_ZBLOCK_MALFORMED, the fields from there on are
 * 0, and it defines nothing.  Raw and RLE blocks have these fields 0.
 * src[k] of block i is the nearest block j < i that DEFINED the table of kind k, or -1:
 *     CHIP_ZSRC_HUF        a compressed block with lit_type == 2
 *     CHIP_ZSRC_LL/OF/ML   a compressed block with n_seq > 0 whose mode of that kind is not 3 (predefined and RLE define a table;
 *                          a block with no sequences defines nothing)
 * src is filled for every block, whether it reuses a table or not: block i needs src[CHIP_ZSRC_HUF] when lit_type == 3 and
 * src[CHIP_ZSRC_LL + k] when n_seq > 0 and mode[k] == 3, and a -1 there means the frame cannot be decoded.
 * `blocks` receives the first min(n_blocks, max_blocks) blocks and nothing behind them is written: max_blocks = 0 with a NULL
 * array counts, a second call fills.  CHIP_E_INVALID, checked before the device is looked for: summary NULL, a NULL buffer with
 * len > 0, a NULL array with max_blocks > 0 (chip_zstd_blocks: in_base not 4-byte aligned, len > 2^40).
 * The limits are chip_zstd_plan's (the same buffer goes to both): 2^40 bytes, and the alignment chip_zstd_parallel's token pass needs
 * for its dword loads although the walk itself reads bytes; chip_zstd_parallel narrows len to 2^32 - 1.
 * A consumer tests CHIP_ZBLOCK_MALFORMED first: the literals fields of such a block are kept when only the sequences header failed to
 * fit.  The record does not say whether Huffman literals come in one stream or four (Size_Format 0 against 1 to 3 of the first body
 * byte): the token pass parses that header itself.
 * No reference counterpart: compu decodes a frame front to back.
 */
#define CHIP_ZBLOCKS_UNSIZED 0xFFFFFFFFFFFFFFFFull /* content_size of a frame without Frame_Content_Size */
enum { CHIP_ZBLOCK_LAST = 1, CHIP_ZBLOCK_MALFORMED = 2 };
enum { CHIP_ZSRC_HUF = 0, CHIP_ZSRC_LL = 1, CHIP_ZSRC_OF = 2, CHIP_ZSRC_ML = 3 };
typedef struct {
    uint64_t offset;    /* of the 3-byte block header in the buffer */
    uint32_t size;      /* the Block_Size field: the body's bytes (raw, compressed) or the count of an RLE block */
    uint32_t lit_regen, lit_comp, n_seq;
    uint8_t type, flags, lit_type, mode[3], pad[2];
    int32_t src[4];
} chip_zstd_block;
typedef struct {
    uint64_t n_blocks, in_used, content_size, window_size;
    int32_t status;     /* CHIP_ZPLAN_OK, _TRUNCATED, _BAD_HEADER, _TOO_LARGE */
    uint32_t descriptor, header_bytes, pad;
} chip_zstd_blocks_summary;

/* On HOST memory: pure host arithmetic, no device needed. */
int chip_zstd_blocks_host(const uint8_t *in, uint64_t len, uint64_t max_blocks, chip_zstd_block *blocks, chip_zstd_blocks_summary *summary);

/* The same answer for a buffer in DEVICE memory, with the conventions of chip_zstd_plan: in_base and blocks are DEVICE pointers,
 * summary is a HOST pointer; in_base 4-byte aligned, its allocation padded to a multiple of 4 bytes.  One lane hops over the
 * block headers, then one lane per block reads its section headers and one workgroup scans for the sources.  SYNCHRONOUS on
 * `stream`: it waits once behind the hop for the block count and once at the end.  A launch slot of its own (the summary only),
 * released by chip_trim().  The calling thread's current device is left as it was. */
int chip_zstd_blocks(const void *in_base, uint64_t len, uint64_t max_blocks, chip_zstd_block *blocks, chip_zstd_blocks_summary *summary,
                     void *stream);

/*
 * ONE large zstd frame decoded by the whole GPU, with the conventions of chip_inflate_parallel: in_base and
 * out_base are DEVICE pointers, in_base 4-byte aligned and its allocation padded to a multiple of 4; summary is a HOST pointer;
 * SYNCHRONOUS on `stream`; scratch in a launch slot of its own, released by chip_trim(); the calling thread's device is left as it
 * was.  window_log_max as in chip_decoder_opts (0 is 27).  Only the FIRST frame of the buffer is decoded; in_used says where it ended.
 * The passes: chip_zstd_blocks; a token pass, one wave per block, that rebuilds the tables its block reuses from the blocks
 * chip_zstd_blocks names, decodes the literals and stores the sequences with symbolic repeat offsets; the host's prefix sums and
 * carried repeat offsets; one 32-bit word per content byte (a final byte or the position it copies), every offset checked; pointer
 * jumping W[p] = W[W[p]] until no word is left (at most 32 rounds below 2^31 bytes; after CHIP_ZPAR_ROUNDS_MAX the serial path); the
 * bytes, and XXH64 over them on one wave.
 * A CLEAN frame of at least two blocks with total_out <= out_cap: path = CHIP_ZPAR_PARALLEL; the bytes, out_len, in_used and status
 * (CHIP_FINISHED) are those of chip_decode_batch(CHIP_FMT_ZSTD, 1, ..) for that unit.  Clean: the buffer starts with the frame magic;
 * the frame header is accepted (reserved bit, dictionary ID, the window against window_log_max); every block is present and of a
 * legal type; the token pass fails in no block; every table reuse has a source; every offset lies within the content before it and
 * the window; every block decodes to at most Block_Maximum_Size; the blocks add up to Frame_Content_Size where one is stated;
 * total_out < 2^31; the content checksum matches if one is present and not waived.
 * The same with total_out > out_cap: CHIP_NEED_OUTPUT, out_len = 0, total_out the exact size to come back with; nothing is written
 * (the checksum is compared by the call that has the room).
 * Anything else: path = CHIP_ZPAR_SERIAL and the answer is the one-unit batch decode's, which is the arbiter of every verdict -- if
 * the frame fits a unit (out_cap <= 2^32 - 1 and at most 2^28 bytes of input: the first frame's own length where the block walk
 * reaches its end, else len); else path = CHIP_ZPAR_REFUSED and nothing is written.  A clean frame is not bounded by 2^28: a wave of
 * the token pass reads from the earliest block whose table its block reuses to the end of its block, and only that span must stay
 * below 2^28 bytes (a reuse across more is "anything else").
 * CHIP_ZPAR_NO_CHECKSUM: on the parallel path the checksum is read over, not compared (XXH64 is one serial chain: one wave hashes
 * the whole content).  The one deliberate difference from the batch.  summary.check is 0.  Where the checksum is compared the bytes
 * are delivered into scratch, hashed there and copied to out_base only when they match: a mismatch writes nothing before the
 * serial decode does.
 * CHIP_E_INVALID before the device is looked for: summary NULL, a NULL buffer with a length, in_base misaligned, unknown flag bits,
 * len > 2^32 - 1.  The bytes and every summary field except `rounds` are a property of the frame.
 * CHIP_ZPAR_TIMING in the environment (read on every call; a diagnostic): the call waits behind every phase and prints its time on
 * stderr -- describe, tokens, place, each jump round with the words left, deliver, checksum, copy.
 * Scratch: 4 bytes per content byte (5 where the checksum is compared), 12 per sequence, Regenerated_Size + 8 736 per block with Huffman literals, about 140 per block;
 * CHIP_E_NOMEM if it cannot be had.
 */
enum { CHIP_ZPAR_SERIAL = 0, CHIP_ZPAR_PARALLEL = 1, CHIP_ZPAR_REFUSED = 2 };
#define CHIP_ZPAR_NO_CHECKSUM 1u      /* flags: do not verify Content_Checksum */
#define CHIP_ZPAR_ROUNDS_MAX 40
typedef struct {
    uint64_t n_blocks, n_sequences, out_len, in_used, total_out;
    int32_t status;
    uint32_t path, rounds, check;
} chip_zstd_parallel_summary;
int chip_zstd_parallel(const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, int window_log_max, uint32_t flags,
                       chip_zstd_parallel_summary *summary, void *stream);

/*
 * chip_zstd_parallel_next: the NEXT PART of one zstd frame of any length, by the passes of chip_zstd_parallel over a SLAB of it
 * (DESIGN.md sec. 4.20).  The caller owns a CURSOR, plain host data that may be copied and saved (all zero = the beginning of a
 * frame), and beside it `state`, state_cap bytes of DEVICE memory which a copy of the cursor needs a copy of:
 *     [0, CHIP_ZCUR_CARRY_BYTES)   four slots of CHIP_ZCUR_SLOT_BYTES, one per table kind (CHIP_ZSRC_*): the bytes, 3-byte header and
 *                                  body, of the nearest block in front of the cursor that defined the table (cur->carry_len[k] of them)
 *     behind them                  the window, cur->window_size bytes, as a ring: content byte j of the frame lies at j mod window_size
 * in_base is a device pointer to frame byte cur->in_total and len the bytes of the frame that stand there, at most 2^31.  in_base
 * needs no alignment and no padding: the slab is staged behind the carried blocks in scratch.  out_cap is below 2^31.  Positions
 * inside a call are slab-relative, the totals of the cursor are 64-bit: neither bound limits the frame.  window_log_max as in
 * chip_decoder_opts (0 is 27, at most 31); flags: CHIP_ZPAR_NO_CHECKSUM, the same in every call of a frame.  SYNCHRONOUS on `stream`.
 * The header step (phase = CHIP_ZCUR_HEADER) reads the frame header and judges it with the batch decode's codes: the magic (-10), the
 * reserved bit (-14), the window against window_log_max (-16), a dictionary ID other than 0 (-32).  A header that is not whole in the
 * slab is CHIP_NEED_INPUT without progress.  It fills the cursor and moves to CHIP_ZCUR_BLOCKS.  When state_cap is below
 * CHIP_ZCUR_CARRY_BYTES + window_size the call stops there: in_used = the header's bytes, out_len = 0, status = CHIP_NEED_OUTPUT and
 * need_state = the bytes to come back with (a call at phase BLOCKS with too small a state answers the same with in_used = 0; at
 * phase CHECKSUM the state is not read any more and its size is not looked at).
 * Otherwise it goes straight on.
 * Where a call ends: it moves the cursor from a block boundary to a later block boundary, or through the checksum, and delivers
 * exactly the content of the whole blocks between the two at out_base[0 .. out_len); nothing behind out_len is written.  It appends
 * those bytes to the window ring (only the last window_size of a call are moved), copies the nearest definer of each table kind
 * into its carry slot, brings cur->xxh up to out_total, and answers in_used: the next slab begins at in_base + in_used.
 *   - CHIP_FINISHED: the last block and, where the frame has one, the 4 checksum bytes were in the slab; Frame_Content_Size was
 *     compared with out_total in 64 bits and the checksum was compared unless waived.  phase = CHIP_ZCUR_DONE; in_used counts through
 *     the frame and nothing behind it.
 *   - CHIP_NEED_INPUT: everything whole was delivered.  in_used == 0 && out_len == 0: the slab holds no whole block (or not the
 *     whole checksum); come back with a longer slab.  A block cut by the slab's end is dropped and read again by the next call.
 *   - CHIP_NEED_OUTPUT: the next block was whole in the slab and did not fit the room left; need_out is its exact decoded size.
 *   - a negative code: sticky; phase = CHIP_ZCUR_ERROR, cur->error keeps it and every later call answers it.  out_len counts the
 *     whole blocks of true content delivered in front of the failing block.
 * Progress: a slab with one whole block behind the cursor and room for that block's bytes always advances the cursor.
 * There is NO serial path: the passes are a complete decoder for clean blocks, and a block that is not clean is an error with the
 * code of the one-unit batch decode for the same damage: -20 for everything inside a block (the token pass is that kernel's text),
 * for a reserved block type, a block above Block_Maximum_Size, a reuse of a table without a source, an offset beyond the content or
 * the window, and content that does not add up to Frame_Content_Size; -22 for a wrong checksum -- which is found when ALL content
 * has already been delivered: a slabbed decode cannot hold content back as chip_zstd_parallel does.
 * The passes per call: the block walk from the cursor (chip_zstd_slab_blocks_host is its text); the token pass over
 * [carried definers | slab], the carried blocks being replay-only records in front of the slab's; the host's prefix sums from the
 * cursor's repeat offsets, as many leading blocks as fit out_cap; place, where a source in front of the slab's first byte is read
 * from the window ring as a final byte (an offset is legal when off <= hist + position and off <= window_size) and the FIRST block
 * with a bad offset is found; jump and deliver over the blocks in front of it; the window, the carry, the checksum.
 * A wave of the token pass reads one range from the earliest block whose table its block reuses to its block's end; a call takes
 * blocks only while that range stays below 2^28 bytes (the next call has the definer in its carry), and at most
 * CHIP_ZPLAN_MAX_BLOCKS blocks.
 * CHIP_E_INVALID, before a device is looked for: cur, state, summary NULL; in_base NULL with len > 0; out_base NULL with out_cap > 0;
 * len > 2^31; out_cap >= 2^31; unknown flags; window_log_max outside 0..31; a cursor no call has left (an unknown phase,
 * hist != min(out_total, window_size), ring != out_total mod window_size, a carry length above the slot or below 3, xxh.tail_n > 31
 * or xxh.total != out_total of a frame whose checksum is compared, a repeat offset of 0 behind the header); the flag changed
 * mid-frame.  CHIP_E_NOMEM / CHIP_E_LAUNCH: the cursor is as it was, the state may not be: the decode cannot go on.
 * Scratch per (device, stream), in chip_zstd_parallel's launch slot, released by chip_trim(): 4 bytes per byte delivered in the
 * call, 12 per sequence of the slab, Regenerated_Size + 8 736 per block of the slab with Huffman literals, the staged slab and
 * carry, about 200 bytes per block.  It does not depend on the frame's length.
 * CHIP_ZPAR_TIMING as chip_zstd_parallel: walk, tokens, place, each jump round, deliver, checksum, window.
 */
enum { CHIP_ZCUR_HEADER = 0, CHIP_ZCUR_BLOCKS = 1, CHIP_ZCUR_CHECKSUM = 2, CHIP_ZCUR_DONE = 3, CHIP_ZCUR_ERROR = 4 };
#define CHIP_ZCUR_SLOT_BYTES 131088u                          /* Block_Maximum_Size + 3, rounded up to 16 */
#define CHIP_ZCUR_CARRY_BYTES (4u * CHIP_ZCUR_SLOT_BYTES)     /* 524 352 */
/* A running XXH64 (seed 0): the four accumulators, the bytes covered, the bytes behind the last whole 32-byte stripe.  All zero =
 * nothing hashed yet (the accumulators are started by the first update).  One definition for the kernel and the host functions. */
typedef struct {
    uint64_t acc[4];
    uint64_t total;
    uint8_t tail[32];
    uint32_t tail_n, pad;
} chip_xxh64_state;
typedef struct {
    uint64_t in_total;     /* bytes of the frame in front of the next call's first byte */
    uint64_t out_total;    /* bytes delivered so far */
    uint64_t window_size;  /* from the frame header (Single_Segment: the content size) */
    uint64_t content_size; /* Frame_Content_Size, or CHIP_ZBLOCKS_UNSIZED */
    uint64_t hist;         /* valid bytes of the window: min(out_total, window_size) */
    uint64_t ring;         /* where the next content byte goes in the ring: out_total mod window_size */
    uint64_t carry_at[4];  /* frame offset of the carried definer of each kind (orders their replay) */
    uint32_t carry_len[4]; /* its bytes in the slot, header and body; 0 = none */
    uint32_t rep[3];       /* the repeat offsets at the cursor */
    uint32_t phase;        /* CHIP_ZCUR_* */
    uint32_t descriptor;   /* Frame_Header_Descriptor (bit 2: the frame has a checksum) */
    uint32_t waived;       /* 1: the frame is decoded with CHIP_ZPAR_NO_CHECKSUM */
    int32_t error;         /* the sticky status once phase == ERROR */
    uint32_t pad;
    chip_xxh64_state xxh;  /* over out_total bytes (untouched while waived) */
} chip_zstd_cursor;        /* all zero = the beginning of a frame */
typedef struct {
    uint64_t in_used, out_len, need_out, need_state, n_blocks, n_sequences;
    int32_t status; /* why the call stopped */
    uint32_t rounds;
} chip_zstd_next_summary;
int chip_zstd_parallel_next(chip_zstd_cursor *cur, void *state, uint64_t state_cap, const void *in_base, uint64_t len, void *out_base,
                            uint64_t out_cap, int window_log_max, uint32_t flags, chip_zstd_next_summary *summary, void *stream);

/* The host twins of its steps: pure host arithmetic on HOST memory, no device needed.
 * chip_zstd_slab_blocks_host: the walk from a block boundary.  `in` points at a block header, block_max is the frame's
 * Block_Maximum_Size (min(window_size, 131072)).  Per block: len - q < 3 or a body beyond len -> the walk stops, status
 * CHIP_ZPLAN_TRUNCATED (a cut block is never an error); type 3 or Block_Size > block_max -> CHIP_ZPLAN_BAD_HEADER; more than
 * CHIP_ZPLAN_MAX_BLOCKS -> CHIP_ZPLAN_TOO_LARGE; behind the block with the last-block flag: CHIP_ZPLAN_OK, last = 1.  n_blocks counts
 * the whole blocks in front of where it stopped and in_used their bytes, whatever the status.  The records are chip_zstd_blocks_host's
 * with slab-relative offsets; src names the nearest definer INSIDE the slab, -1 where it lies in front of it.
 * chip_zstd_cursor_header_host: the header step on the first `len` bytes of a frame.  Returns CHIP_FINISHED with the cursor filled
 * (phase BLOCKS, in_total = *header_bytes) and *need_state set; CHIP_NEED_INPUT (nothing changed) for a cut header; else the negative
 * code, which it also makes the cursor's sticky error.
 * chip_xxh64_update_host / chip_xxh64_digest_host: the running XXH64 over a chip_xxh64_state; the digest leaves the state usable. */
typedef struct {
    uint64_t n_blocks, in_used;
    int32_t status; /* CHIP_ZPLAN_* */
    uint32_t last;  /* 1: the frame's last block is block n_blocks - 1 */
} chip_zstd_slab_summary;
int chip_zstd_slab_blocks_host(const uint8_t *in, uint64_t len, uint64_t block_max, uint64_t max_blocks, chip_zstd_block *blocks,
                               chip_zstd_slab_summary *summary);
int chip_zstd_cursor_header_host(chip_zstd_cursor *cur, const uint8_t *in, uint64_t len, int window_log_max, uint32_t flags,
                                 uint32_t *header_bytes, uint64_t *need_state);
int chip_xxh64_update_host(chip_xxh64_state *st, const uint8_t *data, uint64_t len);
uint64_t chip_xxh64_digest_host(const chip_xxh64_state *st);

/* ---- gzip members: from a file to a batch (additive API) ------------------- */

/*
 * A gzip file may hold many members (RFC 1952 sec. 2.2: WARC / Common Crawl records, `pigz -i` output, `cat a.gz b.gz`, a BGZF file
 * with foreign subfields, the files chip_encode_file(CHIP_FMT_GZIP) writes).  A member does not state its length: where it ends is
 * known only once its deflate stream has been walked, which is what the size pass (chip_decode_batch_sizes) answers as in_used.
 * This call turns such a buffer into the four arrays of chip_decode_batch(CHIP_FMT_GZIP, ..), one unit and so one wave per member,
 * where the same buffer as ONE unit with CHIP_F_MEMBERS is decoded by a single wave.  The size pass runs over every position that
 * looks like a member's start, all of them at once, one wave each; the members are the chain of those from position 0.
 * The plan of `len` bytes is DEFINED by this walk, in which size1(p, room) is what chip_decode_batch_sizes(CHIP_FMT_GZIP, flags 0)
 * answers for the unit in[p .. p + room): (st, size, iu) = (status, out_size, in_used).
 *   p = 0; n = 0; total = 0
 *   loop:
 *     p == len                 -> OK
 *     len - p < 4              -> TRUNCATED
 *     bytes at p are not 1f 8b 08, or (byte[p + 3] & 0xe0) != 0   -> BAD_HEADER
 *     room = min(len - p, CHIP_GZPLAN_WINDOW)
 *     (st, size, iu) = size1(p, room)
 *     st == CHIP_NEED_INPUT    -> room < len - p ? TOO_LARGE : TRUNCATED
 *     st != CHIP_FINISHED      -> BAD_MEMBER, member_status = st
 *     size > 0xFFFFFFFE        -> TOO_LARGE        (0xFFFFFFFF stays CHIP_ZPLAN_UNSIZED for chip_read_ranges' layout check)
 *     member n: in_off = p, in_len = iu, out_off = total, out_cap = size;  n++; total += size; p += iu
 * summary: n_members = n and total_out = total of the WHOLE walk, status why it stopped, in_used = the p where it stopped: a member
 * that is cut or refused is not consumed.  member_status is the size pass's status of the member at in_used when status is
 * CHIP_GZPLAN_BAD_MEMBER (e.g. -3), else 0.
 * The arrays receive the first min(n_members, max_members) members and nothing behind them is written: max_members = 0 with null
 * arrays counts, a second call fills.  in_off is relative to the buffer and out_off starts at 0, so the arrays go unchanged to
 * chip_decode_batch(CHIP_FMT_GZIP, n_members, in_base, in_off, in_len, out, out_off, out_cap, ..) and to
 * chip_read_ranges(CHIP_FMT_GZIP, ..).
 * Conventions of chip_zstd_plan: in_base and the four arrays are DEVICE pointers, summary is a HOST pointer; in_base 4-byte
 * aligned, its allocation padded to a multiple of 4 bytes; len is arbitrary.  SYNCHRONOUS on `stream`: it returns when the arrays
 * are in device memory and *summary is filled, and waits once in between to size its scratch by the number of candidates.
 * CHIP_E_INVALID, checked before the device is looked for: summary NULL, a NULL buffer with len > 0, NULL arrays with
 * max_members > 0, in_base not 4-byte aligned, len > 2^40.  len == 0 is CHIP_OK with an all-zero summary.  More than 2^31 - 1
 * candidates: CHIP_E_NOMEM.  Input that changes during the call: CHIP_E_LAUNCH, nothing is written out of range.  The calling
 * thread's current device is left as it was.
 * Scratch per (device, stream), a launch slot of its own, kept between calls and released by chip_trim(): 16 bytes per 16 KiB of
 * input and 80 + 4 * ceil(log2(candidates + 1)) bytes per candidate (20 of them the size pass's answers); the size pass itself
 * runs on the inflate slot of that stream, as chip_decode_batch_sizes does.  A candidate is a position whose four bytes are
 * 1f 8b 08 and a FLG without reserved bits: random data holds about one per 128 MiB.
 * What follows from the definition:
 *   - CRC-32.  The size pass makes every check but the CRC-32 comparison.  A member whose only fault is its CRC is a member of the
 *     plan and is -3 in the decode that follows (rule 4 of the size pass); its neighbours decode.
 *   - Trailing bytes.  Bytes behind the last member that are no header (zero padding) stop the plan with BAD_HEADER; the members
 *     in front stay listed and in_used says where.  As chip_bgzf_plan and chip_zstd_plan, and unlike CHIP_F_MEMBERS, which calls
 *     them trailing bytes and answers CHIP_FINISHED.
 *   - 1f 8b 07.  CHIP_F_MEMBERS starts a member at any 1f 8b and answers -3 for 1f 8b 07; the plan answers BAD_HEADER there, and
 *     for a reserved FLG bit.
 *   - No host form.  There is no chip_gzip_plan_host: this library has no CPU inflate, and finding a member's end is an inflate.
 *   - One wave per member.  A file that is ONE huge member still runs on one wave here, and a member of more than CHIP_GZPLAN_WINDOW
 *     input bytes or more than 2^32 - 2 decoded bytes is TOO_LARGE.  This is for files of many members; a file of one large member
 *     is read more than once through its checkpoint index (chip_inflate_index_build, below).
 * No reference counterpart: compu has no container formats.
 */
enum { CHIP_GZPLAN_OK = 0, CHIP_GZPLAN_TRUNCATED = 1, CHIP_GZPLAN_BAD_HEADER = 2, CHIP_GZPLAN_TOO_LARGE = 3, CHIP_GZPLAN_BAD_MEMBER = 4 };
#define CHIP_GZPLAN_WINDOW ((1u << 29) - 64u)  /* input bytes a member may take: the limit of a unit's input */
typedef struct {
    uint64_t n_members, total_out, in_used;
    int32_t status;         /* CHIP_GZPLAN_* */
    int32_t member_status;  /* CHIP_GZPLAN_BAD_MEMBER: the size pass's status of the member at in_used (e.g. -3); else 0 */
} chip_gzip_plan_summary;
int chip_gzip_plan(const void *in_base, uint64_t len, uint64_t max_members, uint64_t *in_off, uint32_t *in_len,
                   uint64_t *out_off, uint32_t *out_cap, chip_gzip_plan_summary *summary, void *stream);

/* ---- ZIP archives: directory plan, entry decode, CRC-32 (additive API) ------ */

/*
 * A ZIP archive (.zip, .npz, .jar, .apk, .docx / .xlsx, .whl, .epub) states in its central directory, per entry, where the data
 * lies, its compressed size, its decoded size and its CRC-32; entries are independent raw-DEFLATE (method 8) or stored (method 0)
 * streams.  chip_zip_plan[_host] turns the directory into an array of chip_zip_entry records, chip_zip_decode decodes, copies and
 * verifies selected entries, chip_crc32_batch is the check on its own.
 * The plan of `len` bytes is DEFINED by this walk (all integers little endian; a status ends the walk):
 *   End record.  Positions p with max(0, len - 22 - 65535) <= p <= len - 22 qualify when the bytes at p are 50 4b 05 06 and
 *     p + 22 + LE16(p + 20) == len: the comment reaches exactly to the end.  The highest qualifying p wins.  None, or len < 22:
 *     CHIP_ZIP_NO_EOCD.  So trailing bytes behind the archive refuse it, and a comment that spells an end record whose length
 *     field reaches the end IS the end record.
 *   ZIP64.  When p >= 20 and the bytes at p - 20 are 50 4b 06 07 (the locator): e = LE64(p - 12) needs e + 56 <= p - 20 and the
 *     bytes 50 4b 06 06 at e, else CHIP_ZIP_BAD_DIRECTORY; n = LE64(e + 32), cd_size = LE64(e + 40), cd_off = LE64(e + 48),
 *     zip64 = 1.  Without a locator n = LE16(p + 10), cd_size = LE32(p + 12), cd_off = LE32(p + 16).
 *   Spanning.  LE16(p + 4) != 0, LE16(p + 6) != 0, LE16(p + 8) != LE16(p + 10); with ZIP64 also LE32(p - 16) != 0 (the locator's
 *     disk), LE32(p - 4) != 1 (its total), LE32(e + 16) != 0, LE32(e + 20) != 0, LE64(e + 24) != n: CHIP_ZIP_UNSUPPORTED.
 *   Bounds.  cd_off + cd_size (formed without wrapping) must not exceed e with ZIP64, p without, and n <= 2^32 - 1; else
 *     CHIP_ZIP_BAD_DIRECTORY.  Offsets are taken as stated: an archive with prepended bytes (a self-extractor) is not re-based.
 *   Directory.  q = cd_off; for i = 0 .. n:
 *     the 46 bytes at q lie inside [cd_off, cd_off + cd_size) and start with 50 4b 01 02, else CHIP_ZIP_BAD_DIRECTORY, bad_index = i
 *     flags = LE16(+8), method = LE16(+10), crc = LE32(+16), csize = LE32(+20), usize = LE32(+24), nlen = LE16(+28),
 *     xlen = LE16(+30), clen = LE16(+32), disk = LE16(+34), lho = LE32(+42)
 *     the record of 46 + nlen + xlen + clen bytes lies inside the directory, else stop as above
 *     the extra field's subfields (id:u16 size:u16 data) are walked; a subfield that reaches out of the extra field ends the chain.
 *       The first subfield with id 1 supplies 64-bit values in this order: usize if it was 0xFFFFFFFF, then csize if it was
 *       0xFFFFFFFF, then lho if it was 0xFFFFFFFF, each from the bytes that lie in both the subfield and the extra field.  A
 *       0xFFFFFFFF field with no value for it: stop as above.  What the chain holds behind the needed values is not looked at
 *       (the 32-bit disk number an id-1 subfield may carry included).
 *     entry i (below); q += 46 + nlen + xlen + clen
 *     What lies in the directory behind the n-th record is not looked at.
 * Entry i is a chip_zip_entry.  status is the first of these that applies:
 *   CHIP_ZIPENT_UNSUPPORTED  disk != 0 (and not 0xFFFF with an id-1 subfield present), or a method other than 0 and 8 (zstd-in-ZIP,
 *                            method 93, included)
 *   CHIP_ZIPENT_ENCRYPTED    flag bit 0, 6 or 13
 *   CHIP_ZIPENT_BAD_LOCAL    the local header: header_off + 30 <= cd_off; the bytes 50 4b 03 04 at header_off;
 *                            data_off = header_off + 30 + LE16(header_off + 26) + LE16(header_off + 28);
 *                            data_off + comp_size <= cd_off (formed without wrapping); method 0 needs comp_size == size.
 *                            If any of these fails data_off is 0 (whatever the status), else it is that sum.
 *   CHIP_ZIPENT_TOO_LARGE    method 8 with comp_size > 2^29 - 64 or size > 2^32 - 2, the limits of a unit.  data_off / comp_size of
 *                            such an entry are what chip_inflate_parallel_next takes with CHIP_FMT_DEFLATE.
 *   CHIP_ZIPENT_OK
 * The local header's own sizes, CRC and name are not looked at: with a data descriptor (flag bit 3) they are zero, the directory
 * is the authority.  The name of entry i is the name_len bytes at name_off, in the directory.
 * summary: n_entries, n_ok and total_size (sum of `size` over the OK entries, modulo 2^64) are those of the WHOLE walk; a walk that
 * stops at entry i keeps entries 0 .. i with n_entries = i.  eocd_off = p, cd_off, cd_size and zip64 as read (0 where the walk
 * stopped before reading them).  The array receives the first min(n_entries, max_entries) records and nothing behind them is
 * written: max_entries = 0 with a NULL array counts, a second call fills.
 * chip_zip_plan: conventions of chip_zstd_plan.  in_base and `entries` are DEVICE pointers, summary is a HOST pointer; in_base
 * 4-byte aligned, its allocation padded to a multiple of 4 bytes; len <= 2^40.  SYNCHRONOUS on `stream`: it waits for the end record,
 * for the number of candidates and at the end.  CHIP_E_INVALID, checked before the device is looked for: summary NULL, a NULL buffer
 * with len > 0, a NULL array with max_entries > 0, in_base not 4-byte aligned, len > 2^40.  len == 0 is CHIP_OK with an all-zero
 * summary except status = CHIP_ZIP_NO_EOCD.  More than 2^31 - 1 candidates: CHIP_E_NOMEM.  Input that changes during the call:
 * CHIP_E_LAUNCH, nothing is written out of range.  A candidate is a position of the directory whose four bytes are 50 4b 01 02.
 * Scratch per (device, stream), a launch slot of its own, kept between calls and released by chip_trim(): 16 bytes per 16 KiB of
 * directory and 36 + 4 * ceil(log2(candidates + 1)) bytes per candidate.
 * No reference counterpart: compu has no container formats.
 */
enum { CHIP_ZIP_OK = 0, CHIP_ZIP_NO_EOCD = 1, CHIP_ZIP_BAD_DIRECTORY = 2, CHIP_ZIP_UNSUPPORTED = 3 };
/* Entry statuses.  All but CHIP_ZIPENT_OK, which chip_zip_decode never writes into its status array, are numbers no decode status
 * has. */
enum {
    CHIP_ZIPENT_OK = 0,
    CHIP_ZIPENT_UNSUPPORTED = 16,
    CHIP_ZIPENT_ENCRYPTED = 17,
    CHIP_ZIPENT_BAD_LOCAL = 18,
    CHIP_ZIPENT_TOO_LARGE = 19,
    CHIP_ZIPENT_BAD_SIZE = 20,  /* chip_zip_decode: the stream finished with another length than `size` */
    CHIP_ZIPENT_BAD_CRC = 21,   /* chip_zip_decode: the bytes' CRC-32 is not the directory's */
    CHIP_ZIPENT_BAD_INDEX = 22  /* chip_zip_decode: sel[k] >= n_entries */
};
typedef struct {       /* 56 bytes, no implicit padding */
    uint64_t header_off; /* the local header offset */
    uint64_t data_off;   /* first byte of the entry's data; 0 when the local header's checks fail */
    uint64_t comp_size;
    uint64_t size;       /* decoded size */
    uint64_t name_off;   /* the name's place in the directory */
    uint32_t crc32;
    uint16_t name_len, method, flags, pad;
    int32_t status;      /* CHIP_ZIPENT_* */
} chip_zip_entry;
typedef struct {
    uint64_t n_entries, n_ok, total_size, cd_off, cd_size, eocd_off, bad_index;
    int32_t status; /* CHIP_ZIP_* */
    int32_t zip64;
} chip_zip_plan_summary;
int chip_zip_plan_host(const uint8_t *in, uint64_t len, uint64_t max_entries, chip_zip_entry *entries, chip_zip_plan_summary *summary);
int chip_zip_plan(const void *in_base, uint64_t len, uint64_t max_entries, chip_zip_entry *entries, chip_zip_plan_summary *summary,
                  void *stream);

/*
 * CRC-32 of many device ranges: crc[i] = the RFC 1952 CRC-32 (zlib's crc32) of base[off[i] .. + len[i]); len[i] == 0 gives 0.  All
 * four arrays and base are DEVICE pointers, off[i] at any alignment.  A range is cut into pieces of CHIP_CRC_PIECE bytes,
 * right-aligned: only the first piece of a range is short.  One wave does each piece; a second kernel folds the pieces of each
 * range on the device, crc = multmodp(x^(8 * CHIP_CRC_PIECE), crc) ^ piece_crc, one wave per range.  So one 4 GiB range and a
 * million 100-byte ranges both fill the card.  The call enqueues on `stream` and waits ONCE in between, for the number of pieces,
 * to size its scratch; the results are in device memory when the stream reaches them, not when the call returns.
 * CHIP_E_INVALID, before the device is looked for: a NULL array or base with n > 0; n > 2^32 - 1.  n == 0: CHIP_OK, the device is
 * not touched.  More than 2^31 - 1 pieces: CHIP_E_NOMEM.  Scratch per (device, stream), a launch slot of its own released by
 * chip_trim(): 16 bytes per range and 4 bytes per piece.
 * No reference counterpart.
 */
#define CHIP_CRC_PIECE 65536u
int chip_crc32_batch(size_t n, const void *base, const uint64_t *off, const uint64_t *len, uint32_t *crc, void *stream);

/*
 * Selected entries of a planned archive, decoded, copied and verified in DEVICE memory.  in_base / len are the archive the plan
 * was made of (alignment and padding as for chip_zip_plan), `entries` the plan's records (DEVICE memory) and n_entries their
 * number; sel is a DEVICE array of n_sel entry indices in any order, repeats allowed; sel NULL means entries 0 .. n_sel in order.
 * out_off (u64) and status (i32) are DEVICE arrays of n_sel entries; summary is a HOST pointer.
 * The records are read as the caller hands them over.  An entry takes part when its record's status is CHIP_ZIPENT_OK and the
 * record passes the checks every load depends on: method 0 or 8, data_off + comp_size <= len, method 0 with comp_size == size,
 * method 8 within a unit's limits; a record with status OK that fails them is CHIP_ZIPENT_BAD_LOCAL.  So no load is out of range,
 * whatever the records hold.
 *   out_off[k]  the exclusive 64-bit sum over the selection of `size` of the entries that take part; every other entry contributes 0
 *   total_out   the sum of them all.  total_out > out_cap: summary status CHIP_READ_NEED_OUTPUT, total_out exact, out_off answered,
 *               status[k] is CHIP_NEED_OUTPUT for an entry that would take part and the verdict below for one that would not,
 *               nothing is decoded and no byte of out_base is written.
 * With enough room (summary status CHIP_READ_OK): the method 8 entries go as one batch to chip_decode_batch(CHIP_FMT_DEFLATE) with
 * in_off = data_off, in_len = comp_size, out_cap = size; the method 0 entries are copied with chip_pack_units' discipline (a
 * destination byte is written once, by a store no wider than the bytes that belong to it); one chip_crc32_batch pass runs over all
 * of them.  status[k] is then
 *   the record's status, or CHIP_ZIPENT_BAD_LOCAL as above, or CHIP_ZIPENT_BAD_INDEX for sel[k] >= n_entries: nothing is written for it
 *   the decode's own status when that is not CHIP_FINISHED: CHIP_NEED_INPUT (the stream is cut), CHIP_NEED_OUTPUT (it holds more
 *     than `size`), -3
 *   CHIP_ZIPENT_BAD_SIZE when it finished with fewer than `size` bytes
 *   CHIP_ZIPENT_BAD_CRC
 *   CHIP_FINISHED: out_base[out_off[k] .. + size) is the entry.
 * The bytes of an entry that is not CHIP_FINISHED are unspecified inside its own range.  Nothing outside out_base[0 .. total_out)
 * is ever written.  summary: n_sel; n_ok the entries that are CHIP_FINISHED, n_bad the others, first_bad the lowest k that is not
 * (0 without one); total_out; status CHIP_READ_OK or CHIP_READ_NEED_OUTPUT.  out_base must not overlap in_base.
 * SYNCHRONOUS on `stream`: it waits once for total_out and the number of deflated entries and once at the end.
 * CHIP_E_INVALID, before the device is looked for: summary NULL; in_base NULL with len > 0, not 4-byte aligned, len > 2^40; entries
 * NULL with n_entries > 0; out_off or status NULL with n_sel > 0; out_base NULL with out_cap > 0; n_entries or n_sel above
 * 2^31 - 1.  n_sel == 0: CHIP_OK, an all-zero summary, the device is not touched.
 * Scratch per (device, stream), a launch slot of its own released by chip_trim(): 112 bytes per selected entry and 4 bytes per
 * CHIP_CRC_PIECE bytes of output; the decode runs on the inflate slot of that stream, as chip_decode_batch does.
 * No reference counterpart.
 */
typedef struct {
    uint64_t n_sel, n_ok, n_bad, first_bad, total_out;
    int32_t status; /* CHIP_READ_OK, CHIP_READ_NEED_OUTPUT */
    int32_t pad;
} chip_zip_decode_summary;
int chip_zip_decode(const void *in_base, uint64_t len, const chip_zip_entry *entries, uint64_t n_entries, uint64_t n_sel,
                    const uint32_t *sel, void *out_base, uint64_t out_cap, uint64_t *out_off, int32_t *status,
                    chip_zip_decode_summary *summary, void *stream);

/* ---- ZIP archives: writing ------------------------------------------------- */

/*
 * The archive chip_zip_plan reads back, made on the device.  Sizes and CRC-32 are known before the first byte is placed, so the
 * archive has no data descriptors: every header states its true sizes and CRC.  Entry i is a chip_zip_source: its content is
 * content[data_off .. + size), its name names[name_off .. + name_len) (any bytes, may be empty), `method` what the caller asks for.
 *   chip_zip_assemble_host  the whole assembly on the host from streams that are already encoded: comp_off (u64) and comp_len (u32)
 *                           give entry i's raw deflate stream inside comp[0 .. comp_all), crc[i] is the CRC-32 of the content.  comp,
 *                           comp_off and comp_len may all be NULL: every entry is then stored.
 *   chip_zip_assemble       the same with every array and buffer in DEVICE memory, summary on the HOST, and a stream: for a caller
 *                           with encoder settings of its own (chip_encode_batch_ex), or one that re-bundles deflated entries of
 *                           another archive without recompressing them (chip_zip_plan's data_off / comp_size / crc32 are its inputs).
 *   chip_zip_write          content to archive in one call: chip_crc32_batch over every entry's content, then
 *                           chip_encode_batch(CHIP_FMT_DEFLATE, level, ..) over the deflate-eligible entries -- method 8 with
 *                           0 < size <= CHIP_ZIPW_DEFLATE_MAX -- each one unit and one wave, into scratch slots of
 *                           up16(chip_encode_bound(CHIP_FMT_DEFLATE, size)) bytes that a kernel lays out with a scan; then the
 *                           assembly of chip_zip_assemble.  level as for chip_encode_batch (-1 .. 9).  in_base is 4-byte aligned and
 *                           its allocation padded to a multiple of 4, as the encoder requires; data_off may have any alignment.
 *   chip_zip_write_bound    content_total + 2 * names_total + 124 * n + 98, or 0 when that overflows 64 bits: always enough, because
 *                           an entry is only written deflated when that is smaller.
 * The archive is DEFINED by these rules (all integers little endian; M32 = 0xFFFFFFFF; FORCE = flags & CHIP_ZW_ZIP64):
 *   Method.  Entry i is written deflated (method 8, c_i = comp_len[i]) when its source asks for 8, a stream is given and
 *     0 < comp_len[i] < size; otherwise stored (method 0, c_i = size).  So an empty entry such as "dir/", an incompressible one, one
 *     above CHIP_ZIPW_DEFLATE_MAX and level 0 (stored blocks never shrink) are all stored.
 *   Local part of entry i at header_off_i; the entries follow each other in order with no gaps, header_off_0 = 0:
 *     50 4b 03 04 | version v_i | gp flags (0x0800 with CHIP_ZW_UTF8, else 0) | method | dos_time | dos_date | crc | csize | usize |
 *     name_len | xlen | the name | the extra field | the data.
 *     zs_i = FORCE || size >= M32 || c_i >= M32.  With zs_i both size fields are M32 and the extra field is
 *     01 00 10 00 LE64(size) LE64(c_i) (20 bytes); without it xlen is 0.
 *   Central record of entry i; the records follow each other from cd_off, the end of the last entry's data:
 *     50 4b 01 02 | made-by v_i | version v_i | the same seven fields as the local header | name_len | xlen | comment length 0 |
 *     disk 0 | internal attributes 0 | external attributes 0 | lho | the name | the extra field.
 *     zl_i = FORCE || header_off_i >= M32.  The extra field is one id-1 subfield holding, in this order, size and c_i (both, when
 *     zs_i) and then header_off_i (when zl_i): 0, 12, 20 or 28 bytes with its 4-byte header.  The fields it replaces are M32.
 *     v_i = 45 when the central record has the subfield, else 20 for method 8 and 10 for method 0; the local header has the same v_i.
 *   End.  z = FORCE || n >= 0xFFFF || cd_size >= M32 || cd_off >= M32.  With z the 56-byte ZIP64 end record comes first:
 *     50 4b 06 06 | LE64 44 | LE16 45 | LE16 45 | LE32 0 | LE32 0 | n | n | cd_size | cd_off; then the 20-byte locator:
 *     50 4b 06 07 | LE32 0 | LE64 the record's offset | LE32 1.  Then the 22-byte end record with min(n, 0xFFFF) twice,
 *     min(cd_size, M32), min(cd_off, M32) and comment length 0; eocd_off is its place, zip64 = z.  n == 0 gives 22 bytes (98 with
 *     FORCE).  There are no data descriptors, comments, timestamp subfields or alignment padding.
 *   entries[i] (may be NULL) is the chip_zip_entry chip_zip_plan produces for entry i of the written archive: header_off, data_off,
 *     comp_size, size, name_off (inside the directory), crc32, name_len, the written method, flags, pad 0, status CHIP_ZIPENT_OK --
 *     CHIP_ZIPENT_TOO_LARGE, as the plan says, for a deflated entry beyond a unit's limits, which only the assemble calls can be
 *     handed.  The caller holds the index of what it wrote without planning it again.
 * summary: n_entries = n, n_deflated the entries written with method 8, out_len, cd_off, cd_size, eocd_off, zip64, status:
 *   CHIP_ZIPW_BAD_SOURCE   bad_index = the LOWEST i whose record fails one of: method not 0 or 8; data_off + size > content_len,
 *                          formed without wrapping; name_off + name_len > names_len, likewise; for an entry that would be written
 *                          deflated in the assemble calls, comp_off + comp_len > comp_all.  Nothing but the summary is written; its
 *                          other fields are 0 except n_entries.
 *   CHIP_ZIPW_NEED_OUTPUT  out_len > out_cap: out_len is exact, entries and the summary are answered, no byte of `out` is written and
 *                          no byte of content / comp is read.  The host form is then pure arithmetic on the records.
 *   CHIP_ZIPW_OK           nothing outside out[0 .. out_len) is written; `out` may have any alignment; every byte is written exactly
 *                          once, by a store that covers only bytes of its own record or range (chip_pack_units' discipline).
 * `out` must not overlap the inputs.
 * CHIP_E_INVALID, before a device is looked for: summary NULL; src NULL with n > 0, names NULL with names_len > 0, content (in_base)
 * NULL with content_len > 0, crc NULL with n > 0; out NULL with out_cap > 0; exactly one or two of the three comp arrays NULL;
 * n > 2^31 - 1; unknown flag bits; level out of range and in_base not 4-byte aligned (chip_zip_write); and arguments that allow an
 * archive of 2^63 bytes or more: content_len >= 2^62, or n * (content_len + 131 194) > 2^63 - 98.
 * n == 0 is answered by the host without touching the device, with or without room: the end records alone, placed with one copy
 * on `stream` that is waited for (chip_zip_assemble_host: written directly).
 * The device calls are SYNCHRONOUS on `stream`.  chip_zip_assemble waits twice: for out_len against the room, and at the end.
 * chip_zip_write waits four times: for the scratch sizes (the slot bytes and the number of deflate-eligible entries), once inside
 * chip_crc32_batch (its pieces), for out_len, and at the end.
 * Scratch per (device, stream), a launch slot of its own released by chip_trim(): 160 bytes per entry for the assembly (and 24
 * bytes per 1024 entries); chip_zip_write adds 84 bytes per entry and the slot area, the sum of up16(chip_encode_bound(CHIP_FMT_DEFLATE, size)) over the
 * deflate-eligible entries -- a little more than their content -- each allocation with a quarter of headroom; the CRC pass and the
 * encoder run on their own slots of that stream.  CHIP_E_NOMEM: the scratch could not be allocated.  CHIP_E_LAUNCH: a launch
 * failed, the inputs changed during the call, or a unit did not end CHIP_ENC_FINISHED (which the slots rule out).
 * No reference counterpart: compu has no container formats.
 */
enum { CHIP_ZIP_STORE = 0, CHIP_ZIP_DEFLATE = 8 };
enum { CHIP_ZW_ZIP64 = 1, CHIP_ZW_UTF8 = 2 };                 /* call flags */
enum { CHIP_ZIPW_OK = 0, CHIP_ZIPW_NEED_OUTPUT = 1, CHIP_ZIPW_BAD_SOURCE = 2 };
#define CHIP_ZIPW_DEFLATE_MAX (1u << 30)                      /* chip_encode_file's unit limit */
typedef struct {            /* 32 bytes, no implicit padding */
    uint64_t data_off, size;          /* the content: content[data_off .. + size) */
    uint64_t name_off;                /* the name: names[name_off .. + name_len), any bytes, may be empty */
    uint16_t name_len, method, dos_time, dos_date;   /* method: what the caller asks for, 0 or 8 */
} chip_zip_source;
typedef struct {            /* 64 bytes */
    uint64_t n_entries, n_deflated, out_len, cd_off, cd_size, eocd_off, bad_index;
    int32_t status, zip64;
} chip_zip_write_summary;
int chip_zip_assemble_host(uint64_t n, const chip_zip_source *src, const uint8_t *names, uint64_t names_len, const uint8_t *content,
                           uint64_t content_len, const uint8_t *comp, uint64_t comp_all, const uint64_t *comp_off, const uint32_t *comp_len,
                           const uint32_t *crc, uint32_t flags, uint8_t *out, uint64_t out_cap, chip_zip_entry *entries,
                           chip_zip_write_summary *summary);
int chip_zip_assemble(uint64_t n, const chip_zip_source *src, const void *names, uint64_t names_len, const void *content,
                      uint64_t content_len, const void *comp, uint64_t comp_all, const uint64_t *comp_off, const uint32_t *comp_len,
                      const uint32_t *crc, uint32_t flags, void *out, uint64_t out_cap, chip_zip_entry *entries,
                      chip_zip_write_summary *summary, void *stream);
int chip_zip_write(int level, uint32_t flags, uint64_t n, const chip_zip_source *src, const void *names, uint64_t names_len,
                   const void *in_base, uint64_t in_len, void *out_base, uint64_t out_cap, chip_zip_entry *entries,
                   chip_zip_write_summary *summary, void *stream);
uint64_t chip_zip_write_bound(uint64_t n, uint64_t names_total, uint64_t content_total);

/* ---- tar archives: the member plan (additive API) --------------------------- */

/*
 * A tar image (what chip_inflate_parallel or chip_zstd_parallel leaves of a .tar.gz / .tar.zst, or a plain .tar) has no directory:
 * every 512-byte header says where the next one is, and a member's content may hold valid headers of its own (a tar in a tar).
 * chip_tar_plan[_host] turns the image into an array of chip_tar_entry records, one per member, in file order.  Nothing is copied:
 * member i's content is in[data_off .. data_off + size), its name in[name_off .. name_off + name_len), behind the prefix
 * in[header_off + 345 .. + prefix_len) and a '/' when prefix_len > 0.  Formats: POSIX ustar, GNU (L / K long names, base-256
 * numbers) and pax (x headers: path, linkpath, size).  Not read: v7 archives without the `ustar` magic, old-GNU and pax sparse
 * members, multi-volume archives.
 *
 * The plan of `len` bytes (any value, not only a multiple of 512) is DEFINED by this walk; all offsets are into the image.
 *   A number field (size, chksum, mode, mtime).  First byte 0x80: the remaining bytes are a big-endian base-256 value, invalid when
 *     it is >= 2^63.  First byte 0xFF: invalid.  Else: leading spaces are skipped, octal digits read, and the byte behind the digits,
 *     if the field has one, must be NUL or space (else invalid); no digits is 0.
 *   is_header(p): p % 512 == 0 and p + 512 <= len; bytes 257..261 are `ustar` (the POSIX magic "ustar\0" and the GNU magic "ustar "
 *     alike); size and chksum are valid; chksum equals the sum of the 512 bytes with bytes 148..155 taken as spaces, the bytes
 *     summed unsigned or signed (both accepted, as Python's tarfile does).
 *   The walk starts at e = 0 and repeats: e == len: stop, CHIP_TAR_OK.  len - e < 512: stop, CHIP_TAR_TRUNCATED.  The 512 bytes at e
 *     all zero: stop, CHIP_TAR_OK, zero_blocks = 2 if the next block lies inside len and is all zero too, else 1; nothing behind
 *     them is looked at.  is_header(e) false: stop, CHIP_TAR_BAD_HEADER.  Else the group at e is read and e becomes its end.
 *   A group is a run of extension headers and the member header they modify.  From q = e, by the typeflag (byte 156) of the header
 *   at q, s its size field:
 *     L, K, x  More than CHIP_TAR_EXT_MAX extension headers in the group or s > CHIP_TAR_EXT_BYTES: CHIP_TAR_UNSUPPORTED, bad_off = q.
 *              q2 = q + 512 + roundup512(s); q2 + 512 > len: CHIP_TAR_TRUNCATED, bad_off = q; is_header(q2) false:
 *              CHIP_TAR_BAD_HEADER, bad_off = q2.  L sets the name to the data in[q + 512 .. + s) up to its first NUL (or all of it),
 *              K the link name likewise.  x holds records "<decimal length> <key>=<value>\n": the length has 1 to 10 digits and a
 *              space behind them, counts the whole record, must end on the record's '\n' inside the data, and the record must hold
 *              a '='; the records fill the s bytes.  Key `path` sets the name, `linkpath` the link name, `size` (1 to 19 decimal
 *              digits) the size; a key that begins with `GNU.sparse.`: CHIP_TAR_UNSUPPORTED, bad_off = q; a malformed record or size
 *              value: CHIP_TAR_BAD_HEADER, bad_off = q (the first record out of order decides).  Other keys (mtime among them) are
 *              not applied.  When two extension headers set the same thing the later one wins.  Continue at q = q2.
 *     g        Legal only with q == e (else CHIP_TAR_BAD_HEADER, bad_off = q): a group of its own, counted in n_global, that ends
 *              at q + 512 + roundup512(s) (above len: CHIP_TAR_TRUNCATED, bad_off = q).  Its records are NOT parsed and NOT
 *              applied to the members behind it.
 *     S, M     CHIP_TAR_UNSUPPORTED, bad_off = q.
 *     else     the member.  size = the pax override, else the field; 0 for the types '1'..'6', which carry no data (tarfile's
 *              rule).  data_off = q + 512, the group ends at data_off + roundup512(size) (above len: CHIP_TAR_TRUNCATED,
 *              bad_off = q).  Without a name override the name is bytes 0..99 up to the first NUL and prefix_len the length of bytes
 *              345..499 up to the first NUL (the full name is prefix + "/" + name, as tarfile builds it); with one prefix_len = 0.
 *              Without a link override the link name is bytes 157..256 up to the first NUL.  flags says where name, link name and
 *              size came from (CHIP_TARF_*: for each the extension header that won; SIZE_BASE256: the field in its base-256 form).
 * A walk that stops keeps the members in front of the stop.  stop_off = the start of the group, or the position, where the walk
 * stopped; bad_off = the offending header (= stop_off unless stated above).  n_entries, n_global and total_size (the sum of the
 * members' sizes) are those of the whole walk whatever max_entries is.
 *
 * chip_tar_plan: conventions of chip_zip_plan.  in_base and `entries` are DEVICE pointers, summary is a HOST pointer; in_base
 * 4-byte aligned and its allocation padded to a multiple of 4 bytes; len <= 2^40 (both forms).  max_entries = 0 with entries NULL
 * only counts.  Nothing is written behind min(n_entries, max_entries) records.  CHIP_E_INVALID (a NULL summary, a NULL buffer with
 * len > 0, a NULL array with max_entries > 0, a misaligned in_base, len > 2^40) is answered before the device is looked for.
 * len == 0: CHIP_OK with an all-zero summary.  More than 2^31 - 1 candidates: CHIP_E_NOMEM.  Input that changes during the call:
 * CHIP_E_LAUNCH, and nothing is written out of range.  SYNCHRONOUS on `stream` (waits twice: the candidate count, the summary).
 * Scratch in a launch slot of its own per (device, stream), released by chip_trim(): 16 bytes per 128 KiB of input, and per
 * candidate -- a 512-aligned position whose bytes 257..261 are `ustar`, headers inside member data included -- 128 + 4 * levels
 * bytes (levels = ceil(log2(candidates + 1))): 72 of them the candidate's record.
 */
enum { CHIP_TAR_OK = 0, CHIP_TAR_TRUNCATED = 1, CHIP_TAR_BAD_HEADER = 2, CHIP_TAR_UNSUPPORTED = 3 };
#define CHIP_TAR_EXT_MAX 16u
#define CHIP_TAR_EXT_BYTES (1u << 20)
enum { CHIP_TARF_NAME_GNU = 1, CHIP_TARF_NAME_PAX = 2, CHIP_TARF_LINK_GNU = 4, CHIP_TARF_LINK_PAX = 8,
       CHIP_TARF_SIZE_PAX = 16, CHIP_TARF_SIZE_BASE256 = 32 };
typedef struct {            /* 72 bytes, no implicit padding */
    uint64_t group_off;     /* first header of the group (== header_off without extension headers) */
    uint64_t header_off, data_off, size, name_off, link_off;
    int64_t  mtime;         /* header field; an invalid field is 0 (pax mtime is not applied) */
    uint32_t name_len, link_len, mode;   /* mode: header field, invalid is 0 */
    uint16_t prefix_len;    /* prefix bytes at header_off + 345 */
    uint8_t  typeflag, flags;            /* CHIP_TARF_* */
} chip_tar_entry;
typedef struct {
    uint64_t n_entries, n_global, total_size, stop_off, bad_off;
    int32_t status;         /* CHIP_TAR_* */
    int32_t zero_blocks;
} chip_tar_plan_summary;
int chip_tar_plan_host(const uint8_t *in, uint64_t len, uint64_t max_entries, chip_tar_entry *entries, chip_tar_plan_summary *summary);
int chip_tar_plan(const void *in_base, uint64_t len, uint64_t max_entries, chip_tar_entry *entries, chip_tar_plan_summary *summary,
                  void *stream);

/* ---- tar archives: writing (additive API) ----------------------------------- */

/*
 * The image chip_tar_plan, Python's tarfile and GNU tar read back, made on the device: the counterpart of chip_zip_write.  Member i
 * is a chip_tar_source: its content is content[data_off .. + size), its name names[name_off .. + name_len), its link name
 * names[link_off .. + link_len) (may be empty).  The image is not compressed; chip_encode_file makes the .tar.zst or .tar.gz.
 *   chip_tar_write_host   the whole image on the host; the definition.
 *   chip_tar_write        the same with every array and buffer in DEVICE memory, summary on the HOST, and a stream.
 *   chip_tar_write_bound  up(content_total + 2 * names_total + 3072 * n + 1024, record), or 0 when that overflows 64 bits or
 *                         record_bytes is refused: always enough.  A group is 512 + up512(size) and, per name above 100 bytes, at
 *                         most 512 + up512(len + 1) <= 822 + 2 * len, so 2667 bytes above size + 2 * names bound it.
 * The image is DEFINED by these rules.  GNU = flags & CHIP_TW_GNU, else the image is pax.
 *   Accepted sources; anything else is CHIP_TARW_BAD_SOURCE with bad_index the LOWEST offender, nothing but the summary is written
 *     and its other fields are 0 except n_entries: typeflag '0'..'7'; size == 0 for '1'..'6'; 1 <= name_len <= CHIP_TARW_NAME_MAX,
 *     link_len <= CHIP_TARW_NAME_MAX; no NUL byte in the name or the link name; name_off + name_len and link_off + link_len inside
 *     names_len, data_off + size inside content_len, the sums formed without wrapping; mode <= 07777777; uid, gid < 8^7;
 *     0 <= mtime < 8^11; pad == 0.
 *   A header block, 512 bytes, zero where nothing is said: 0 name (up to 100 bytes) | 100, 108, 116 mode, uid, gid as %07o NUL |
 *     124 size as %011o NUL, or base-256: 80 and 11 big-endian bytes | 136 mtime as %011o NUL | 148 chksum as %06o NUL space: the
 *     unsigned sum of the block with this field taken as spaces | 156 typeflag | 157 link name (up to 100 bytes) | 257 "ustar" NUL
 *     "00", GNU: "ustar" two spaces NUL | 265, 297 uname, gname: empty | 329, 337 devmajor, devminor: "0000000" NUL | 345 prefix (up
 *     to 155 bytes).  A field that is exactly full has no NUL behind it.
 *   The group of member i; the groups follow each other from offset 0 with no gaps.  BIG = size >= 8^11 or CHIP_TW_FORCE_EXT.
 *     pax   A name of at most 100 bytes goes into the name field.  A longer one is split at the LARGEST p with name[p] == '/',
 *           1 <= p <= 155 and 1 <= name_len - p - 1 <= 100: prefix = name[0 .. p), name field = name[p + 1 ..).  Without such a p a
 *           `path` record carries the name and the field holds its first 100 bytes.  A link name above 100 bytes gets a `linkpath`
 *           record and the field its first 100 bytes.  BIG gets a `size` record in decimal; the size field is the size when it is
 *           below 8^11, else 0.  With at least one record ONE x header precedes the member header: name "././@PaxHeader", mode
 *           0644, uid and gid 0, the member's mtime, size = the records' length; the records follow in the order path, linkpath,
 *           size, zero-padded to 512.  A record is "<L> <key>=<value>\n", L the smallest decimal number that counts the whole
 *           record, its own digits included.
 *     GNU   No prefix split.  A link name above 100 bytes gets a K header, a name above 100 bytes an L header, K first: name
 *           "././@LongLink", mode, uid, gid and mtime 0, size = len + 1; the data is the bytes and one NUL, zero-padded to 512.
 *           The member header holds the first 100 bytes of each.  BIG writes the size field in base-256.
 *     Then the member header and the content, zero-padded to 512.
 *   The end: two zero blocks at end_off, then zeros up to the next multiple of record_bytes (a multiple of 512, at most 2^20;
 *     0 means 10 240, the default of tar and tarfile).
 *   entries[i] (may be NULL) is the chip_tar_entry chip_tar_plan produces for member i of the written image: the offsets,
 *     prefix_len, and the flags NAME_PAX / NAME_GNU / LINK_* / SIZE_PAX / SIZE_BASE256.
 * summary: n_entries = n, n_ext the extension headers written, out_len the whole image, end_off, total_size the sum of the sizes.
 *   CHIP_TARW_NEED_OUTPUT  out_len > out_cap: out_len is exact, entries and the summary are answered, no byte of `out` is written and
 *                          no byte of content is read.  Names are read: the layout depends on them.
 *   CHIP_TARW_OK           every byte of out[0 .. out_len) is written exactly once, by a store that covers only bytes of its own
 *                          block or range (chip_pack_units' discipline): the padding, the end blocks and the record padding are
 *                          bytes of the image and are written as zeros.  Nothing outside is written; `out` may have any alignment.
 * `out` must not overlap the inputs.
 * CHIP_E_INVALID, before a device is looked for: summary NULL; src NULL with n > 0, names NULL with names_len > 0, content NULL
 * with content_len > 0, out NULL with out_cap > 0; unknown flag bits; record_bytes no multiple of 512 or above 2^20; n > 2^31 - 1;
 * and arguments that allow an image of 2^63 bytes or more: content_len >= 2^62, or n * (content_len + 134 144) > 2^63 - 2^20 - 1024.
 * n == 0 is answered by the host: the end blocks alone, zeroed with one memset on `stream` that is waited for.
 * chip_tar_write is SYNCHRONOUS on `stream` and waits twice: for the groups' total against the room, and at the end.  Scratch per
 * (device, stream), a launch slot of its own released by chip_trim(): 284 bytes per entry (64 the kept record, 24 the scan, 196 the
 * seven pieces of the copy) and 24 bytes per 1024 entries, with a quarter of headroom.  CHIP_E_NOMEM: the scratch could not be
 * allocated.  CHIP_E_LAUNCH: a launch failed, or the inputs changed during the call; nothing is ever written out of range.
 * Not written: uname and gname, device numbers, pax mtime / uid records, sparse members, global headers.
 * No reference counterpart: compu has no container formats.
 */
enum { CHIP_TW_GNU = 1, CHIP_TW_FORCE_EXT = 2 };                       /* call flags */
enum { CHIP_TARW_OK = 0, CHIP_TARW_NEED_OUTPUT = 1, CHIP_TARW_BAD_SOURCE = 2 };
#define CHIP_TARW_NAME_MAX 65535u
typedef struct {            /* 64 bytes, no implicit padding */
    uint64_t data_off, size;        /* content[data_off .. + size) */
    uint64_t name_off, link_off;    /* names[name_off .. + name_len), names[link_off .. + link_len) */
    int64_t  mtime;
    uint32_t name_len, link_len, mode, uid, gid;
    uint8_t  typeflag, pad[3];      /* pad must be 0 */
} chip_tar_source;
typedef struct {            /* 56 bytes */
    uint64_t n_entries, n_ext, out_len, end_off, total_size, bad_index;
    int32_t status, pad;
} chip_tar_write_summary;
int chip_tar_write_host(uint64_t n, const chip_tar_source *src, const uint8_t *names, uint64_t names_len, const uint8_t *content,
                        uint64_t content_len, uint32_t flags, uint32_t record_bytes, uint8_t *out, uint64_t out_cap,
                        chip_tar_entry *entries, chip_tar_write_summary *summary);
int chip_tar_write(uint64_t n, const chip_tar_source *src, const void *names, uint64_t names_len, const void *content,
                   uint64_t content_len, uint32_t flags, uint32_t record_bytes, void *out, uint64_t out_cap,
                   chip_tar_entry *entries, chip_tar_write_summary *summary, void *stream);
uint64_t chip_tar_write_bound(uint64_t n, uint64_t names_total, uint64_t content_total, uint32_t record_bytes);

/* ---- encoder: mirrors encoder::Interface, src/encoder/mod.rs:52-57 ---------------------------- */

typedef struct chip_encoder chip_encoder;

/* ZlibStrategy src/encoder/zlib_common.rs:5-24 (what zlib_ng.rs:69-75 hands to deflateInit2_) */
enum { CHIP_STRATEGY_DEFAULT = 0, CHIP_STRATEGY_FILTERED = 1, CHIP_STRATEGY_HUFFMAN_ONLY = 2, CHIP_STRATEGY_RLE = 3, CHIP_STRATEGY_FIXED = 4 };

/* ZlibOptions src/encoder/zlib_common.rs:47-103, every field (zlib-ng keeps them in its state and ignores the two
 * bytes compu replays on reset: src/encoder/zlib_ng.rs:84,95) */
typedef struct {
    int32_t mode;        /* CHIP_FMT_DEFLATE | CHIP_FMT_ZLIB | CHIP_FMT_GZIP (default Gzip, zlib_common.rs:33-37) */
    int32_t compression; /* 0..9, or -1 = zlib's default (6) as zlib_common.rs:96-103 allows: 0 stored blocks, 1 greedy
                          * match + one fixed-Huffman block, 2..9 the same match finder + dynamic-Huffman blocks,
                          * 4..9 with lazy choice (a match gives way to a longer one at the next position),
                          * 6..9 with two candidate positions per hash slot (the older one wins with a longer match) */
    int32_t device;      /* HIP device ordinal, -1 = current */
    int32_t strategy;    /* CHIP_STRATEGY_*: HuffmanOnly emits no matches, Rle only distance-1 matches, Fixed forces the
                          * fixed code at every level (zlib's Z_FIXED); Default and Filtered are the same here */
    int32_t mem_level;   /* 1..9 (zlib's memLevel; 0 = default 8): accepted for compatibility, the GPU state has one size */
} chip_encoder_opts;

/* Interface::zlib_ng(opts) src/encoder/zlib_ng.rs:50-87 */
chip_encoder *chip_encoder_new(const chip_encoder_opts *opts);
/* encode_fn src/encoder/zlib_ng.rs:90-92 (+ macro src/encoder/mod.rs:334-370) */
chip_encode_result chip_encode(chip_encoder *e, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, int op);
/* reset_fn src/encoder/zlib_ng.rs:95-104 */
chip_encoder *chip_encoder_reset(chip_encoder *e);
/* drop_fn src/encoder/zlib_ng.rs:107-111 */
void chip_encoder_free(chip_encoder *e);

/* chip_encode_batch with a strategy (CHIP_STRATEGY_*, CHIP_ZSTD_STRATEGY_* for CHIP_FMT_ZSTD, or the brotli mode 0..3 for
 * CHIP_FMT_BROTLI); chip_encode_batch is strategy Default (mode 0). */
int chip_encode_batch_ex(int format, int level, int strategy, size_t n, const void *in_base, const uint64_t *in_off,
                         const uint32_t *in_len, void *out_base, const uint64_t *out_off, const uint32_t *out_cap,
                         uint32_t *out_len, int32_t *status, void *stream);

/* Batched encode of n independent units (device pointers, one wavefront per unit).  CHIP_FMT_ZSTD: level as in
 * chip_zstd_encoder_opts, window_log 27; each unit becomes one zstd frame with the content checksum (single segment with
 * Frame_Content_Size up to 2^27 bytes, a 2^27 window above).  CHIP_FMT_BROTLI: level = quality 0..11 (0 = 11, -1 is
 * CHIP_E_INVALID), strategy = mode 0..3; each unit becomes one brotli stream with lgwin 22.
 * out_len[i] = compressed size; status[i] = CHIP_ENC_FINISHED or CHIP_ENC_NEED_OUTPUT.  Each unit becomes
 * one complete stream of `format` (wrapper, one fixed-Huffman or stored deflate body, trailer).  The
 * range out_off[i] .. +out_cap[i] may be used as scratch beyond out_len[i].
 * CHIP_FMT_BGZF: levels and strategies as CHIP_FMT_GZIP, and the same deflate body; each unit becomes one BGZF block -- the
 * 18-byte header of chip_bgzf_plan with MTIME 0, XFL as for gzip, OS ff (as htslib writes) and BSIZE = out_len[i] - 1, then
 * CRC-32 and ISIZE.  A unit with in_len[i] > 65280 (htslib's block payload) is CHIP_ENC_ERROR with out_len[i] = 0; a block never
 * exceeds 65 536 bytes (incompressible input is stored: 65 280 + 5 + 26; a dynamic-level block costs at most 6 bytes more).
 * The blocks stay in their slots: chip_pack_units lays them end to end, and chip_encode_file does all of it -- cut, encode, pack,
 * EOF marker (chip_bgzf_eof_block) -- in one call (below, "writing files"). */
int chip_encode_batch(int format, int level, size_t n, const void *in_base, const uint64_t *in_off,
                      const uint32_t *in_len, void *out_base, const uint64_t *out_off, const uint32_t *out_cap,
                      uint32_t *out_len, int32_t *status, void *stream);
/* Worst-case compressed size for in_len input bytes in `format` (sizing out_cap). */
size_t chip_encode_bound(int format, size_t in_len);

/* chip_encode_batch for data in (pinned) host memory: same two-stream slicing and layout rules as
 * chip_decode_batch_host (exactly out_len[i] bytes are written at out_off[i]). */
int chip_encode_batch_host(int format, int level, size_t n, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                           void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int32_t *status,
                           int device, size_t slice_bytes);

/* ---- writing files: from a batch to a file (additive API) ---------------- */

/*
 * chip_encode_batch leaves every unit in a slot of its own; a file is those units end to end.  chip_pack_units is that step on
 * the device.  src_base, src_off, src_len, dst_base and dst_off are DEVICE pointers, total is a HOST pointer.
 *   dst_off[i] = the exclusive 64-bit sum of src_len[0 .. i)             (dst_off may be NULL: not wanted)
 *   *total     = the sum of all lengths
 *   *total <= dst_cap:  the bytes src_base[src_off[i] .. + src_len[i]) land at dst_base[dst_off[i] ..)
 *   *total >  dst_cap:  no byte of dst_base is written; the call is still CHIP_OK and *total and dst_off are answered -- the caller
 *                       compares, allocates and calls again
 * The contract.  src_base and dst_base may have any alignment.  Source ranges may lie in any order, with gaps, and may overlap
 * each other; the destination must not overlap any of them.  Nothing outside [src_off[i], src_off[i] + src_len[i]) is read and
 * nothing outside dst_base[0 .. total) is written; every destination byte is written exactly once, with a store that covers
 * only bytes of the range (the byte behind `total` keeps its value, whatever the alignment).
 * SYNCHRONOUS on `stream`, as chip_layout_units (the caller allocates or writes `total` bytes next).  n == 0 writes *total = 0
 * without touching the device.  CHIP_E_INVALID before the device is looked for: total NULL, src_base / src_off / src_len NULL
 * with n > 0, dst_base NULL with dst_cap > 0, n > 2^32 - 1.  Scratch: 8 bytes per unit (the offsets) and 8 bytes per 1024 units in
 * the slot of chip_encode_file.  The calling thread's current device is left as it was.
 * No reference counterpart: compu has no container formats.  Without it a caller copies out_len[] to the host, sums it and
 * issues one copy per unit.
 */
int chip_pack_units(size_t n, const void *src_base, const uint64_t *src_off, const uint32_t *src_len, void *dst_base, uint64_t dst_cap,
                    uint64_t *dst_off, uint64_t *total, void *stream);

/*
 * From a buffer to a file, both in DEVICE memory: the file chip_bgzf_plan, chip_gzip_plan (or CHIP_F_MEMBERS) or chip_zstd_plan reads back.  The
 * input is cut into n = ceil(len / unit_bytes) units, unit i = [i * unit_bytes, min(len, (i + 1) * unit_bytes)); every unit is
 * encoded by chip_encode_batch(format, level, ..) -- the same kernels, the same bytes -- into a scratch slot of
 * chip_encode_bound(format, unit_bytes) bytes rounded up to 16; the encoded units are packed end to end into out_base
 * (chip_pack_units' kernel) and the format's trailer follows.
 *   CHIP_FMT_BGZF  unit_bytes 0 (= 65 280, htslib's payload) or 1 .. 65 280; one BGZF block per unit, then htslib's 28-byte EOF
 *                  block.  len == 0: the EOF block alone (n_units = 0), as bgzip writes for empty input.
 *   CHIP_FMT_GZIP  unit_bytes 0 (= 262 144) or 1 .. 2^30; one gzip member per unit: the series gzip -d and CHIP_F_MEMBERS read.
 *                  len == 0: one member of empty content (a file of no bytes is not gzip).
 *   CHIP_FMT_ZSTD  unit_bytes as for gzip; one frame per unit, with content checksum and Frame_Content_Size as the batch
 *                  encoder writes them.  len == 0: one frame of empty content.  With CHIP_W_SEEK_TABLE the seek table of zstd's
 *                  seekable format (contrib/seekable_format, without per-frame checksums) follows the last frame:
 *                    LE32 0x184D2A5E | LE32 8 * n + 9 | n x { LE32 compressed size, LE32 content size } | LE32 n | u8 0 |
 *                    LE32 0x8F92EAB1                                                  -- 17 + 8 * n bytes, a skippable frame
 * level: as chip_encode_batch (strategy Default).  The 262 144 is a convention (the frame size DESIGN.md sec. 4.12 was measured
 * at), not a tuned number.
 * summary (HOST): n_units = units encoded; out_len = the file's length; table_off = where the seek table starts (out_len without
 * one); status = CHIP_FILE_OK, or CHIP_FILE_NEED_OUTPUT when out_len > out_cap: out_len is then the exact size to come back with
 * and no byte of out_base has been written.  chip_encode_file_bound is the size that is always enough:
 * (n - 1) * chip_encode_bound(unit_bytes) + chip_encode_bound(last unit) + trailer; pure host arithmetic, 0 for arguments
 * chip_encode_file refuses.
 * in_base is 4-byte aligned and its allocation padded to a multiple of 4 bytes, as for chip_encode_batch.  SYNCHRONOUS on
 * `stream`: it waits once for the packed size and once for the file.
 * CHIP_E_INVALID, before the device is looked for: summary NULL; in_base NULL with len > 0 or not 4-byte aligned; out_base NULL
 * with out_cap > 0; len > 2^40; n > 2^31 - 1; any other format (brotli, deflate and zlib have no concatenation convention);
 * level or unit_bytes out of range; unknown flag bits; CHIP_W_SEEK_TABLE with another format than zstd, or with
 * n > 0x8000000 (the format's limit; its other limit, 0x40000000 bytes per frame, is the limit of unit_bytes).
 * CHIP_E_NOMEM: the scratch could not be allocated.  CHIP_E_LAUNCH: a launch failed, or a unit did not end CHIP_ENC_FINISHED
 * (which slots of chip_encode_bound bytes rule out).
 * Scratch per (device, stream), a launch slot kept between calls and released by chip_trim(): the slot area, n * up16(
 * chip_encode_bound(format, unit_bytes)) bytes -- a little more than the input -- plus 32 bytes per unit of arrays (filled by a
 * kernel, not uploaded) and 8 bytes per 1024 units, each allocation with a quarter of headroom.  There are no slabs yet: the
 * whole input is encoded before the first byte is packed.  The calling thread's current device is left as it was.
 * No reference counterpart.
 */
enum { CHIP_W_SEEK_TABLE = 1 };
enum { CHIP_FILE_OK = 0, CHIP_FILE_NEED_OUTPUT = 1 };
typedef struct {
    uint64_t n_units, out_len, table_off;
    int32_t status;
    uint32_t pad;
} chip_file_summary;
int chip_encode_file(int format, int level, uint32_t unit_bytes, uint32_t flags, const void *in_base, uint64_t len, void *out_base,
                     uint64_t out_cap, chip_file_summary *summary, void *stream);
uint64_t chip_encode_file_bound(int format, uint32_t unit_bytes, uint32_t flags, uint64_t len);

/* ---- reading ranges: random access on a plan (additive API) -------------- */

/*
 * BGZF blocks and the frames of a seekable zstd file are small so that a reader can fetch a region without decoding the file.
 * These calls answer "give me bytes [lo, lo + len) of the decoded content" for many ranges at once: the units the ranges touch are
 * found, each is decoded once, and the ranges land end to end.
 * The inputs are n_units units with in_off, in_len, out_off, out_cap as chip_bgzf_plan, chip_zstd_plan or chip_layout_units leave
 * them, and n_ranges ranges (range_lo[r] u64, range_len[r] u32) in content coordinates, the coordinates of out_off.  The answer
 * is defined by this walk (host and device implement the same one):
 *   n_ranges == 0 -> an all-zero summary, the layout is not looked at
 *   layout check.  For every unit i the link to i + 1 FAILS when out_cap[i] == CHIP_ZPLAN_UNSIZED (a frame without a size; the
 *       last unit too), or out_off[i] + out_cap[i] exceeds 2^64 - 1, or i + 1 < n_units and out_off[i + 1] != out_off[i] +
 *       out_cap[i].  Any failing link: status = CHIP_READ_BAD_LAYOUT, bad_index = the lowest such i + 1, every other field of the
 *       summary is 0 and NOTHING else is written.
 *   begin = out_off[0];  end = out_off[n_units - 1] + out_cap[n_units - 1]     (both 0 for n_units == 0)
 *   per range r, (lo, len):
 *     len == 0                          -> CHIP_RANGE_OK, touches no unit, 0 bytes
 *     lo < begin, or lo + len > end     -> CHIP_RANGE_OUTSIDE, touches no unit, counts 0 bytes (the sum is formed without
 *                                          wrapping; there is no clipping)
 *     otherwise                         -> CHIP_RANGE_OK;  first[r] = the last unit u with out_off[u] <= lo: the unit that holds
 *                                          byte lo (empty units at lo sit in front of it);  last[r] = the same for lo + len - 1
 *   selection.  Unit u is selected when out_cap[u] > 0 and some range has first <= u <= last: units of no content are never
 *     decoded.  The selected units ascend by index; k(u) is u's position among them; sel_out_off[k] = the exclusive 64-bit sum of
 *     the selected units' out_cap, scratch_bytes the total.  The units one range selects are therefore contiguous in that image.
 *   src_off[r] = sel_out_off[k(first[r])] + (lo - out_off[first[r]])                (0 for a range that touches no unit)
 *   dst_off[r] = the exclusive 64-bit sum of the lengths that count (len of a range that is OK, 0 for CHIP_RANGE_OUTSIDE)
 *   out_len    = the sum of those lengths;  n_outside = the number of CHIP_RANGE_OUTSIDE ranges
 * Ranges may come in any order, overlap, nest and repeat: every one gets its own bytes in the output, a unit is selected once.
 */
enum { CHIP_READ_OK = 0, CHIP_READ_NEED_OUTPUT = 1, CHIP_READ_BAD_LAYOUT = 2 };
enum { CHIP_RANGE_OK = 0, CHIP_RANGE_OUTSIDE = 1, CHIP_RANGE_BAD_UNIT = 2 };
typedef struct {
    uint64_t n_sel, scratch_bytes, out_len, n_outside, bad_index;
    int32_t status; /* CHIP_READ_OK or CHIP_READ_BAD_LAYOUT */
    uint32_t pad;
} chip_select_summary;

/* The walk itself on HOST memory: pure host arithmetic, no device needed (as chip_bgzf_plan_host).  sel_unit (the unit's index
 * in the plan) and the four arrays of the sub-batch, sel_in_off / sel_in_len / sel_out_off / sel_out_cap -- what chip_decode_batch
 * takes to decode the selection into scratch_bytes bytes -- receive the first min(n_sel, max_sel) selected units and nothing behind
 * them is written: max_sel = 0 with null arrays counts, a second call fills.  src_off, dst_off and range_status have n_ranges
 * entries; each may be NULL (not wanted).  CHIP_E_INVALID: summary NULL, a plan array NULL with n_units > 0, range_lo or range_len
 * NULL with n_ranges > 0, one of the five sel arrays NULL with max_sel > 0, n_units or n_ranges above 2^32 - 1.  CHIP_E_NOMEM:
 * the 12 bytes per unit and 4 per range of working memory could not be allocated. */
int chip_select_units_host(size_t n_units, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap,
                           size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, uint64_t max_sel, uint32_t *sel_unit,
                           uint64_t *sel_in_off, uint32_t *sel_in_len, uint64_t *sel_out_off, uint32_t *sel_out_cap, uint64_t *src_off,
                           uint64_t *dst_off, int32_t *range_status, chip_select_summary *summary);

/* The same answer for DEVICE arrays (every array pointer; summary is a HOST pointer): the index step alone, for a caller that
 * decodes into a buffer of its own.  Arguments are checked before the device is looked for.  SYNCHRONOUS on `stream` (n_sel and
 * scratch_bytes are host arguments of what follows).  Scratch per (device, stream), a launch slot of its own, kept between calls
 * and released by chip_trim(): 24 bytes per unit, 28 bytes per range, at most 24 bytes per 1024 of either, with a quarter of headroom.
 * The calling thread's current device is left as it was. */
int chip_select_units(size_t n_units, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap,
                      size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, uint64_t max_sel, uint32_t *sel_unit,
                      uint64_t *sel_in_off, uint32_t *sel_in_len, uint64_t *sel_out_off, uint32_t *sel_out_cap, uint64_t *src_off, uint64_t *dst_off,
                      int32_t *range_status, chip_select_summary *summary, void *stream);

/*
 * Select, decode and gather, all in DEVICE memory: the bytes of range r land at dst_base[dst_off[r] .. + range_len[r]).  in_base is
 * the file the plan was made of; `format` goes on to chip_decode_batch(format, n_sel, ..), whose formats, alignment and padding
 * rules of in_base hold (CHIP_FMT_GZIP for a BGZF plan, CHIP_FMT_ZSTD for a frame plan).  dst_off and range_status are DEVICE
 * arrays of n_ranges entries, each may be NULL; summary is a HOST pointer.
 *   status = CHIP_READ_BAD_LAYOUT (bad_index says where): nothing is decoded, nothing at all is written.
 *   status = CHIP_READ_NEED_OUTPUT when out_len > dst_cap: out_len is the exact size to come back with, dst_off and range_status
 *            are answered, nothing is decoded (n_units = 0) and no byte of dst_base is written.
 *   status = CHIP_READ_OK: n_units = n_sel units were decoded, each once, into the slot's scratch area.  A selected unit that did
 *            not end CHIP_FINISHED with out_len == out_cap is a bad unit: n_bad counts them, first_bad is the lowest one's index
 *            in the plan and bad_status its decode status (CHIP_FINISHED when only the length was wrong); without one all three
 *            are 0.  A range whose span first .. last holds a bad unit gets CHIP_RANGE_BAD_UNIT, and the bytes in its own
 *            [dst_off[r], + len) are unspecified; every other range has its bytes.  Units no range touches are never decoded,
 *            damaged or not.
 * Nothing outside dst_base[0 .. out_len) is ever written, at any alignment of dst_base; a destination byte is written once, by
 * a store that covers only bytes of the output (chip_pack_units' copy).  dst_base must not overlap in_base.
 * SYNCHRONOUS on `stream`: it waits once for {n_sel, scratch_bytes, out_len} and once at the end.
 * CHIP_E_INVALID, before the device is looked for: summary NULL; a plan array or in_base NULL with n_units > 0; range_lo or
 * range_len NULL with n_ranges > 0; dst_base NULL with dst_cap > 0; n_units or n_ranges above 2^32 - 1; a format
 * chip_decode_batch refuses; in_base not 4-byte aligned.  n_ranges == 0: CHIP_OK, an all-zero summary, the device is not touched.
 * CHIP_E_NOMEM: the scratch could not be allocated.  CHIP_E_LAUNCH: a launch failed, or more than 2^31 - 1 units were selected.
 * Scratch per (device, stream), the slot of chip_select_units: 72 bytes per unit (the selection may be every unit: the sub-batch
 * and the decode's answers are sized for it), 28 bytes per range, and scratch_bytes + 64 for the decoded image, each allocation
 * with a quarter of headroom.  The calling thread's current device is left as it was.
 * No reference counterpart: compu has no container formats.  Without it a caller decodes the whole plan and slices, or copies the
 * plan to the host, searches it there, uploads a sub-batch and issues one copy per range.
 */
typedef struct {
    uint64_t n_units, out_len, n_outside, n_bad, first_bad, bad_index;
    int32_t status; /* CHIP_READ_* */
    int32_t bad_status;
} chip_read_summary;
int chip_read_ranges(int format, size_t n_units, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off,
                     const uint32_t *out_cap, size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, void *dst_base,
                     uint64_t dst_cap, uint64_t *dst_off, int32_t *range_status, chip_read_summary *summary, void *stream);

/* ---- seekable zstd files: the seek table as a plan (additive API) ------------ */

/*
 * zstd's seekable format (contrib/seekable_format) ends a series of frames with a skippable frame that lists every frame's
 * compressed size, content size and, optionally, the low 32 bits of the content's XXH64.  A reader takes the last few KiB of the
 * file, knows where every frame lies, and fetches and decodes only the frames its ranges touch.  These calls read such a table as
 * a plan (the four arrays of chip_zstd_plan, plus the checksums), write one, make the checksums, and read ranges with the
 * checksums verified on the device.  The table is untrusted input: its sizes are checked by the decode (a frame that does not end
 * CHIP_FINISHED at exactly out_cap bytes is a bad unit), its checksums by chip_zstd_seek_read.
 *
 * `tail` is the last tail_len bytes of a file of file_len bytes: byte j of tail is byte file_len - tail_len + j of the file.  All
 * integers are little endian.  The answer is defined by this walk (host and device implement the same one):
 *   file_len < 17                                   -> CHIP_ZSEEK_NO_TABLE
 *   tail_len < 17                                   -> CHIP_ZSEEK_NEED_TAIL, table_bytes = 17
 *   LE32(tail_len - 4) != 0x8F92EAB1                -> CHIP_ZSEEK_NO_TABLE
 *   desc = byte(tail_len - 5);  desc & 0x7C         -> CHIP_ZSEEK_BAD_TABLE   (reserved bits; the two low bits are ignored)
 *   cs = desc >> 7;  es = 8 + 4 * cs;  n = LE32(tail_len - 9)
 *   n > 0x8000000                                   -> CHIP_ZSEEK_BAD_TABLE
 *   T = 17 + es * n;  T > file_len                  -> CHIP_ZSEEK_BAD_TABLE
 *      from here on the summary has n_frames = n, table_bytes = T, checksums = cs
 *   tail_len < T                                    -> CHIP_ZSEEK_NEED_TAIL   (come back with the last T bytes)
 *   LE32(tail_len - T) != 0x184D2A5E, or LE32(tail_len - T + 4) != T - 8      -> CHIP_ZSEEK_BAD_TABLE
 *   entry i at tail_len - T + 8 + es * i:  c_i = LE32, d_i = LE32, x_i = LE32 when cs (else 0)
 *      some d_i == 0xFFFFFFFF (CHIP_ZPLAN_UNSIZED is taken)  -> CHIP_ZSEEK_TOO_LARGE, bad_index = the lowest such i
 *      in_off[i] = c_0 + .. + c_(i-1)  (FILE coordinates, 64-bit),  in_len[i] = c_i,
 *      out_off[i] = d_0 + .. + d_(i-1),  out_cap[i] = d_i,  checksum[i] = x_i
 *   C = sum of c_i;  C > file_len - T               -> CHIP_ZSEEK_BAD_LAYOUT  (C < file_len - T is accepted: foreign skippable
 *                                                                             frames may sit in front of the table)
 *   CHIP_ZSEEK_OK: frames_bytes = C, total_out = sum of d_i
 * Every field of the summary that the walk has not set by the line it stops at is 0.  The arrays receive the first
 * min(n, max_frames) entries and nothing behind them is written: max_frames = 0 with NULL arrays counts, a second call fills.
 * `checksum` may be NULL (not wanted).  With a status other than CHIP_ZSEEK_OK the arrays' contents are unspecified.
 * The plan judges only the table.  An entry is taken to be one zstd frame: an entry that is several frames, or a skippable frame
 * with d_i > 0, surfaces as a bad unit at decode; entries with d_i == 0 are never selected by a read.
 * CHIP_E_INVALID: summary NULL, tail NULL with tail_len > 0, tail_len > file_len, file_len > 2^40, or one of in_off, in_len,
 * out_off, out_cap NULL with max_frames > 0.
 */
enum { CHIP_ZSEEK_OK = 0, CHIP_ZSEEK_NO_TABLE = 1, CHIP_ZSEEK_NEED_TAIL = 2, CHIP_ZSEEK_BAD_TABLE = 3, CHIP_ZSEEK_TOO_LARGE = 4,
       CHIP_ZSEEK_BAD_LAYOUT = 5 };
typedef struct {
    uint64_t n_frames, table_bytes, frames_bytes, total_out, bad_index;
    int32_t status;     /* CHIP_ZSEEK_* */
    uint32_t checksums; /* 1: the entries carry checksums */
} chip_zstd_seek_summary;

/* The walk on HOST memory: pure host arithmetic, no device needed. */
int chip_zstd_seek_plan_host(const uint8_t *tail, uint64_t tail_len, uint64_t file_len, uint64_t max_frames, uint64_t *in_off,
                             uint32_t *in_len, uint64_t *out_off, uint32_t *out_cap, uint32_t *checksum, chip_zstd_seek_summary *summary);

/* The same answer for a tail in DEVICE memory: tail and the five arrays are DEVICE pointers, summary is a HOST pointer.  tail may
 * have any alignment (a file's table starts wherever it starts); reads stay inside the aligned dwords that hold bytes of the tail.
 * Arguments are checked before the device is looked for, and a walk that stops before a byte is read (file_len or tail_len below
 * 17) is answered on the host.  SYNCHRONOUS on `stream`: it waits once for the footer and the table's header (the grid is sized
 * from n), once for the sums.  One lane per entry reads its 8 or 12 bytes; the offsets are two 64-bit exclusive scans.  Every byte
 * of the tail is read once and every position follows from the n the host holds, so input that changes during the call changes
 * the answer and never where something is read or written; CHIP_E_LAUNCH: a launch failed, or what came back from the device
 * contradicts itself.  CHIP_E_NOMEM: the scratch could not be allocated.  Scratch per (device, stream), a launch slot of its own,
 * kept between calls and released by chip_trim(): 16 bytes per entry, with a quarter of headroom.  The calling thread's current
 * device is left as it was.  No reference counterpart: compu has no container formats. */
int chip_zstd_seek_plan(const void *tail, uint64_t tail_len, uint64_t file_len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len,
                        uint64_t *out_off, uint32_t *out_cap, uint32_t *checksum, chip_zstd_seek_summary *summary, void *stream);

/*
 * Writing a table: 17 + (checksum ? 12 : 8) * n bytes at dst,
 *   LE32 0x184D2A5E | LE32 size - 8 | n x { LE32 c_len[i], LE32 d_len[i] [, LE32 checksum[i]] } | LE32 n | u8 (checksum ? 0x80 : 0) |
 *   LE32 0x8F92EAB1
 * The entries go out as they are handed in.  With checksum == NULL the bytes are the ones chip_encode_file(.., CHIP_W_SEEK_TABLE)
 * writes for the same lengths.  *table_bytes (HOST) is always the exact size; when it exceeds dst_cap nothing is written.
 * CHIP_E_INVALID: table_bytes NULL, n > 0x8000000 (the format's limit), c_len or d_len NULL with n > 0, dst NULL with dst_cap > 0.
 * chip_zstd_seek_table_write: the three arrays and dst are DEVICE pointers; dst may have any alignment, each destination byte is
 * written once, by a store that covers only bytes of the table.  It only enqueues on `stream` (no wait, no scratch); arguments are
 * checked before the device is looked for, and a table that does not fit does not touch it.  No reference counterpart.
 */
int chip_zstd_seek_table_write_host(uint64_t n, const uint32_t *c_len, const uint32_t *d_len, const uint32_t *checksum, void *dst,
                                    uint64_t dst_cap, uint64_t *table_bytes);
int chip_zstd_seek_table_write(uint64_t n, const uint32_t *c_len, const uint32_t *d_len, const uint32_t *checksum, void *dst,
                               uint64_t dst_cap, uint64_t *table_bytes, void *stream);

/*
 * XXH64 of many ranges of DEVICE memory: digest[i] = XXH64, seed 0, of base[off[i] .. + len[i]), all 64 bits (a table's entry
 * holds the low 32); len[i] == 0 gives 0xEF46DB3751D8E999.  Every pointer is a DEVICE pointer.  off[i] may have any alignment;
 * loads stay inside the aligned dwords that hold bytes of the range.  len is 32-bit so that a plan's out_off / out_cap go in
 * unchanged.  It only enqueues on `stream`: no wait, no scratch.
 * One wave hashes one range.  XXH64 is a serial chain per range: many ranges fill the card, one huge range runs at one wave's
 * rate (1.1 GB/s) -- that is the limit of this form.
 * CHIP_E_INVALID, before the device is looked for: a NULL array or base with n > 0, n > 2^31 - 1.  n == 0: CHIP_OK, the device is
 * not touched.  CHIP_E_LAUNCH: the launch failed.  No reference counterpart.
 */
int chip_xxh64_batch(size_t n, const void *base, const uint64_t *off, const uint32_t *len, uint64_t *digest, void *stream);

/*
 * chip_read_ranges(CHIP_FMT_ZSTD, ..) over the plan of a seek table, with the table's checksums verified on the device.
 * With checksum == NULL it IS that call, to the byte and to the summary.  With checksum (a DEVICE array of n_units entries):
 * behind the decode and its check of status and length, one wave hashes the decoded image of each selected unit that is not
 * already bad; a unit whose XXH64's low 32 bits differ from checksum[unit] becomes a bad unit with bad_status -22, the decoder's
 * own code for a wrong content checksum.  n_bad counts a unit once; ranges whose span holds a bad unit get CHIP_RANGE_BAD_UNIT.
 * The rest of chip_read_ranges' contract holds word for word: the argument checks (the format is fixed), the two waits, the
 * scratch and its slot, and "units no range touches are never decoded, damaged or not" -- nor are their checksums or in_off looked
 * at.  in_off are whatever the caller hands over: a reader that holds only part of the file rebases the selected units' offsets
 * to its own buffer.  No reference counterpart.
 */
int chip_zstd_seek_read(size_t n_units, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off,
                        const uint32_t *out_cap, const uint32_t *checksum, size_t n_ranges, const uint64_t *range_lo,
                        const uint32_t *range_len, void *dst_base, uint64_t dst_cap, uint64_t *dst_off, int32_t *range_status,
                        chip_read_summary *summary, void *stream);

/* ---- LZ4: blocks and frames (additive API, decoding) ---------------------- */

/*
 * CHIP_FMT_LZ4_BLOCK (102): a unit is ONE raw block of the LZ4 block format, delimited by in_len[i]; no prefix, no dictionary.
 * CHIP_FMT_LZ4 (103): a unit is ONE frame of the LZ4 frame format 1.6.x (magic 0x184D2204).
 * Both go to chip_decode_batch / _ex / _sizes / _host / _multi, one wave per unit.  CHIP_F_COMPU_STATUS and CHIP_F_MEMBERS with
 * either tag: CHIP_E_INVALID before the device is looked for (compu has no LZ4 to mirror; concatenated frames are the caller's
 * loop).  chip_detect / CHIP_FMT_DETECT never route to them, the streaming decoders do not take them.  No reference counterpart.
 *
 * THE BLOCK RULES, which chip_lz4_block_decode_host defines (p: input cursor, o: bytes produced, len = in_len, cap = out_cap):
 *   sequence:  t = p (the token's offset)
 *     p == len                                   -> CHIP_NEED_INPUT      (so in_len == 0 is CHIP_NEED_INPUT)
 *     token = in[p++];  L = token >> 4;  if L == 15: add bytes while the byte just added was 255 (p == len there: CHIP_NEED_INPUT)
 *     L > len - p                                -> CHIP_NEED_INPUT      (the input is looked at before the room)
 *     L > cap - o                                -> CHIP_NEED_OUTPUT
 *     copy L literals;  o += L;  p += L
 *     p == len                                   -> CHIP_FINISHED        (the low nibble of this last token is not looked at)
 *     len - p < 2                                -> CHIP_NEED_INPUT
 *     offset = LE16(p);  p += 2
 *     offset == 0 or offset > o                  -> CHIP_LZ4_E_OFFSET    (before the match length's extension bytes are read)
 *     M = token & 15;  if M == 15: extension bytes as above (CHIP_NEED_INPUT where they end with the input);  M += 4
 *     M > cap - o                                -> CHIP_NEED_OUTPUT
 *     copy M bytes from o - offset, byte by byte in effect (offset < M repeats a period);  o += M
 * Lengths accumulate in 64 bits: no run of extension bytes wraps anything.  The end-of-block restrictions of the format document
 * (the last five bytes are literals, the last match starts 12 bytes before the end) are duties of encoders and are NOT enforced;
 * offsets are checked strictly.  The one-byte block 00 decodes to nothing.
 * On CHIP_FINISHED in_used == in_len.  On every other status in_used = t, the offset of the token of the sequence in which
 * decoding stopped, and out_len = o, the complete literal runs and matches in front of the run that stopped it (a literal run
 * that was copied counts, although its sequence did not finish).  Bytes between out_len and out_cap may have been used; nothing
 * beyond out_cap is touched.
 *
 * THE FRAME RULES, in the order of the checks (q: input cursor; every offset below is relative to the unit's first byte):
 *   len < 7                                      -> CHIP_NEED_INPUT
 *   LE32(0) != 0x184D2204                        -> CHIP_LZ4_E_HEADER    (the legacy magic 0x184C2102 and the skippable magics
 *                                                                         0x184D2A50..5F included: one unit is one frame)
 *   FLG = in[4], BD = in[5]:  version (FLG >> 6) != 1, FLG bit 1, BD bit 7 or BD bits 0..3 set, block maximum code
 *   (BD >> 4) & 7 outside 4..7                   -> CHIP_LZ4_E_HEADER
 *   hs = 7 + (C.Size ? 8 : 0) + (DictID ? 4 : 0);  len < hs -> CHIP_NEED_INPUT
 *   in[hs - 1] != (XXH32(in[4 .. hs - 1), 0) >> 8) & 0xff   -> CHIP_LZ4_E_HEADER
 *   DictID flag (FLG bit 0)                      -> CHIP_LZ4_E_DICT      (there are no dictionaries here)
 *   block maximum = 64 KiB, 256 KiB, 1 MiB, 4 MiB for the codes 4..7;  q = hs
 *   per block, b = q:
 *     len - q < 4                                -> CHIP_NEED_INPUT
 *     w = LE32(q);  w == 0: the EndMark, q += 4, the blocks are done
 *     size = w & 0x7fffffff > block maximum      -> CHIP_LZ4_E_BLOCK_SIZE  (compressed or stored)
 *     len - q - 4 < size + (B.Checksum ? 4 : 0)  -> CHIP_NEED_INPUT
 *     stored (w bit 31): size > cap - o -> CHIP_NEED_OUTPUT; the bytes are copied
 *     compressed: the block rules over in[q + 4 .. + size), where an offset may reach as far as the block's own first byte
 *       (B.Indep) or the frame's first byte (linked blocks; at most 65 535 back, the field's range), with these changes:
 *       a literal run or match that takes the block beyond the block maximum -> CHIP_LZ4_E_BLOCK_SIZE (looked at before the
 *       room), and what is CHIP_NEED_INPUT for a lone block is CHIP_LZ4_E_BLOCK here (the block's bytes are all present)
 *     B.Checksum: LE32 behind the block != XXH32(the block's `size` bytes as they lie in the file, 0) -> CHIP_LZ4_E_BLOCK_CHECKSUM
 *     q += 4 + size (+ 4)
 *   C.Checksum and len - q < 4                   -> CHIP_NEED_INPUT
 *   C.Size and the stated size != o              -> CHIP_LZ4_E_CONTENT_SIZE
 *   C.Checksum and LE32(q) != XXH32(content, 0)  -> CHIP_LZ4_E_CONTENT_CHECKSUM
 *   CHIP_FINISHED, in_used = the frame's length; bytes behind the frame are trailing bytes and are not counted.
 * Where the issue is one element's, the checks of that element run in the order written, elements front to back: a frame whose
 * second block is damaged and whose fourth is cut off answers for the second.
 * out_len: the content in front of the error -- on CHIP_NEED_OUTPUT, CHIP_LZ4_E_BLOCK, _OFFSET and _BLOCK_SIZE inside a block the
 * complete runs and matches in front of the one that failed (earlier blocks in full); on CHIP_LZ4_E_BLOCK_CHECKSUM the blocks in
 * front of the block whose checksum is wrong; on CHIP_LZ4_E_CONTENT_SIZE and CHIP_LZ4_E_CONTENT_CHECKSUM the whole content.
 * in_used on anything but CHIP_FINISHED: the offset of the element in which decoding stopped -- 0 for the frame header, b for a
 * block (its 4-byte header; the EndMark's offset when the content checksum behind it is cut off), and the frame's length for
 * CHIP_LZ4_E_CONTENT_SIZE and CHIP_LZ4_E_CONTENT_CHECKSUM, which are found behind its last byte.
 * The size pass (chip_decode_batch_sizes) keeps its four contract rules: every check above except the two XXH32 comparisons of
 * blocks and content (the header checksum IS checked); a stated content size is not trusted, the blocks are walked.
 */
enum {
    CHIP_LZ4_E_HEADER = -200,
    CHIP_LZ4_E_DICT = -201,
    CHIP_LZ4_E_BLOCK_SIZE = -202,
    CHIP_LZ4_E_BLOCK = -203,
    CHIP_LZ4_E_OFFSET = -204,
    CHIP_LZ4_E_BLOCK_CHECKSUM = -205,
    CHIP_LZ4_E_CONTENT_SIZE = -206,
    CHIP_LZ4_E_CONTENT_CHECKSUM = -207
};

/* The block rules on HOST memory, and their definition: returns the status (CHIP_FINISHED, CHIP_NEED_INPUT, CHIP_NEED_OUTPUT,
 * CHIP_LZ4_E_OFFSET), or CHIP_E_INVALID for a NULL out_len / in_used, a NULL `in` with len > 0 or a NULL `out` with cap > 0.
 * len and cap are at most 2^32 - 1 (CHIP_E_INVALID), as a unit's are.  Pure host arithmetic. */
int chip_lz4_block_decode_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used);

/*
 * The blocks of the FIRST frame of a buffer, from its headers alone, with chip_zstd_blocks' conventions.  The walk of `len` bytes:
 *     len < 7 -> TRUNCATED;  the header checks of the frame rules: CHIP_LZ4_E_HEADER and CHIP_LZ4_E_DICT -> BAD_HEADER,
 *     CHIP_NEED_INPUT -> TRUNCATED;  q = hs;  n = 0
 *     per block:  len - q < 4 -> TRUNCATED;  w = LE32(q);  w == 0 -> the EndMark: the block before it gets CHIP_LZ4BLOCK_LAST, q += 4
 *                 size = w & 0x7fffffff > block_max -> BAD_HEADER;  n + 1 > CHIP_ZPLAN_MAX_BLOCKS -> TOO_LARGE
 *                 len - q - 4 < size + (B.Checksum ? 4 : 0) -> TRUNCATED
 *                 block n: offset = q, size, flags = (w >> 31) ? CHIP_LZ4BLOCK_STORED : 0, checksum = the LE32 behind it or 0
 *                 n++;  q += 4 + size (+ 4)
 *     C.Checksum: len - q < 4 -> TRUNCATED;  content_checksum = LE32(q);  q += 4
 *     in_used = q, status CHIP_ZPLAN_OK
 * A walk that stops early keeps the blocks it has counted, with in_used = 0.  Nothing is decoded, no checksum but the header's is
 * compared.  `blocks` receives the first min(n_blocks, max_blocks) records: max_blocks = 0 with a NULL array counts, a second call
 * fills (CHIP_LZ4BLOCK_LAST is set only on a record that is written).  status: CHIP_ZPLAN_OK, _TRUNCATED, _BAD_HEADER, _TOO_LARGE.
 * flg, bd, header_bytes (hs), block_max and content_size are filled once the header has been accepted, else 0 /
 * CHIP_LZ4BLOCKS_UNSIZED.  CHIP_E_INVALID, before the device is looked for: summary NULL, a NULL buffer with len > 0, a NULL array
 * with max_blocks > 0 (chip_lz4_blocks: in_base not 4-byte aligned, len > 2^40).
 */
#define CHIP_LZ4BLOCKS_UNSIZED 0xFFFFFFFFFFFFFFFFull /* content_size of a frame without C.Size */
enum { CHIP_LZ4BLOCK_STORED = 1, CHIP_LZ4BLOCK_LAST = 2 };
typedef struct {
    uint64_t offset;   /* of the block's 4-byte header in the buffer */
    uint32_t size;     /* the bytes behind the header: compressed, or stored as they are */
    uint32_t flags;    /* CHIP_LZ4BLOCK_* */
    uint32_t checksum; /* the stored block checksum (B.Checksum), else 0 */
    uint32_t pad;
} chip_lz4_block;
typedef struct {
    uint64_t n_blocks, in_used, content_size;
    uint32_t block_max, flg, bd, header_bytes;
    uint32_t content_checksum; /* the stored one (C.Checksum, status OK), else 0 */
    int32_t status;
} chip_lz4_blocks_summary;
int chip_lz4_blocks_host(const uint8_t *in, uint64_t len, uint64_t max_blocks, chip_lz4_block *blocks, chip_lz4_blocks_summary *summary);
/* The same for DEVICE memory: in_base and blocks are DEVICE pointers, summary is a HOST pointer; in_base 4-byte aligned, its
 * allocation padded to a multiple of 4.  One lane hops over the block headers.  SYNCHRONOUS on `stream` (one wait); a launch
 * slot of its own (the summary only), released by chip_trim(). */
int chip_lz4_blocks(const void *in_base, uint64_t len, uint64_t max_blocks, chip_lz4_block *blocks, chip_lz4_blocks_summary *summary,
                    void *stream);

/* XXH32 of many ranges of DEVICE memory, chip_xxh64_batch's sibling: digest[i] = XXH32 with `seed` of base[off[i] .. + len[i]).
 * Every pointer is a DEVICE pointer, off[i] may have any alignment; it only enqueues on `stream`: no wait, no scratch.  One wave
 * hashes one range, and XXH32 is one serial chain per range.  CHIP_E_INVALID, before the device is looked for: a NULL array or
 * base with n > 0, n > 2^31 - 1.  n == 0: CHIP_OK, the device is not touched. */
int chip_xxh32_batch(size_t n, const void *base, const uint64_t *off, const uint32_t *len, uint32_t seed, uint32_t *digest, void *stream);

/*
 * ONE large LZ4 frame decoded by the whole GPU, a wave per block, with chip_zstd_parallel's conventions: in_base and out_base are
 * DEVICE pointers, in_base 4-byte aligned and its allocation padded to a multiple of 4; summary is a HOST pointer; SYNCHRONOUS on
 * `stream`; scratch in a launch slot of its own (80 bytes per block: its record and its unit arrays), released by chip_trim().  Only the
 * FIRST frame of the buffer is decoded; in_used says where it ended.
 * path = CHIP_LZ4PAR_PARALLEL when: the walk (chip_lz4_blocks) is OK; B.Indep is set; the frame has at least two blocks; the size
 * pass over the compressed blocks (a CHIP_FMT_LZ4_BLOCK batch) answers CHIP_FINISHED for each with at most block_max bytes; a
 * stated content size equals the counted one; every block checksum and the content checksum match (the latter unless waived).  The passes: the walk; the size pass; a device scan for the layout (chip_layout_units); the block batch straight
 * into out_base; stored blocks placed by the file writer's copy; the block checksums by the XXH32 batch; the content checksum on
 * one wave.  The bytes, out_len, in_used and status (CHIP_FINISHED) are those of chip_decode_batch(CHIP_FMT_LZ4, 1, ..).
 * The same with total_out > out_cap: CHIP_NEED_OUTPUT, out_len = 0, total_out the exact size to come back with; nothing is
 * written and no checksum is compared (the call that has the room compares them).
 * Anything else, a linked-block frame and a checksum mismatch included: path = CHIP_LZ4PAR_SERIAL and the answer is the one-unit
 * CHIP_FMT_LZ4 decode's, status and out_len included -- that decode is the arbiter of every verdict (after a mismatch it writes
 * the bytes again) -- if a unit can hold the frame (len and out_cap at most 2^32 - 1); else path = CHIP_LZ4PAR_REFUSED and nothing
 * is written.
 * CHIP_LZ4PAR_NO_CHECKSUM: on the parallel path the content checksum is read over, not compared (XXH32 is one serial chain: one
 * wave hashes the whole content); block checksums are still compared.  The one deliberate difference from the batch.
 * summary.check: the content checksum computed on the parallel path, else 0.
 * CHIP_E_INVALID before the device is looked for: summary NULL, a NULL buffer with a length, in_base misaligned, unknown flag
 * bits, len > 2^40.
 */
enum { CHIP_LZ4PAR_SERIAL = 0, CHIP_LZ4PAR_PARALLEL = 1, CHIP_LZ4PAR_REFUSED = 2 };
#define CHIP_LZ4PAR_NO_CHECKSUM 1u /* flags: do not verify the content checksum on the parallel path */
typedef struct {
    uint64_t n_blocks, out_len, in_used, total_out;
    int32_t status;
    uint32_t path, check, pad;
} chip_lz4_parallel_summary;
int chip_lz4_parallel(const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, uint32_t flags,
                      chip_lz4_parallel_summary *summary, void *stream);

/* ---- LZ4: encoding (additive API) ------------------------------------------ */

/*
 * chip_encode_batch[_ex], chip_encode_batch_host and chip_encode_bound take CHIP_FMT_LZ4_BLOCK and CHIP_FMT_LZ4; chip_encode_file
 * takes CHIP_FMT_LZ4.  No reference counterpart: compu has no LZ4.  This is the library's own match finder, not liblz4's: the
 * bytes differ from liblz4's, and every conformant decoder reads them.
 *
 * level: -1 .. 12, the `lz4` command's range (-1 and 0 mean 1); anything else is CHIP_E_INVALID.  Three finder groups:
 *   1 - 2    greedy, one position per hash slot, a growing skip over incompressible stretches (level 1 grows it faster)
 *   3 - 5    greedy, two positions per slot
 *   6 - 12   two positions per slot and a one-step lazy choice (a match gives way to a longer one at the next position)
 *
 * THE DUTIES of a block, which liblz4's decoders rely on and every block written here keeps:
 *   the last 5 bytes are literals; no match starts within the last 12 bytes; a block of fewer than 13 bytes is one literal run;
 *   offsets are 1 .. 65 535 (never 0, never 65 536); no offset reaches in front of the block (independent blocks only, no
 *   dictionary); empty input is the one byte 0x00.
 *
 * CHIP_FMT_LZ4_BLOCK: a unit becomes ONE raw block.  strategy must be 0.  status[i] = CHIP_ENC_FINISHED with out_len[i], or
 * CHIP_ENC_NEED_OUTPUT (out_len 0) when out_cap[i] is too small -- no byte is stored at or past out_cap[i] -- or CHIP_ENC_ERROR for
 * in_len[i] > 0x7E000000 (LZ4_MAX_INPUT_SIZE).  chip_encode_bound = n + n / 255 + 16, the format's own worst case.
 *
 * CHIP_FMT_LZ4: a unit becomes ONE frame of the frame format 1.6.x, written by one wave block after block: version 01,
 * independent blocks, Content_Size always stated, the end mark, and by default a 64 KiB block maximum (BD id 4), the content
 * checksum and no block checksums.  A block that does not come out smaller than its content is stored (high bit of its header).
 * An empty unit is header + end mark (+ the checksum of nothing).  strategy carries the options as bits: CHIP_LZ4_S_BLOCK_CHECKSUM,
 * CHIP_LZ4_S_NO_CONTENT_CHECKSUM and a block-size id (0 = default, else 4 .. 7 = 64 KiB, 256 KiB, 1 MiB, 4 MiB) shifted by
 * CHIP_LZ4_S_BLOCK_ID_SHIFT; any other value is CHIP_E_INVALID.  Statuses as for blocks.
 * chip_encode_bound = n + 8 * ceil(n / 65 536) + 23: the 15-byte header, the end mark and the content checksum, and around every
 * stored 64 KiB block a header and a block checksum -- it covers every option (larger blocks only need less).
 *
 * chip_lz4_block_encode_host and chip_lz4_frame_encode_host are the host forms and THE DEFINITION OF THE BYTES: the kernels write
 * the same bytes for every input, level and option (one source, compu_amd/csrc/lz4_enc_core.h).  in, out, out_len are HOST
 * pointers.  They answer CHIP_ENC_FINISHED (*out_len = the size), CHIP_ENC_NEED_OUTPUT (cap too small, *out_len = 0; nothing is
 * stored at or past cap), CHIP_ENC_ERROR (len > 0x7E000000) or CHIP_E_INVALID (out_len NULL, a NULL buffer with a length, a level
 * or strategy out of range).
 *
 * chip_encode_file(CHIP_FMT_LZ4, ..) writes ONE frame across the GPU, the counterpart of chip_lz4_parallel and what the `lz4`
 * command writes: the 15-byte header (Content_Size always), one block per unit, the end mark.  unit_bytes is the block maximum: 0
 * (= 65 536), 65 536, 262 144, 1 048 576 or 4 194 304; anything else is CHIP_E_INVALID.  flags, valid with this format only:
 * CHIP_W_LZ4_CONTENT_CHECKSUM and CHIP_W_LZ4_BLOCK_CHECKSUM.  The content checksum is OFF by default here: XXH32 is one serial chain
 * that one wave runs over the whole input (0.57 GB/s measured for the decode side).
 * The passes, on the caller's stream: the units are cut; a CHIP_FMT_LZ4_BLOCK batch encodes them into slots; a block with
 * out_len >= in_len is stored; chip_xxh32_batch hashes every block's bytes as they will lie in the file (block checksums); a scan
 * lays the blocks out; ONE destination-driven copy takes each block from its slot or from the input; small kernels write the
 * block headers and checksums, the frame header, the end mark and the content checksum.  The blocks are the bytes of
 * chip_lz4_block_encode_host.  len == 0: the empty frame (n_units = 0).  summary.table_off = out_len.  chip_encode_file_bound =
 * 15 + len + n * (4 + 4 with block checksums) + 4 + (4 with the content checksum), n = ceil(len / unit_bytes).
 */
enum { CHIP_LZ4_S_BLOCK_CHECKSUM = 1, CHIP_LZ4_S_NO_CONTENT_CHECKSUM = 2, CHIP_LZ4_S_BLOCK_ID_SHIFT = 4, CHIP_LZ4_S_BLOCK_ID_MASK = 0x70 };
enum { CHIP_W_LZ4_CONTENT_CHECKSUM = 2, CHIP_W_LZ4_BLOCK_CHECKSUM = 4 };
int chip_lz4_block_encode_host(const uint8_t *in, uint64_t len, int level, uint8_t *out, uint64_t cap, uint64_t *out_len);
int chip_lz4_frame_encode_host(const uint8_t *in, uint64_t len, int level, int strategy, uint8_t *out, uint64_t cap, uint64_t *out_len);

/* ---- Snappy: blocks and framed streams (additive API, decoding) -------------- */

/*
 * CHIP_FMT_SNAPPY_BLOCK (104): a unit is ONE raw block of the Snappy format (format_description.txt): a varint preamble that states
 * the decoded length, then elements; delimited by in_len[i].  What snappy::RawCompress writes and a Parquet / ORC / Avro page holds.
 * CHIP_FMT_SNAPPY (105): a unit is ONE stream of the Snappy framing format (framing_format.txt, a .sz file), delimited by
 * in_len[i]: the format has no end mark.
 * Both go to chip_decode_batch / _ex / _sizes / _host / _multi, one wave per unit.  Flags must be 0: CHIP_F_COMPU_STATUS and
 * CHIP_F_MEMBERS with either tag are CHIP_E_INVALID before the device is looked for.  chip_detect / CHIP_FMT_DETECT never route to
 * them, the streaming objects do not take them, every encode entry point refuses them.  No reference counterpart.
 *
 * THE BLOCK RULES, which chip_snappy_block_decode_host defines (p: input cursor, o: bytes produced, len = in_len, cap = out_cap):
 *   preamble: n = little-endian varint of at most 5 bytes
 *     the input ends inside it (len == 0 included)  -> CHIP_NEED_INPUT
 *     5th byte >= 16                                -> CHIP_SNAPPY_E_PREAMBLE  (the continuation bit set, or more than 32 bits)
 *     non-minimal forms such as 80 00 are valid
 *     n > cap                                       -> CHIP_NEED_OUTPUT, out_len = 0, in_used = 0, nothing written
 *       (so the decode never needs a room check per element: o <= n <= cap)
 *   per element, t = p:
 *     p == len                                      -> o == n ? CHIP_FINISHED : CHIP_NEED_INPUT
 *     o == n (bytes remain)                         -> CHIP_SNAPPY_E_LENGTH    (every element produces at least one byte)
 *     tag = in[p++]
 *     literal (tag & 3 == 0):
 *       L = tag >> 2;  L >= 60: nb = L - 59;  len - p < nb -> CHIP_NEED_INPUT;  L = LE(nb bytes);  p += nb
 *       L += 1  (in 64 bits: the 4-byte form ff ff ff ff is 2^32 and wraps nothing)
 *       L > len - p                                 -> CHIP_NEED_INPUT         (the input is looked at before the length)
 *       L > n - o                                   -> CHIP_SNAPPY_E_LENGTH
 *       copy L bytes;  o += L;  p += L
 *     copy:
 *       tag & 3 == 1: 1 more byte,  M = 4 + ((tag >> 2) & 7), offset = ((tag >> 5) << 8) | byte
 *       tag & 3 == 2: 2 more bytes, M = (tag >> 2) + 1, offset = LE16
 *       tag & 3 == 3: 4 more bytes, M = (tag >> 2) + 1, offset = LE32
 *       the bytes are missing                       -> CHIP_NEED_INPUT
 *       offset == 0 or offset > o                   -> CHIP_SNAPPY_E_OFFSET
 *       M > n - o                                   -> CHIP_SNAPPY_E_LENGTH
 *       copy M bytes from o - offset, byte by byte in effect (offset < M repeats a period);  o += M
 * On CHIP_FINISHED in_used == in_len.  On every other status in_used = t, the offset of the tag of the element in which decoding
 * stopped (0 inside the preamble), and out_len = o, the complete elements in front of it.  Nothing beyond out_cap is touched.  The
 * one-byte block 00 decodes to nothing.
 *
 * THE FRAME RULES, in the order of the checks (q: input cursor).  A chunk is 1 type byte, a 3-byte little-endian length s of what
 * follows, and those s bytes:
 *   len < 4                                         -> CHIP_NEED_INPUT
 *   the first chunk is not ff 06 00 00 "sNaPpY"     -> CHIP_SNAPPY_E_HEADER  (cut inside it: CHIP_NEED_INPUT, unless the bytes
 *                                                                            that are present already differ)
 *   per chunk, b = q:
 *     q == len                                      -> CHIP_FINISHED, in_used = len
 *     len - q < 4, or len - q - 4 < s               -> CHIP_NEED_INPUT
 *     type ff: s != 6 or the six bytes differ       -> CHIP_SNAPPY_E_HEADER;  else stepped over (concatenated streams)
 *     type fe (padding) and 80..fd (skippable): stepped over
 *     type 02..7f (reserved, unskippable)           -> CHIP_SNAPPY_E_CHUNK
 *     type 00 (compressed) and 01 (uncompressed):  s < 4 -> CHIP_SNAPPY_E_CHUNK_SIZE;  c = LE32(q + 4)
 *       01: s - 4 > 65536                           -> CHIP_SNAPPY_E_CHUNK_SIZE
 *           s - 4 > cap - o                         -> CHIP_NEED_OUTPUT
 *           the bytes are copied
 *       00: the block rules over the s - 4 bytes behind the CRC, with these changes:
 *           a preamble n > 65536                    -> CHIP_SNAPPY_E_CHUNK_SIZE
 *           n > cap - o                             -> CHIP_NEED_OUTPUT
 *           what is CHIP_NEED_INPUT for a lone block -> CHIP_SNAPPY_E_BLOCK  (the chunk's bytes are all present)
 *       mask(CRC-32C(the chunk's content)) != c     -> CHIP_SNAPPY_E_CHECKSUM;  mask(x) = ((x >> 15) | (x << 17)) + 0xa282ead8
 *     q += 4 + s
 * On anything but CHIP_FINISHED in_used = b, the offset of the chunk in which decoding stopped (0 for the first).  out_len: the
 * chunks in front in full; inside a failing block also that block's complete elements; on CHIP_SNAPPY_E_CHECKSUM the failing
 * chunk's content is not counted.
 * The size pass (chip_decode_batch_sizes): every verdict above depends on positions, never on decoded bytes, so the pass is the
 * parse without the copies and exact on every unit; it is blind only to the CRC-32C comparison (rule 4 of its contract).  The
 * preamble is not trusted: the elements are walked.
 */
enum {
    CHIP_SNAPPY_E_PREAMBLE = -210,
    CHIP_SNAPPY_E_OFFSET = -211,
    CHIP_SNAPPY_E_LENGTH = -212,
    CHIP_SNAPPY_E_HEADER = -213,
    CHIP_SNAPPY_E_CHUNK = -214,
    CHIP_SNAPPY_E_CHUNK_SIZE = -215,
    CHIP_SNAPPY_E_BLOCK = -216,
    CHIP_SNAPPY_E_CHECKSUM = -217
};

/* The block rules on HOST memory, and their definition: returns the status (CHIP_FINISHED, CHIP_NEED_INPUT, CHIP_NEED_OUTPUT,
 * CHIP_SNAPPY_E_PREAMBLE, _OFFSET, _LENGTH), or CHIP_E_INVALID for a NULL out_len / in_used, a NULL `in` with len > 0 or a NULL
 * `out` with cap > 0.  len and cap are at most 2^32 - 1 (CHIP_E_INVALID), as a unit's are.  Pure host arithmetic. */
int chip_snappy_block_decode_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used);

/*
 * The DATA chunks of a framed buffer, from the chunk headers alone, with chip_lz4_blocks' conventions.  The walk of `len` bytes:
 *     the first chunk as in the frame rules: len < 4 or cut inside the identifier -> TRUNCATED, another first chunk -> BAD_HEADER
 *     per chunk, b = q:  q == len -> status CHIP_ZPLAN_OK, in_used = len
 *                 len - q < 4 or len - q - 4 < s -> TRUNCATED
 *                 type ff that is not the identifier, types 02..7f, types 00 / 01 with s < 4 -> BAD_HEADER
 *                 types ff, fe, 80..fd: n_skipped + 1 > CHIP_ZPLAN_MAX_BLOCKS -> TOO_LARGE;  n_skipped++ (the first identifier is
 *                 not counted)
 *                 types 00 / 01: n_chunks + 1 > CHIP_ZPLAN_MAX_BLOCKS -> TOO_LARGE;  chunk n: offset = b, size = s, type, crc = the
 *                 stored (masked) LE32;  n_chunks++
 *                 q += 4 + s
 * A walk that stops early keeps what it has counted, with in_used = b: the chunks in front of b are whole.  Nothing deeper is
 * looked at: no chunk-size limit, no preamble, no CRC.  `chunks` receives the first min(n_chunks, max_chunks) records:
 * max_chunks = 0 with a NULL array counts, a second call fills.  CHIP_E_INVALID, before the device is looked for: summary NULL, a
 * NULL buffer with len > 0, a NULL array with max_chunks > 0 (chip_snappy_chunks: in_base not 4-byte aligned, len > 2^40).
 */
typedef struct {
    uint64_t offset; /* of the chunk's 4-byte header in the buffer */
    uint32_t size;   /* s: the bytes behind the header, the 4 CRC bytes included */
    uint32_t type;   /* 0 compressed, 1 uncompressed */
    uint32_t crc;    /* the stored, masked CRC-32C of the content */
    uint32_t pad;
} chip_snappy_chunk;
typedef struct {
    uint64_t n_chunks, n_skipped, in_used;
    int32_t status; /* CHIP_ZPLAN_OK, _TRUNCATED, _BAD_HEADER, _TOO_LARGE */
    uint32_t pad;
} chip_snappy_chunks_summary;
int chip_snappy_chunks_host(const uint8_t *in, uint64_t len, uint64_t max_chunks, chip_snappy_chunk *chunks, chip_snappy_chunks_summary *summary);
/* The same for DEVICE memory: in_base and chunks are DEVICE pointers, summary is a HOST pointer; in_base 4-byte aligned, its
 * allocation padded to a multiple of 4.  One lane hops over the chunk headers.  SYNCHRONOUS on `stream` (one wait); a launch slot
 * of its own (the summary only), released by chip_trim(). */
int chip_snappy_chunks(const void *in_base, uint64_t len, uint64_t max_chunks, chip_snappy_chunk *chunks, chip_snappy_chunks_summary *summary,
                       void *stream);

/* CRC-32C (Castagnoli, reflected polynomial 0x82F63B78, initial value and final inversion 0xFFFFFFFF) of many ranges of DEVICE
 * memory, chip_xxh32_batch's sibling: crc[i] = CRC-32C of base[off[i] .. + len32[i]).  UNMASKED: the value iSCSI and ext4 store; the
 * Snappy framing format stores mask() of it (above).  Every pointer is a DEVICE pointer, off[i] may have any alignment; it only
 * enqueues on `stream`: no wait, no scratch.  One wave per range (its 64 lanes take 64 pieces and combine them), so one huge range
 * runs at one wave's rate: only many ranges fill the card.  CHIP_E_INVALID, before the device is looked for: a NULL array or base
 * with n > 0, n > 2^31 - 1.  n == 0: CHIP_OK, the device is not touched. */
int chip_crc32c_batch(size_t n, const void *base, const uint64_t *off, const uint32_t *len32, uint32_t *crc, void *stream);

/*
 * ONE framed stream decoded with a wave per chunk, with chip_lz4_parallel's conventions: in_base and out_base are DEVICE pointers,
 * in_base 4-byte aligned and its allocation padded to a multiple of 4; summary is a HOST pointer; SYNCHRONOUS on `stream`; scratch
 * in a launch slot of its own (80 bytes per chunk: its record and its unit arrays), released by chip_trim().  flags must be 0.  A
 * chunk holds at most 65 536 bytes of content and never refers to another, so the stream is a batch by construction.
 * The passes, all on `stream`: the walk (chip_snappy_chunks); the size pass over the compressed chunks as CHIP_FMT_SNAPPY_BLOCK
 * units (an uncompressed chunk is an empty unit that gets its size from s), and one thread per chunk that counts the chunks that
 * did not finish or exceed 65 536 bytes; chip_layout_units; the block batch straight into out_base; the uncompressed chunks by the
 * file writer's copy; chip_crc32c_batch over the content ranges, compared by one thread per chunk.
 * path = CHIP_SNAPPYPAR_PARALLEL when the walk is OK, there are at least two data chunks and every pass is clean: the bytes,
 * out_len, in_used and status (CHIP_FINISHED) are those of chip_decode_batch(CHIP_FMT_SNAPPY, 1, ..).  The same with
 * total_out > out_cap: CHIP_NEED_OUTPUT, out_len = 0, total_out the exact size to come back with; nothing is written and no CRC is
 * compared (the call that has the room compares them).
 * Anything else: path = CHIP_SNAPPYPAR_SERIAL and the answer is the one-unit CHIP_FMT_SNAPPY decode's of the same buffer, status
 * and out_len included -- that decode is the arbiter of every verdict -- if a unit can hold the buffer (len and out_cap at most
 * 2^32 - 1); else path = CHIP_SNAPPYPAR_REFUSED and nothing is written.
 * CHIP_E_INVALID before the device is looked for: summary NULL, a NULL buffer with a length, in_base misaligned, flags != 0,
 * len > 2^40.
 */
enum { CHIP_SNAPPYPAR_SERIAL = 0, CHIP_SNAPPYPAR_PARALLEL = 1, CHIP_SNAPPYPAR_REFUSED = 2 };
typedef struct {
    uint64_t n_chunks, out_len, in_used, total_out;
    int32_t status;
    uint32_t path, n_skipped, pad;
} chip_snappy_parallel_summary;
int chip_snappy_parallel(const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, uint32_t flags,
                         chip_snappy_parallel_summary *summary, void *stream);

/* ---- one large stream: the checkpoint index (additive API) ------------------ */

/*
 * The commonest compressed file is ONE gzip member, or one zlib or raw deflate stream, and a stream is decoded by one wave from its
 * first bit to its last.  The answer of zran.c, indexed_gzip and `bgzip -r`: decode once and keep a checkpoint every so many bytes
 * -- the bit position of a block boundary and the 32 KiB of content in front of it.  Every stretch between two checkpoints is then
 * an independent unit: a second read of the file is a batch, and bytes [lo, lo + n) cost the chunks they touch.
 *
 * chip_inflate_index_build IS a decode.  in_base[0 .. len) is one unit (chip_decode_batch's alignment and padding rules), `format`
 * CHIP_FMT_DEFLATE, CHIP_FMT_ZLIB, CHIP_FMT_GZIP or CHIP_FMT_AUTO, out_base[0 .. out_cap) its room.  The bytes written to
 * out_base and summary->out_len, in_used and status are exactly what chip_decode_batch(format, 1, ..) answers for the same unit and
 * room (flags 0): CHIP_NEED_OUTPUT, CHIP_NEED_INPUT, CHIP_NEED_DICT and the negative codes alike.  wrap = 0 raw, 1 zlib, 2 gzip.
 * With status CHIP_FINISHED, check = the CRC-32 (gzip) / Adler-32 (zlib) of the whole content (0 for raw) and end_bit = the bit
 * behind the final block's end-of-block code; else both are 0.
 * The points are DEFINED by this walk.  The decoder reaches the boundaries of blocks b_0, b_1, .. each at the top of its block
 * loop; s_j = the bit offset of block j's header counted from in_base byte 0, o_j = the decoded bytes in front of block j.
 *   point 0 = (s_0, 0)
 *   boundary j >= 1 is a point if and only if o_j - o_(the last point) >= spacing
 * spacing == 0 means 1 MiB (zran's convention); any spacing >= 1 is allowed, so a boundary with no new output is never a point.
 * Boundaries reached before the room or the input ran out count.  A unit whose wrapper is refused has n_points = 0.
 * n_points counts the WHOLE walk; pt_bit, pt_out, pt_check and windows receive the first min(n_points, max_points) points and
 * nothing behind them is written: max_points = 0 with null arrays is the plain decode with a count.  A truncated index is still a
 * valid index, its last chunk is just long.  Per point k:
 *   pt_bit[k]   = s_j           pt_out[k] = o_j
 *   pt_check[k] = the CRC-32 (gzip) / Adler-32 (zlib) of content[0 .. pt_out[k]), 0 for raw deflate
 *   windows + 32768 * k: the first wl_k = min(32768, pt_out[k]) bytes are content[pt_out[k] - wl_k .. pt_out[k]); the rest of the
 *   slot is not written
 * SYNCHRONOUS on `stream` (it waits for the point count, then for the summary).  summary is a HOST pointer, everything else DEVICE
 * memory.  CHIP_E_INVALID, before the device is looked for: summary, in_base or out_base NULL; in_base not 4-byte aligned; a format
 * other than the four; len > CHIP_GZPLAN_WINDOW; out_cap > 2^32 - 16; a NULL array with max_points > 0.  Scratch per (device,
 * stream), a launch slot of its own, released by chip_trim(): the token rows of one wave (60 KiB).  The calling thread's current
 * device is left as it was.  The first pass stays one wave: this call costs what chip_decode_batch costs for the unit, plus one
 * more read of the output for the checks.
 */
typedef struct {
    uint64_t n_points, out_len, in_used, end_bit;
    int32_t status;
    uint32_t wrap, check, pad;
} chip_inflate_index_summary;
int chip_inflate_index_build(int format, const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, uint32_t spacing,
                             uint64_t max_points, uint64_t *pt_bit, uint64_t *pt_out, uint32_t *pt_check, void *windows,
                             chip_inflate_index_summary *summary, void *stream);

/*
 * The chunks of an index, on HOST arrays: pure arithmetic, no device.  `format` is CHIP_FMT_DEFLATE, CHIP_FMT_ZLIB or
 * CHIP_FMT_GZIP (the build's wrap 0, 1, 2).  Chunk k runs from point k to point k + 1, the last one to the end of the stream:
 *   end_out = k + 1 < n_points ? pt_out[k + 1] : total_out          out_cap[k] = end_out - pt_out[k]
 *   end_in  = k + 1 < n_points ? ceil(pt_bit[k + 1] / 8) : len
 *   in_off[k] = pt_bit[k] >> 3, one byte less when pt_bit[k] is a multiple of 8 and not 0;   in_len[k] = end_in - in_off[k]
 *   win_len[k] = wl_k = min(32768, pt_out[k])
 *   resume[6 k ..] = { pt_bit[k] - 8 * in_off[k], wl_k, wrap, pt_check[k], pt_out[k], pt_out[k] - wl_k }     (low 32 bits)
 * The inflate kernel reads resume word 0 == 0 as "from the start", hence the byte in front of a byte-aligned point; bit 0, point 0
 * of a raw stream, IS the start.  The smallest block (a fixed block of only its end-of-block code) is 10 bits and at most 7 bits
 * trail the next boundary inside a chunk's input: a chunk cannot reach a boundary behind its own end.
 * Layout check: chunk k OFFENDS when (k == 0 and pt_out[0] != 0), or pt_bit[k] >= 8 * len, or k + 1 < n_points and pt_bit[k + 1] <=
 * pt_bit[k], or end_out < pt_out[k], or out_cap[k] > 2^32 - 16 - 32768, or in_len[k] > CHIP_GZPLAN_WINDOW.  Any offender:
 * *status = CHIP_READ_BAD_LAYOUT, *bad_index = the lowest such k, and no array is written.  Else *status = CHIP_READ_OK, *bad_index
 * = 0.  Each of the five arrays may be NULL (not wanted).  CHIP_E_INVALID: status or bad_index NULL, a point array NULL with
 * n_points > 0, another format, n_points > 2^32 - 1.
 */
int chip_inflate_index_units_host(int format, uint64_t len, uint64_t n_points, const uint64_t *pt_bit, const uint64_t *pt_out,
                                  const uint32_t *pt_check, uint64_t total_out, uint64_t *in_off, uint32_t *in_len, uint32_t *out_cap,
                                  uint32_t *win_len, uint32_t *resume, int32_t *status, uint64_t *bad_index);

/*
 * chip_read_ranges through an index: the units are the chunks above (out_off = pt_out), the arrays of the index and `windows` are
 * DEVICE memory as the build left them, in_base[0 .. len) is the stream and total_out its decoded length (the build's out_len).
 * n_ranges == 0: CHIP_OK, an all-zero summary.  Layout check as above: status = CHIP_READ_BAD_LAYOUT, bad_index = the lowest
 * offending k, nothing is decoded or written.  Selection, dst_off, CHIP_RANGE_OUTSIDE, CHIP_READ_NEED_OUTPUT and the write rules
 * of dst_base are exactly chip_read_ranges' walk over those units.
 * Every selected chunk is decoded once, as a RESUMED unit of the batch decoder, into a scratch slot [window | chunk].  A chunk that
 * is not the last is GOOD if and only if its run ended CHIP_NEED_INPUT or CHIP_NEED_OUTPUT at the boundary pt_bit[k + 1] with
 * exactly the chunk's output and a running check equal to pt_check[k + 1]; the last chunk if and only if it ended CHIP_FINISHED
 * with exactly its output (the kernel has then compared the trailer's check, and gzip's ISIZE, itself).  By induction over these
 * links a read of [0, total_out) with n_bad == 0 has verified the stream's own CRC-32 / Adler-32, whether or not the index is
 * trusted.  Bad chunks are reported as chip_read_ranges reports bad units: n_bad, first_bad (the chunk's k), bad_status (its decode
 * status) and CHIP_RANGE_BAD_UNIT for the ranges whose span holds one; every other range has its bytes.
 * SYNCHRONOUS on `stream`.  CHIP_E_INVALID, before the device is looked for: summary NULL; in_base NULL or not 4-byte aligned; a
 * format other than the three (CHIP_FMT_AUTO too: the build's wrap says which); len > 2^61; a point array or windows NULL with
 * n_points > 0; range_lo or range_len NULL with n_ranges > 0; dst_base NULL with dst_cap > 0; n_points or n_ranges above 2^32 - 1.
 * Scratch per (device, stream), a launch slot of its own: 132 bytes per chunk, 28 per range, and for the selection twice its
 * content plus 32 KiB per chunk (the slots, and the image the ranges are gathered from).  The calling thread's current device is
 * left as it was.  No wave waits for another: the chunks are independent units.
 */
int chip_inflate_index_read(int format, const void *in_base, uint64_t len, uint64_t n_points, const uint64_t *pt_bit,
                            const uint64_t *pt_out, const uint32_t *pt_check, const void *windows, uint64_t total_out, size_t n_ranges,
                            const uint64_t *range_lo, const uint32_t *range_len, void *dst_base, uint64_t dst_cap, uint64_t *dst_off,
                            int32_t *range_status, chip_read_summary *summary, void *stream);

/* ---- one large stream: block starts (additive API) ------------------------- */

/*
 * The first pass of a parallel decode of ONE stream: where, behind its beginning, may a wave start?  A deflate block can be decoded
 * from its first bit on by whoever knows that bit, and a dynamic block's header can be recognised without decoding what is in front
 * of it (pugz, rapidgzip).  These two calls look for such headers; they decode nothing, build no table and use no window.
 * A bit position p of in[0 .. len) (bit p = bit p % 8 of byte p / 8, as the index's pt_bit counts) is a CANDIDATE if and only if
 *   - the three bits at p are BFINAL = 0, BTYPE = 2;
 *   - the dynamic header that starts there is one the decoder's header path accepts: HLIT <= 29 and HDIST <= 29; a complete
 *     code-length code; the code-length sequence decodes within HLIT + HDIST + 258 entries by zlib's rules (no repeat of a previous
 *     length at entry 0, no run past the last entry); the end-of-block code has a length; the literal/length and the distance set
 *     are ones zlib's inflate_table accepts (not over-subscribed; incomplete only as a single code of length 1; a distance set
 *     without any code is accepted);
 *   - the header, to the last bit of its last code-length symbol, lies inside the buffer.
 * Stored blocks, fixed blocks and final blocks are never candidates.  With B = chunk_bytes, the START of chunk k, k = 1 ..
 * ceil(len / B) - 1, is the least candidate p with 8 k B <= p < 8 (k + 1) B and p > first_bit, or none.  first_bit is the bit of the
 * stream's first block header (the caller's to know: 0 for raw deflate, behind the wrapper else); chunk 0 has no start.
 * A candidate is not a promise.  Bits inside a block's data, and a stored block's payload, can spell a header; a decode that begins at a start has to be confirmed by the decode that arrives there from the front.
 * Every real boundary of a non-final dynamic block, on the other hand, IS a candidate, so a chunk that holds one has a start at or
 * in front of it.
 * starts receives, ascending, the starts of the chunks that have one: the first min(*n, max) of them, and nothing behind them is
 * written; *n counts them all.  max = 0 with a null array counts, a second call fills.
 * chip_inflate_find_starts_host: `in`, starts and n are HOST memory; pure host arithmetic, no device.
 * chip_inflate_find_starts: the same answer for a buffer in DEVICE memory; starts is a DEVICE array, n a HOST pointer.  SYNCHRONOUS
 * on `stream`.  A wave per 2 KiB piece of a chunk tests 64 consecutive positions at a time with the 13-bit pre-filter (the first
 * three conditions: 11 % of random positions pass), the survivors check their whole header, and a chunk's pieces stop at its first
 * hit.  Scratch per (device,
 * stream), a launch slot of its own, released by chip_trim(): 8 bytes per chunk.  The calling thread's current device is left as it
 * was.
 * CHIP_E_INVALID, for both before a device is looked for: n NULL; a NULL buffer with len > 0; a NULL array with max > 0; chunk_bytes
 * outside 256 .. CHIP_GZPLAN_WINDOW; len > CHIP_GZPLAN_WINDOW (a unit's limit); first_bit > 8 len.  No alignment is asked of the
 * buffer.  No reference counterpart: compu decodes a stream on one thread.
 */
int chip_inflate_find_starts_host(const uint8_t *in, uint64_t len, uint64_t first_bit, uint32_t chunk_bytes, uint64_t max,
                                  uint64_t *starts, uint64_t *n);
int chip_inflate_find_starts(const void *in_base, uint64_t len, uint64_t first_bit, uint32_t chunk_bytes, uint64_t max,
                             uint64_t *starts, uint64_t *n, void *stream);

/*
 * chip_inflate_parallel: ONE raw deflate / zlib / gzip stream decoded by the whole GPU, with the checkpoint index of the section above
 * as a by-product.  Arguments, formats, limits, alignment, the host `summary` and the counted-then-filled point arrays are
 * chip_inflate_index_build's; chunk_bytes is 0 (128 KiB) or 256 .. CHIP_GZPLAN_WINDOW; out_base may be NULL when out_cap is 0.
 * How: every chunk of chunk_bytes with a start (above) gets a wave that decodes from its start on without output (the size pass
 * with two licences: no wrapper, and matches may reach up to 32 768 bytes in front of the wave's first byte -- how far is recorded),
 * and ends where it arrives at a later start: it is LINKED to it.  A wave that walks over CHIP_PAR_PASS_MAX (8) starts without
 * arriving at one gives up.  The CHAIN follows the links from the stream's beginning; its members are real boundaries by induction and
 * every start that is not on it was false (n_false) and cost its wave.  The stream is CLEAN when the chain ends in a finished final
 * block, no chunk's reach exceeds the content in front of it and the trailer is whole.  Then every chain chunk is decoded once more,
 * into 16-bit elements (a literal, or a marker for "byte j of the 32 768 in front of this chunk"), one workgroup turns each chunk's
 * last 32 KiB into the next chunk's window along the chain, a parallel pass resolves the markers into out_base, and the per-chunk
 * CRC-32 / Adler-32 are combined along the chain into pt_check and the stream's check, which is compared with the trailer.
 * The contract:
 *   - A clean stream of at least two chain chunks, total_out <= out_cap: path = CHIP_PAR_PARALLEL.  The bytes, out_len, in_used and
 *     status (CHIP_FINISHED) are chip_decode_batch(format, 1, ..)'s for the unit; wrap, check and end_bit as in the index build;
 *     total_out = out_len.  The POINTS are the stream's first block and every start on the chain: a property of the stream and
 *     chunk_bytes, not of scheduling.  pt_bit, pt_out, pt_check and windows hold the first min(n_points, max_points) of them in
 *     the index's layout and go to chip_inflate_index_read unchanged.
 *   - The same with total_out > out_cap: status = CHIP_NEED_OUTPUT, out_len = 0, total_out = the exact size to come back with
 *     (chip_pack_units' convention, and the one deliberate difference from chip_decode_batch).  No byte at or behind out_base +
 *     out_cap is written, the bytes in front of it are unspecified, the point arrays are not written.
 *   - Anything else -- an error, a truncation, CHIP_NEED_DICT, a wrong check value or ISIZE, a wave that gave up, a stream of one
 *     block, no start on the chain: path = CHIP_PAR_SERIAL and the answer is the serial decode's, chip_inflate_index_build with a
 *     spacing no stream reaches: chip_decode_batch's out_len, in_used, status and bytes, n_points = 1 (the first block) or 0 (the
 *     wrapper was refused).  If that decode ends CHIP_NEED_OUTPUT and the one-unit size pass finishes, the answer is the room-short
 *     one above with the size pass's total_out.  A multi-member gzip buffer: the first member only.
 * n_starts = the finder's count (0 when the call never got there), n_false as above (0 on the serial path).
 * SYNCHRONOUS on `stream`; it waits for the wrapper, the starts, the links, the trailer's bytes and the result; the chain, the sums
 * and the combination of the checks are host work between those waits.  CHIP_E_INVALID as the index build, and:
 * a chunk_bytes outside the range; out_base NULL with out_cap > 0.
 * Scratch per (device, stream), a launch slot of its own, released by chip_trim(): 2 * total_out bytes for the elements; 64 KiB of
 * token rows per unit of the size pass, at most 128 MiB; 32 KiB per chain chunk when max_points is below the chain's length (the
 * windows nobody asked for); about 100 bytes per chunk of the input.  CHIP_E_NOMEM if it cannot be had.
 */
enum { CHIP_PAR_SERIAL = 0, CHIP_PAR_PARALLEL = 1 };
#define CHIP_PAR_PASS_MAX 8
typedef struct {
    uint64_t n_points, out_len, in_used, end_bit, total_out, n_starts, n_false;
    int32_t status;
    uint32_t wrap, check, path; /* path: CHIP_PAR_SERIAL, CHIP_PAR_PARALLEL */
} chip_inflate_parallel_summary;
int chip_inflate_parallel(int format, const void *in_base, uint64_t len, void *out_base, uint64_t out_cap, uint32_t chunk_bytes,
                          uint64_t max_points, uint64_t *pt_bit, uint64_t *pt_out, uint32_t *pt_check, void *windows,
                          chip_inflate_parallel_summary *summary, void *stream);

/*
 * chip_inflate_parallel_next: the NEXT PART of one raw deflate / zlib / gzip stream of any length, by the passes of
 * chip_inflate_parallel over a SLAB of it.  The caller owns a CURSOR, plain host data that may be copied and
 * saved (all zero = the beginning of a stream), and beside it 32 768 bytes of DEVICE memory, `window`, which a copy of the cursor
 * needs a copy of.  in_base is a device pointer to stream byte cur->in_total and len the bytes of the stream that stand there, at
 * most CHIP_GZPLAN_WINDOW per call.  in_base needs no alignment; the bytes up to the next multiple of 4 behind the slab must be
 * readable.  out_cap is at most 2^32 - 16.  format as chip_inflate_parallel (it is read while phase = HEADER only);
 * chunk_bytes is 0 (128 KiB) or 256 .. CHIP_GZPLAN_WINDOW.  SYNCHRONOUS on `stream`.
 * Where a call ends: it moves the cursor from a block boundary to a later TRUE block boundary of the stream, or through the
 * trailer.  It delivers exactly the content between the two at out_base[0 .. out_len), leaves in `window` the last cur->hist bytes
 * of the content delivered so far (bytes of the old window are kept when fewer than 32 768 were delivered), brings cur->check up
 * to cur->out_total, and answers in_used, the whole bytes in front of the new cursor byte: the next slab begins at in_base +
 * in_used.  Chunks are slab-relative (chunk k is slab bytes [k B, (k + 1) B)), so where calls end depends on slab and room; the bytes
 * never do.  status says why the call stopped:
 *   - CHIP_FINISHED: the final block and the whole trailer were in the slab; the Adler-32 was compared, or the CRC-32 and ISIZE
 *     (with out_total mod 2^32).  phase = CHIP_CUR_DONE; in_used counts through the trailer and nothing behind it.
 *   - CHIP_NEED_INPUT: everything deliverable was delivered.  in_used == 0 && out_len == 0: the slab holds no whole step -- an
 *     incomplete header, a block longer than the slab, a cut trailer; come back with a longer slab.
 *   - CHIP_NEED_OUTPUT: the next piece was whole in the slab and did not fit the room left.  need_out is its decoded size where the
 *     call knows it: always on the parallel path, else 0.
 *   - CHIP_NEED_DICT or a negative code: sticky; phase = CHIP_CUR_ERROR, cur->error keeps it and every later call answers it.
 *     out_len counts the bytes of true content delivered in front of the error.
 * Progress: a call whose slab holds at least one whole block behind the cursor, with room for its bytes, advances the cursor.
 * The parallel path (path = CHIP_PAR_PARALLEL) is chip_inflate_parallel's on the slab: unit 0 of the size pass begins at the cursor
 * instead of a wrapper; a match of the first chain chunk may reach cur->hist bytes back; the window walk starts from the carried
 * window.  A chain member that ended neither LINKED nor in the final block -- normally the last one, which ran out of slab -- is
 * dropped and decoded again by the next call; chain chunks are delivered while they fit out_cap; their checks are appended to
 * cur->check.  The one-wave path (CHIP_PAR_SERIAL) advances a slab on which the chain reaches no start (no start at all, a wave
 * that gave up, a chunk the size pass does not vouch for): one wave decodes from the cursor to the last block boundary it reaches
 * inside slab and room.  An error is found and reported there.
 * A stream that fits one slab with ample room answers with the bytes, the total and the check of chip_inflate_parallel on it.
 * n_chunks = ceil(len / B); n_starts and n_false as chip_inflate_parallel's, for this slab.
 * CHIP_E_INVALID, before a device is looked for: a format other than the four; cur, window or summary NULL; in_base NULL with
 * len > 0; out_base NULL with out_cap > 0; len > CHIP_GZPLAN_WINDOW; out_cap > 2^32 - 16; a chunk_bytes outside the range; a cursor
 * no call has left (bit > 7, an unknown phase or wrap, hist != min(out_total, 32 768)).  CHIP_E_NOMEM / CHIP_E_LAUNCH: the cursor
 * is as it was, the window may not be: the decode cannot go on.
 * Scratch per (device, stream), in chip_inflate_parallel's launch slot, released by chip_trim(): twice the bytes delivered in the
 * call for the elements (one-wave path: twice the room it could use); 64 KiB of token rows per unit of the size pass, at most
 * 128 MiB; 32 KiB per delivered chain chunk; about 100 bytes per chunk of the slab.  It does not depend on the stream's length.
 */
enum { CHIP_CUR_HEADER = 0, CHIP_CUR_BLOCKS = 1, CHIP_CUR_TRAILER = 2, CHIP_CUR_DONE = 3, CHIP_CUR_ERROR = 4 };
typedef struct {
    uint64_t in_total;  /* whole bytes of the stream in front of the byte the next call starts in */
    uint64_t out_total; /* bytes delivered so far */
    uint32_t bit;       /* 0..7: where in that byte the next block header begins */
    uint32_t phase;     /* CHIP_CUR_* */
    uint32_t wrap;      /* 0 raw, 1 zlib, 2 gzip (known once phase > HEADER) */
    uint32_t check;     /* running Adler-32 / CRC-32 over out_total bytes */
    uint32_t hist;      /* valid bytes of `window`: min(out_total, 32768) */
    int32_t error;      /* the sticky status once phase == ERROR */
} chip_inflate_cursor;  /* all zero = the beginning of a stream */
typedef struct {
    uint64_t in_used, out_len, need_out, n_chunks, n_starts, n_false;
    int32_t status; /* why the call stopped */
    uint32_t path;  /* CHIP_PAR_SERIAL, CHIP_PAR_PARALLEL */
} chip_inflate_next_summary;
int chip_inflate_parallel_next(int format, chip_inflate_cursor *cur, void *window, const void *in_base, uint64_t len, void *out_base,
                               uint64_t out_cap, uint32_t chunk_bytes, chip_inflate_next_summary *summary, void *stream);

/* ---- zstd encoder: encoder::Interface::zstd, src/encoder/zstd.rs ------------------------------------------------------------ */

/* ZstdStrategy src/encoder/zstd.rs:33-56 (ZSTD_strategy values; 0 = the level's own).  The GPU encoder has four level groups
 * (DESIGN.md sec. 4.6): levels <= 2 greedy with a skip over runs without matches, 3..5 greedy with a repeat-offset probe, 6..12
 * lazy, 13..22 lazy with two positions per hash slot; a strategy other than Default picks the group: Fast the first, Dfast and
 * Greedy the second, Lazy and Lazy2 the third, Btlazy2 and the optimal-parsing strategies the fourth. */
enum {
    CHIP_ZSTD_STRATEGY_DEFAULT = 0,
    CHIP_ZSTD_STRATEGY_FAST = 1,
    CHIP_ZSTD_STRATEGY_DFAST = 2,
    CHIP_ZSTD_STRATEGY_GREEDY = 3,
    CHIP_ZSTD_STRATEGY_LAZY = 4,
    CHIP_ZSTD_STRATEGY_LAZY2 = 5,
    CHIP_ZSTD_STRATEGY_BTLAZY2 = 6,
    CHIP_ZSTD_STRATEGY_BTOPT = 7,
    CHIP_ZSTD_STRATEGY_BTULTRA = 8,
    CHIP_ZSTD_STRATEGY_BTULTRA2 = 9
};

/* ZstdOptions src/encoder/zstd.rs:62-126 */
typedef struct {
    int32_t level;      /* -131072..131072 (0 = 3, above 22 = 22, as libzstd); default 3 */
    int32_t strategy;   /* CHIP_ZSTD_STRATEGY_*; default Default */
    int32_t window_log; /* 10..31, default 27: caps the match distance and the declared window (at most 2^27) */
    int32_t device;     /* HIP device ordinal, -1 = current */
} chip_zstd_encoder_opts;

/* Interface::zstd(opts) src/encoder/zstd.rs:128-160.  NULL opts = ZstdOptions::new(); NULL on an option out of range.
 * The encoder is driven by chip_encode / chip_encoder_reset / chip_encoder_free.  Every frame carries the content checksum
 * (libzstd's default is without it).  chip_encode's status follows src/encoder/zstd.rs:174-197. */
chip_encoder *chip_encoder_new_zstd(const chip_zstd_encoder_opts *opts);

/* ---- brotli encoder: encoder::Interface::brotli_c / brotli_rust, src/encoder/brotli_c.rs, brotli_common.rs ------------------ */

/* BrotliOptions src/encoder/brotli_common.rs.  The GPU encoder has four quality groups: quality 1 greedy
 * with a skip over runs without matches, 2..4 greedy with a last-distance probe, 5..9 lazy, 10..11 lazy with two positions per
 * hash slot.  `mode` is compu's raw byte (BrotliEncoderMode: Generic = 1, Text = 2, Font = 3; 0 = unset), which compu hands
 * to BROTLI_PARAM_MODE unchanged; the GPU encoder has no mode-dependent modelling, so it is accepted and recorded only. */
typedef struct {
    int32_t quality; /* 0..11, 0 = unset = libbrotlienc's default 11 */
    int32_t mode;    /* 0..3 */
    int32_t lgwin;   /* 10..24, default 22: the WBITS field; matches reach at most min(2^lgwin - 16, 65536) bytes */
    int32_t device;  /* HIP device ordinal, -1 = current */
} chip_brotli_encoder_opts;

/* Interface::brotli_c(opts) src/encoder/brotli_c.rs:38-50.  NULL opts = BrotliOptions::new() (quality 0 = 11, mode 0, lgwin
 * 22); NULL on quality > 11, mode > 3 or lgwin outside 10..24.  Driven by chip_encode / chip_encoder_reset / chip_encoder_free:
 * Flush byte-aligns the stream with an empty metadata metablock as libbrotlienc's FLUSH does; chip_encode's status follows
 * src/encoder/brotli_c.rs:63-84. */
chip_encoder *chip_encoder_new_brotli(const chip_brotli_encoder_opts *opts);

#ifdef __cplusplus
}
#endif
#endif
