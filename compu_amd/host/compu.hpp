// compu.hpp -- C++ mirror of compu's Decoder / Encoder surface over the C ABI of libcompu_hip.so.
//
// The reference is a Rust crate; this image has no Rust toolchain, so the host side above the C ABI is
// written in C++ with the reference's names, argument meaning and error behaviour:
//   compu::decoder::{Interface, Decoder, Decode, DecodeStatus, DecodeError, Detection, ZlibMode, ZstdOptions}
//       <- src/decoder/mod.rs, src/decoder/zlib_common.rs, src/decoder/zstd.rs
//   compu::encoder::{Interface, Encoder, Encode, EncodeOp, EncodeStatus, ZlibOptions}
//       <- src/encoder/mod.rs, src/encoder/zlib_common.rs
//   compu::Buffer<N>, compu::PinnedBuffer, compu::DeviceBuffer          <- src/buffer.rs (+ the north star's pinned-host / device types)
// so that tests/cpp/test_reference.cpp reads like tests/decoder.rs / tests/encoder.rs.  The Rust glue a
// maintainer would add to the crate itself is in INTEGRATION.md.
#pragma once

#include <cassert>
#include <cstddef>
#include <cstdint>
#include <optional>
#include <utility>
#include <vector>

#include "../../include/compu_hip.h"

namespace compu {

template <size_t N>
class Buffer;

namespace decoder {

// src/decoder/mod.rs:9-21, 28-114
enum class Detection { Zstd = CHIP_DETECT_ZSTD, Gzip = CHIP_DETECT_GZIP, Zlib = CHIP_DETECT_ZLIB, Unknown = CHIP_DETECT_UNKNOWN };
inline std::optional<Detection> detect(const uint8_t *bytes, size_t len)
{
    int k = chip_detect(bytes, len);
    if (k < 0) return std::nullopt;
    return static_cast<Detection>(k);
}

// src/decoder/mod.rs:117-135
struct DecodeError {
    int32_t code = 0;
    static DecodeError no_error() { return DecodeError{0}; }
    int32_t as_raw() const { return code; }
    bool operator==(const DecodeError &o) const { return code == o.code; }
};

// src/decoder/mod.rs:139-146
enum class DecodeStatus { NeedInput = CHIP_NEED_INPUT, NeedOutput = CHIP_NEED_OUTPUT, Finished = CHIP_FINISHED };

// src/decoder/mod.rs:150-157: status is Result<DecodeStatus, DecodeError>
struct Decode {
    size_t input_remain;
    size_t output_remain;
    bool ok;
    DecodeStatus status;  // valid when ok
    DecodeError error;    // valid when !ok
    bool is(DecodeStatus s) const { return ok && status == s; }
};

// src/decoder/zlib_common.rs:4-29
// chip_decode_batch_ex / chip_decode_batch_sizes options (DeviceBuffer::decode_batch's `flags`); MEMBERS has no compu counterpart
constexpr uint32_t F_COMPU_STATUS = CHIP_F_COMPU_STATUS, F_MEMBERS = CHIP_F_MEMBERS;
enum class ZlibMode : int { Deflate = CHIP_FMT_DEFLATE, Zlib = CHIP_FMT_ZLIB, Gzip = CHIP_FMT_GZIP, Auto = CHIP_FMT_AUTO };

// src/decoder/zstd.rs:22-74
struct ZstdOptions {
    int32_t window_log_ = 0;
    ZstdOptions window_log(int32_t v) const
    {
        ZstdOptions o = *this;
        o.window_log_ = v;
        return o;
    }
};

// src/decoder/mod.rs:269-455
class Decoder {
public:
    Decoder(chip_decoder *h, int fmt) : h_(h), fmt_(fmt) {}
    Decoder(Decoder &&o) noexcept : h_(o.h_), fmt_(o.fmt_) { o.h_ = nullptr; }
    Decoder(const Decoder &) = delete;
    Decoder &operator=(const Decoder &) = delete;
    ~Decoder() { chip_decoder_free(h_); }  // Drop, mod.rs:450-455

    // raw_decode, mod.rs:290-292
    Decode raw_decode(const uint8_t *input, size_t input_len, uint8_t *output, size_t output_len)
    {
        chip_decode_result r = chip_decode(h_, input, input_len, output, output_len);
        Decode d{r.input_remain, r.output_remain, r.err == 0, DecodeStatus::NeedInput, DecodeError{r.err}};
        if (d.ok) d.status = static_cast<DecodeStatus>(r.status);
        return d;
    }
    // decode, mod.rs:309-315
    Decode decode(const uint8_t *input, size_t input_len, uint8_t *output, size_t output_len)
    {
        static uint8_t dummy_in = 0, dummy_out = 0;  // slices are never null in Rust
        return raw_decode(input_len ? input : &dummy_in, input_len, output_len ? output : &dummy_out, output_len);
    }
    // decode_vec, mod.rs:323-335: writes into the spare capacity, advances len only on Ok
    Decode decode_vec(const uint8_t *input, size_t input_len, std::vector<uint8_t> &output)
    {
        const size_t len = output.size(), spare = output.capacity() - len;
        output.resize(output.capacity());
        Decode r = decode(input, input_len, output.data() + len, spare);
        output.resize(r.ok ? len + spare - r.output_remain : len);
        return r;
    }
    // decode_vec_full, mod.rs:360-385
    Decode decode_vec_full(const uint8_t *input, size_t input_len, std::vector<uint8_t> &output)
    {
        constexpr size_t RESERVE_DEFAULT = 1024;
        size_t reserve_size;
        if (input_len < RESERVE_DEFAULT) {
            output.reserve(output.size() + input_len);
            reserve_size = input_len / 3;
        } else if (input_len < RESERVE_DEFAULT * 16) {
            output.reserve(output.size() + input_len + input_len / 3);
            reserve_size = RESERVE_DEFAULT;
        } else {
            output.reserve(output.size() + input_len * 2);
            reserve_size = RESERVE_DEFAULT * 8;
        }
        for (;;) {
            Decode r = decode_vec(input, input_len, output);
            if (r.is(DecodeStatus::NeedOutput)) {
                input += input_len - r.input_remain;
                input_len = r.input_remain;
                output.reserve(output.size() + (reserve_size ? reserve_size : 1));
                continue;
            }
            return r;
        }
    }
    // reset, mod.rs:433-441: the returned instance replaces the held one
    bool reset()
    {
        chip_decoder *n = chip_decoder_reset(h_);
        if (!n) return false;
        h_ = n;
        return true;
    }
    // describe_error, mod.rs:445-447
    const char *describe_error(DecodeError e) const { return chip_decoder_strerror(fmt_, e.as_raw()); }

private:
    chip_decoder *h_;
    int fmt_;
};

// decoder::Interface constructors of the `hip` variant
struct Interface {
    // Interface::zlib_ng(mode), src/decoder/zlib_ng.rs:61-90
    static std::optional<Decoder> zlib_hip(ZlibMode mode = ZlibMode::Auto, int device = -1)
    {
        chip_decoder_opts o{0, device};
        chip_decoder *h = chip_decoder_new(static_cast<int>(mode), &o);
        if (!h) return std::nullopt;
        return Decoder(h, static_cast<int>(mode));
    }
    // Interface::zstd(opts), src/decoder/zstd.rs:81-94
    static std::optional<Decoder> zstd_hip(ZstdOptions opts = {}, int device = -1)
    {
        chip_decoder_opts o{opts.window_log_, device};
        chip_decoder *h = chip_decoder_new(CHIP_FMT_ZSTD, &o);
        if (!h) return std::nullopt;
        return Decoder(h, CHIP_FMT_ZSTD);
    }
    // Interface::brotli_c(), src/decoder/brotli_c.rs:17-27
    static std::optional<Decoder> brotli_hip(int device = -1)
    {
        chip_decoder_opts o{0, device};
        chip_decoder *h = chip_decoder_new(CHIP_FMT_BROTLI, &o);
        if (!h) return std::nullopt;
        return Decoder(h, CHIP_FMT_BROTLI);
    }
};

}  // namespace decoder

namespace encoder {

enum class EncodeOp { Process = CHIP_OP_PROCESS, Flush = CHIP_OP_FLUSH, Finish = CHIP_OP_FINISH };  // mod.rs:12-23
enum class EncodeStatus { Continue = CHIP_ENC_CONTINUE, NeedOutput = CHIP_ENC_NEED_OUTPUT, Finished = CHIP_ENC_FINISHED, Error = CHIP_ENC_ERROR };  // mod.rs:27-38

// src/encoder/mod.rs:42-49
struct Encode {
    size_t input_remain;
    size_t output_remain;
    EncodeStatus status;
};

using ZlibMode = decoder::ZlibMode;  // src/encoder/zlib_common.rs:28-37 (Deflate | Zlib | Gzip)

// src/encoder/zlib_common.rs:5-24
enum class ZlibStrategy { Default = 0, Filtered = 1, HuffmanOnly = 2, Rle = 3, Fixed = 4 };

// src/encoder/zstd.rs:33-56
enum class ZstdStrategy { Default = 0, Fast = 1, DFast = 2, Greedy = 3, Lazy = 4, Lazy2 = 5, BtLazy2 = 6, BtOpt = 7, BtUltra = 8, BtUltra2 = 9 };

// the encoder's ZstdOptions, src/encoder/zstd.rs:62-126 (defaults: level 3, Default strategy, window_log 27)
struct ZstdOptions {
    int32_t level_ = 3;
    ZstdStrategy strategy_ = ZstdStrategy::Default;
    int32_t window_log_ = 27;
    ZstdOptions level(int32_t v) const
    {
        ZstdOptions o = *this;
        o.level_ = v;
        return o;
    }
    ZstdOptions strategy(ZstdStrategy s) const
    {
        ZstdOptions o = *this;
        o.strategy_ = s;
        return o;
    }
    ZstdOptions window_log(int32_t v) const
    {
        ZstdOptions o = *this;
        o.window_log_ = v;
        return o;
    }
};

// src/encoder/brotli_common.rs: compu's raw mode byte (handed to BROTLI_PARAM_MODE unchanged; recorded only on the GPU)
enum class BrotliEncoderMode { Generic = 1, Text = 2, Font = 3 };

// the encoder's BrotliOptions, src/encoder/brotli_common.rs (defaults: quality and mode unset = libbrotlienc's quality 11)
struct BrotliOptions {
    int32_t quality_ = 0;
    int32_t mode_ = 0;
    BrotliOptions quality(int32_t v) const
    {
        assert(v > 0 && v <= 11);
        BrotliOptions o = *this;
        o.quality_ = v;
        return o;
    }
    BrotliOptions mode(BrotliEncoderMode m) const
    {
        BrotliOptions o = *this;
        o.mode_ = static_cast<int32_t>(m);
        return o;
    }
};

// src/encoder/zlib_common.rs:47-103 (defaults: Gzip, Default strategy, mem_level 8, compression 9, :59-66)
struct ZlibOptions {
    ZlibMode mode_ = ZlibMode::Gzip;
    ZlibStrategy strategy_ = ZlibStrategy::Default;
    int mem_level_ = 8;
    int compression_ = 9;
    ZlibOptions strategy(ZlibStrategy s) const
    {
        ZlibOptions o = *this;
        o.strategy_ = s;
        return o;
    }
    ZlibOptions mem_level(int level) const
    {
        ZlibOptions o = *this;
        o.mem_level_ = level;
        return o;
    }
    ZlibOptions mode(ZlibMode m) const
    {
        ZlibOptions o = *this;
        o.mode_ = m;
        return o;
    }
    ZlibOptions compression(int level) const
    {
        ZlibOptions o = *this;
        o.compression_ = level;
        return o;
    }
};

// src/encoder/mod.rs:148-330
class Encoder {
public:
    explicit Encoder(chip_encoder *h) : h_(h) {}
    Encoder(Encoder &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Encoder(const Encoder &) = delete;
    Encoder &operator=(const Encoder &) = delete;
    ~Encoder() { chip_encoder_free(h_); }

    // raw_encode / encode, mod.rs:171-199
    Encode encode(const uint8_t *input, size_t input_len, uint8_t *output, size_t output_len, EncodeOp op)
    {
        static uint8_t dummy_in = 0, dummy_out = 0;
        chip_encode_result r = chip_encode(h_, input_len ? input : &dummy_in, input_len, output_len ? output : &dummy_out, output_len, static_cast<int>(op));
        return Encode{r.input_remain, r.output_remain, static_cast<EncodeStatus>(r.status)};
    }
    // encode_vec, mod.rs:203-213: the length is set even on Error
    Encode encode_vec(const uint8_t *input, size_t input_len, std::vector<uint8_t> &output, EncodeOp op)
    {
        const size_t len = output.size(), spare = output.capacity() - len;
        output.resize(output.capacity());
        Encode r = encode(input, input_len, output.data() + len, spare, op);
        output.resize(len + spare - r.output_remain);
        return r;
    }
    // encode_vec_full, mod.rs:239-267
    Encode encode_vec_full(const uint8_t *input, size_t input_len, std::vector<uint8_t> &output, EncodeOp op)
    {
        constexpr size_t RESERVE_DEFAULT = 1024;
        size_t reserve_size;
        if (input_len < RESERVE_DEFAULT) {
            output.reserve(output.size() + input_len);
            reserve_size = input_len / 3;
        } else if (input_len < RESERVE_DEFAULT * 16) {
            output.reserve(output.size() + input_len / 2);
            reserve_size = RESERVE_DEFAULT;
        } else {
            output.reserve(output.size() + input_len / 3);
            reserve_size = RESERVE_DEFAULT * 8;
        }
        for (;;) {
            Encode r = encode_vec(input, input_len, output, op);
            if (r.status == EncodeStatus::NeedOutput) {
                input += input_len - r.input_remain;
                input_len = r.input_remain;
                output.reserve(output.size() + (reserve_size ? reserve_size : 1));
                continue;
            }
            if (r.status == EncodeStatus::Continue && op == EncodeOp::Finish) {
                input += input_len - r.input_remain;
                input_len = r.input_remain;
                continue;
            }
            return r;
        }
    }
    // reset, mod.rs:314-321
    bool reset()
    {
        chip_encoder *n = chip_encoder_reset(h_);
        if (!n) return false;
        h_ = n;
        return true;
    }

private:
    chip_encoder *h_;
};

struct Interface {
    // Interface::zlib_ng(opts), src/encoder/zlib_ng.rs:50-87
    static std::optional<Encoder> zlib_hip(ZlibOptions opts = {}, int device = -1)
    {
        chip_encoder_opts o{static_cast<int32_t>(opts.mode_), opts.compression_, device, static_cast<int32_t>(opts.strategy_), opts.mem_level_};
        chip_encoder *h = chip_encoder_new(&o);
        if (!h) return std::nullopt;
        return Encoder(h);
    }
    // Interface::zstd(opts), src/encoder/zstd.rs:138-160 (nullopt for an option out of range, as apply() failing)
    static std::optional<Encoder> zstd_hip(ZstdOptions opts = {}, int device = -1)
    {
        chip_zstd_encoder_opts o{opts.level_, static_cast<int32_t>(opts.strategy_), opts.window_log_, device};
        chip_encoder *h = chip_encoder_new_zstd(&o);
        if (!h) return std::nullopt;
        return Encoder(h);
    }
    // Interface::brotli_c(opts), src/encoder/brotli_c.rs:38-50 (lgwin 22, libbrotlienc's default)
    static std::optional<Encoder> brotli_hip(BrotliOptions opts = {}, int device = -1)
    {
        chip_brotli_encoder_opts o{opts.quality_, opts.mode_, 22, device};
        chip_encoder *h = chip_encoder_new_brotli(&o);
        if (!h) return std::nullopt;
        return Encoder(h);
    }
};

}  // namespace encoder

// src/buffer.rs:1-49 with Buffer::decode (src/decoder/mod.rs:507-531) and Buffer::encode
// (src/encoder/mod.rs:395-412)
template <size_t N>
class Buffer {
public:
    const uint8_t *data() const { return buf_; }
    size_t len() const { return cursor_; }
    void consume() { cursor_ = 0; }

    // Ok((consumed, status)) or Err(error); on error the buffer does not advance
    std::pair<bool, std::pair<size_t, decoder::DecodeStatus>> decode(decoder::Decoder &dec, const uint8_t *input, size_t input_len,
                                                                      decoder::DecodeError *err = nullptr)
    {
        const size_t spare = N - cursor_;
        decoder::Decode r = dec.decode(input, input_len, buf_ + cursor_, spare);
        if (!r.ok) {
            if (err) *err = r.error;
            return {false, {0, decoder::DecodeStatus::NeedInput}};
        }
        cursor_ += spare - r.output_remain;
        return {true, {input_len - r.input_remain, r.status}};
    }
    std::pair<size_t, encoder::EncodeStatus> encode(encoder::Encoder &enc, const uint8_t *input, size_t input_len, encoder::EncodeOp op)
    {
        const size_t spare = N - cursor_;
        encoder::Encode r = enc.encode(input, input_len, buf_ + cursor_, spare, op);
        cursor_ += spare - r.output_remain;
        return {input_len - r.input_remain, r.status};
    }

private:
    uint8_t buf_[N];
    size_t cursor_ = 0;
};

// The two buffer types the hip backend adds to src/buffer.rs (north star: "src/buffer.rs grows pinned-host + device
// buffer types"), with Buffer<N>'s cursor API (data / len / consume / spare capacity; src/buffer.rs:9-49).
//
// PinnedBuffer: page-locked host memory (hipHostMalloc through chip_pinned_alloc).  Used exactly like Buffer<N> with the
// streaming Decoder / Encoder; the copies between it and the GPU are real DMA transfers instead of staged ones.
class PinnedBuffer {
public:
    explicit PinnedBuffer(size_t capacity) : buf_((uint8_t *)chip_pinned_alloc(capacity)), cap_(buf_ ? capacity : 0) {}
    ~PinnedBuffer() { chip_pinned_free(buf_); }
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    bool valid() const { return buf_ != nullptr; }
    const uint8_t *data() const { return buf_; }
    size_t len() const { return cursor_; }
    size_t capacity() const { return cap_; }
    void consume() { cursor_ = 0; }
    uint8_t *spare_capacity_mut() { return buf_ + cursor_; }
    size_t spare_capacity_len() const { return cap_ - cursor_; }
    void advance(size_t n) { cursor_ += n; }  // after writing n bytes into the spare capacity

    std::pair<bool, std::pair<size_t, decoder::DecodeStatus>> decode(decoder::Decoder &dec, const uint8_t *input, size_t input_len,
                                                                      decoder::DecodeError *err = nullptr)
    {
        const size_t spare = cap_ - cursor_;
        decoder::Decode r = dec.decode(input, input_len, buf_ + cursor_, spare);
        if (!r.ok) {
            if (err) *err = r.error;
            return {false, {0, decoder::DecodeStatus::NeedInput}};
        }
        cursor_ += spare - r.output_remain;
        return {true, {input_len - r.input_remain, r.status}};
    }
    std::pair<size_t, encoder::EncodeStatus> encode(encoder::Encoder &enc, const uint8_t *input, size_t input_len, encoder::EncodeOp op)
    {
        const size_t spare = cap_ - cursor_;
        encoder::Encode r = enc.encode(input, input_len, buf_ + cursor_, spare, op);
        cursor_ += spare - r.output_remain;
        return {input_len - r.input_remain, r.status};
    }

private:
    uint8_t *buf_;
    size_t cap_;
    size_t cursor_ = 0;
};

// DeviceBuffer: memory of the current GPU (hipMalloc through chip_device_alloc; src/mem.rs routes device allocations
// there).  The batched entry points read and write device memory, so a DeviceBuffer is what a batch decodes out of and
// into without the data ever touching the host: upload() appends host bytes, decode_batch() appends the decoded units
// behind the cursor, download() reads back.
class DeviceBuffer {
public:
    explicit DeviceBuffer(size_t capacity) : buf_((uint8_t *)chip_device_alloc(capacity + 16)), cap_(buf_ ? capacity : 0) {}
    ~DeviceBuffer() { chip_device_free(buf_); }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    bool valid() const { return buf_ != nullptr; }
    const uint8_t *data() const { return buf_; }  // DEVICE pointer to the written part
    size_t len() const { return cursor_; }
    size_t capacity() const { return cap_; }
    void consume() { cursor_ = 0; }
    uint8_t *spare_capacity_mut() { return buf_ + cursor_; }  // DEVICE pointer
    size_t spare_capacity_len() const { return cap_ - cursor_; }
    void advance(size_t n) { cursor_ += n; }

    // append host bytes (synchronous); false when they do not fit
    bool upload(const uint8_t *src, size_t n)
    {
        if (n > cap_ - cursor_) return false;
        if (n && (chip_memcpy_h2d(buf_ + cursor_, src, n, nullptr) != CHIP_OK || chip_stream_sync(nullptr) != CHIP_OK)) return false;
        cursor_ += n;
        return true;
    }
    // copy `n` written bytes from offset `from` to the host (synchronous)
    bool download(uint8_t *dst, size_t from, size_t n) const
    {
        if (from + n > cursor_) return false;
        return n == 0 || (chip_memcpy_d2h(dst, buf_ + from, n, nullptr) == CHIP_OK && chip_stream_sync(nullptr) == CHIP_OK);
    }
    // chip_decode_batch[_ex] with this buffer's spare capacity as the output: unit i lands at spare + out_off[i] (device
    // arrays, as in chip_decode_batch); `span` bytes behind the cursor become part of the data.  Only enqueues.
    // flags: CHIP_F_COMPU_STATUS reports every unit's status exactly as compu's decode_fn would; CHIP_F_MEMBERS decodes a unit
    // as a series of gzip members / zstd frames (include/compu_hip.h).
    int decode_batch(int format, size_t n, const DeviceBuffer &in, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off,
                     const uint32_t *out_cap, uint32_t *out_len, uint32_t *in_used, int32_t *status, size_t span, void *stream = nullptr,
                     uint32_t flags = 0)
    {
        if (span > cap_ - cursor_) return CHIP_E_INVALID;
        const int rc = chip_decode_batch_ex(format, flags, n, in.data(), in_off, in_len, buf_ + cursor_, out_off, out_cap, out_len, in_used, status, stream);
        if (rc == CHIP_OK) cursor_ += span;
        return rc;
    }
    // chip_decode_batch_sizes over a batch held in `in`: the decoded length (64-bit), input consumed and status of every unit
    // (device arrays), without an output buffer -- what a caller needs to give decode_batch() an out_cap[i].  Only enqueues.
    static int decode_batch_sizes(int format, size_t n, const DeviceBuffer &in, const uint64_t *in_off, const uint32_t *in_len, uint64_t *out_size,
                                  uint32_t *in_used, int32_t *status, void *stream = nullptr)
    {
        return chip_decode_batch_sizes(format, 0, n, in.data(), in_off, in_len, out_size, in_used, status, stream);
    }
    // chip_bgzf_plan over the BGZF bytes held in `in` (its first `len` bytes): the four DEVICE arrays of the decode_batch(CHIP_FMT_GZIP, ..)
    // that follows, for the first min(n_blocks, max_blocks) blocks, and the summary of the whole walk.  Synchronous on `stream`.
    static int bgzf_plan(const DeviceBuffer &in, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                         uint32_t *out_cap, chip_bgzf_summary &summary, void *stream = nullptr)
    {
        if (len > in.len()) return CHIP_E_INVALID;
        return chip_bgzf_plan(in.data(), len, max_blocks, in_off, in_len, out_off, out_cap, &summary, stream);
    }
    // chip_zstd_plan over the zstd frames held in `in` (its first `len` bytes): the four DEVICE arrays of the decode_batch(CHIP_FMT_ZSTD, ..)
    // that follows, for the first min(n_frames, max_frames) frames, and the summary of the whole walk.  Synchronous on `stream`.
    static int zstd_plan(const DeviceBuffer &in, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                         uint32_t *out_cap, chip_zstd_plan_summary &summary, void *stream = nullptr)
    {
        if (len > in.len()) return CHIP_E_INVALID;
        return chip_zstd_plan(in.data(), len, max_frames, in_off, in_len, out_off, out_cap, &summary, stream);
    }
    // chip_gzip_plan over the gzip members held in `in` (its first `len` bytes): the four DEVICE arrays of the decode_batch(CHIP_FMT_GZIP, ..)
    // that follows, for the first min(n_members, max_members) members, and the summary of the whole walk.  Synchronous on `stream`.
    static int gzip_plan(const DeviceBuffer &in, uint64_t len, uint64_t max_members, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                         uint32_t *out_cap, chip_gzip_plan_summary &summary, void *stream = nullptr)
    {
        if (len > in.len()) return CHIP_E_INVALID;
        return chip_gzip_plan(in.data(), len, max_members, in_off, in_len, out_off, out_cap, &summary, stream);
    }
    // chip_layout_units: from the out_size of decode_batch_sizes() to the out_off / out_cap of decode_batch() (DEVICE arrays); `total` is
    // what to allocate, `n_over` counts the units above 4 GiB - 1.  Synchronous on `stream`.
    static int layout_units(size_t n, const uint64_t *out_size, uint64_t *out_off, uint32_t *out_cap, uint64_t &total, uint64_t &n_over,
                            void *stream = nullptr)
    {
        return chip_layout_units(n, out_size, out_off, out_cap, &total, &n_over, stream);
    }
    // chip_pack_units into this buffer's spare capacity: the ranges src[src_off[i] .. + src_len[i]) (DEVICE arrays) end to end behind
    // the cursor, which moves by `total` when they fit; when they do not, nothing is written and `total` says how much room is needed.
    // dst_off (DEVICE, may be nullptr) receives the n offsets.  Synchronous on `stream`.
    int pack_units(size_t n, const DeviceBuffer &src, const uint64_t *src_off, const uint32_t *src_len, uint64_t *dst_off, uint64_t &total,
                   void *stream = nullptr)
    {
        const int rc = chip_pack_units(n, src.data(), src_off, src_len, buf_ + cursor_, cap_ - cursor_, dst_off, &total, stream);
        if (rc == CHIP_OK && total <= cap_ - cursor_) cursor_ += total;
        return rc;
    }
    // chip_encode_file into this buffer's spare capacity: the first `len` bytes of `in` as a BGZF file, a file of gzip members or a file of
    // zstd frames (flags CHIP_W_SEEK_TABLE: with the seek table) behind the cursor, which moves by summary.out_len on CHIP_FILE_OK.
    // chip_encode_file_bound(format, unit_bytes, flags, len) of spare capacity is always enough.  Synchronous on `stream`.
    int encode_file(int format, int level, uint32_t unit_bytes, uint32_t flags, const DeviceBuffer &in, uint64_t len, chip_file_summary &summary,
                    void *stream = nullptr)
    {
        if (len > in.len()) return CHIP_E_INVALID;
        const int rc = chip_encode_file(format, level, unit_bytes, flags, in.data(), len, buf_ + cursor_, cap_ - cursor_, &summary, stream);
        if (rc == CHIP_OK && summary.status == CHIP_FILE_OK) cursor_ += summary.out_len;
        return rc;
    }
    // chip_read_ranges into this buffer's spare capacity: the bytes of n_ranges ranges (DEVICE arrays range_lo / range_len, in the
    // coordinates of out_off) of the plan over `in`, end to end behind the cursor, which moves by summary.out_len on CHIP_READ_OK.  Only
    // the units the ranges touch are decoded, each once.  On CHIP_READ_NEED_OUTPUT nothing is written and summary.out_len says how much
    // room is needed.  dst_off and range_status (DEVICE, may be nullptr) receive one entry per range.  Synchronous on `stream`.
    int read_ranges(int format, size_t n_units, const DeviceBuffer &in, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off,
                    const uint32_t *out_cap, size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, uint64_t *dst_off,
                    int32_t *range_status, chip_read_summary &summary, void *stream = nullptr)
    {
        const int rc = chip_read_ranges(format, n_units, in.data(), in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len, buf_ + cursor_,
                                        cap_ - cursor_, dst_off, range_status, &summary, stream);
        if (rc == CHIP_OK && summary.status == CHIP_READ_OK) cursor_ += summary.out_len;
        return rc;
    }
    // chip_inflate_index_build into this buffer's spare capacity: the ONE gzip / zlib / raw deflate stream held in `in` (its first `len`
    // bytes) is decoded behind the cursor, which moves by summary.out_len, and a point is recorded every `spacing` decoded bytes (0 = 1 MiB)
    // into the first max_points entries of the DEVICE arrays pt_bit / pt_out / pt_check / windows (32 768 bytes per point).  The decode's
    // answers are decode_batch()'s for that unit.  Synchronous on `stream`.
    int inflate_index_build(int format, const DeviceBuffer &in, uint64_t len, uint32_t spacing, uint64_t max_points, uint64_t *pt_bit,
                            uint64_t *pt_out, uint32_t *pt_check, void *windows, chip_inflate_index_summary &summary, void *stream = nullptr)
    {
        if (len > in.len()) return CHIP_E_INVALID;
        const size_t room = cap_ - cursor_;
        const int rc = chip_inflate_index_build(format, in.data(), len, buf_ + cursor_, room < 0xFFFFFFF0u ? room : 0xFFFFFFF0u, spacing, max_points,
                                                pt_bit, pt_out, pt_check, windows, &summary, stream);
        if (rc == CHIP_OK) cursor_ += summary.out_len;
        return rc;
    }
    // chip_inflate_index_read into this buffer's spare capacity: read_ranges() over the chunks of an index (the DEVICE arrays of
    // inflate_index_build, n_points of them; total_out = the build's out_len; format = the build's wrap).  Every touched chunk is decoded
    // once, on a wave of its own, and verified against the next point's check value.  Synchronous on `stream`.
    int inflate_index_read(int format, const DeviceBuffer &in, uint64_t len, uint64_t n_points, const uint64_t *pt_bit, const uint64_t *pt_out,
                           const uint32_t *pt_check, const void *windows, uint64_t total_out, size_t n_ranges, const uint64_t *range_lo,
                           const uint32_t *range_len, uint64_t *dst_off, int32_t *range_status, chip_read_summary &summary, void *stream = nullptr)
    {
        if (len > in.len()) return CHIP_E_INVALID;
        const int rc = chip_inflate_index_read(format, in.data(), len, n_points, pt_bit, pt_out, pt_check, windows, total_out, n_ranges, range_lo,
                                               range_len, buf_ + cursor_, cap_ - cursor_, dst_off, range_status, &summary, stream);
        if (rc == CHIP_OK && summary.status == CHIP_READ_OK) cursor_ += summary.out_len;
        return rc;
    }
    // chip_inflate_parallel into this buffer's spare capacity: inflate_index_build()'s stream decoded with a wave per chunk of chunk_bytes
    // (0 = 128 KiB) that holds a block start; the point arrays receive the chain's chunks.  With too little room summary.status is
    // CHIP_NEED_OUTPUT and summary.total_out the size to come back with.  Synchronous on `stream`.
    int inflate_parallel(int format, const DeviceBuffer &in, uint64_t len, uint32_t chunk_bytes, uint64_t max_points, uint64_t *pt_bit, uint64_t *pt_out,
                         uint32_t *pt_check, void *windows, chip_inflate_parallel_summary &summary, void *stream = nullptr)
    {
        if (len > in.len()) return CHIP_E_INVALID;
        const size_t room = cap_ - cursor_;
        const int rc = chip_inflate_parallel(format, in.data(), len, buf_ + cursor_, room < 0xFFFFFFF0u ? room : 0xFFFFFFF0u, chunk_bytes, max_points,
                                             pt_bit, pt_out, pt_check, windows, &summary, stream);
        if (rc == CHIP_OK) cursor_ += summary.out_len;
        return rc;
    }
    // chip_inflate_parallel_next into this buffer's spare capacity: the next part of ONE stream of any length.  `slab` holds `len` bytes of
    // the stream from byte cur.in_total on (from offset `from` of the buffer: the caller keeps what a call did not consume and moves on by
    // summary.in_used), `window` is the cursor's 32 768 bytes of DEVICE memory.  The cursor of this buffer moves by summary.out_len;
    // summary.status says why the call stopped.  Synchronous on `stream`.
    int inflate_parallel_next(int format, chip_inflate_cursor &cur, void *window, const DeviceBuffer &slab, uint64_t from, uint64_t len,
                              uint32_t chunk_bytes, chip_inflate_next_summary &summary, void *stream = nullptr)
    {
        if (from > slab.len() || len > slab.len() - from) return CHIP_E_INVALID;
        const size_t room = cap_ - cursor_;
        const int rc = chip_inflate_parallel_next(format, &cur, window, slab.data() + from, len, buf_ + cursor_, room < 0xFFFFFFF0u ? room : 0xFFFFFFF0u,
                                                  chunk_bytes, &summary, stream);
        if (rc == CHIP_OK) cursor_ += summary.out_len;
        return rc;
    }
    // chip_zstd_parallel_next into this buffer's spare capacity: the next part of ONE zstd frame of any length.  `slab` holds `len` bytes of
    // the frame from byte cur.in_total on (from offset `from` of the buffer: the caller keeps what a call did not consume and moves on by
    // summary.in_used), `state` is the cursor's DEVICE memory: CHIP_ZCUR_CARRY_BYTES and the window (summary.need_state says how much when
    // it is too small).  The cursor of this buffer moves by summary.out_len; summary.status says why the call stopped.  Synchronous on `stream`.
    int zstd_parallel_next(chip_zstd_cursor &cur, DeviceBuffer &state, const DeviceBuffer &slab, uint64_t from, uint64_t len, int window_log_max,
                           uint32_t flags, chip_zstd_next_summary &summary, void *stream = nullptr)
    {
        if (from > slab.len() || len > slab.len() - from) return CHIP_E_INVALID;
        const size_t room = cap_ - cursor_;
        const int rc = chip_zstd_parallel_next(&cur, state.buf_, state.cap_, slab.data() + from, len, buf_ + cursor_, room < 0x7FFFFFFFu ? room : 0x7FFFFFFFu,
                                               window_log_max, flags, &summary, stream);
        if (rc == CHIP_OK) cursor_ += summary.out_len;
        return rc;
    }
    // chip_select_units: the index step of read_ranges alone (DEVICE arrays, HOST summary), for a caller that decodes the sub-batch
    // sel_in_off / sel_in_len / sel_out_off / sel_out_cap into summary.scratch_bytes of its own.  max_sel 0 with null sel arrays
    // counts.  Synchronous on `stream`.
    static int select_units(size_t n_units, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap,
                            size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, uint64_t max_sel, uint32_t *sel_unit,
                            uint64_t *sel_in_off, uint32_t *sel_in_len, uint64_t *sel_out_off, uint32_t *sel_out_cap, uint64_t *src_off,
                            uint64_t *dst_off, int32_t *range_status, chip_select_summary &summary, void *stream = nullptr)
    {
        return chip_select_units(n_units, in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len, max_sel, sel_unit, sel_in_off, sel_in_len,
                                 sel_out_off, sel_out_cap, src_off, dst_off, range_status, &summary, stream);
    }
    // a whole BGZF file of htslib's block payload
    int bgzf_write(int level, const DeviceBuffer &in, uint64_t len, chip_file_summary &summary, void *stream = nullptr)
    {
        return encode_file(CHIP_FMT_BGZF, level, 0, 0, in, len, summary, stream);
    }

private:
    uint8_t *buf_;
    size_t cap_;
    size_t cursor_ = 0;
};

// chip_bgzf_plan_host: the BGZF walk over host memory (no device needed); the arrays are what chip_decode_batch_host / _multi take.
inline int bgzf_plan_host(const uint8_t *in, uint64_t len, uint64_t max_blocks, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                          uint32_t *out_cap, chip_bgzf_summary &summary)
{
    return chip_bgzf_plan_host(in, len, max_blocks, in_off, in_len, out_off, out_cap, &summary);
}
// chip_select_units_host: the units that byte ranges of a plan's content touch, on host memory (no device needed).
inline int select_units_host(size_t n_units, const uint64_t *in_off, const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap,
                             size_t n_ranges, const uint64_t *range_lo, const uint32_t *range_len, uint64_t max_sel, uint32_t *sel_unit,
                             uint64_t *sel_in_off, uint32_t *sel_in_len, uint64_t *sel_out_off, uint32_t *sel_out_cap, uint64_t *src_off,
                             uint64_t *dst_off, int32_t *range_status, chip_select_summary &summary)
{
    return chip_select_units_host(n_units, in_off, in_len, out_off, out_cap, n_ranges, range_lo, range_len, max_sel, sel_unit, sel_in_off, sel_in_len,
                                  sel_out_off, sel_out_cap, src_off, dst_off, range_status, &summary);
}
// chip_inflate_index_units_host: the chunks of a checkpoint index by host arithmetic (no device needed); every output array may be nullptr.
inline int inflate_index_units_host(int format, uint64_t len, uint64_t n_points, const uint64_t *pt_bit, const uint64_t *pt_out,
                                    const uint32_t *pt_check, uint64_t total_out, uint64_t *in_off, uint32_t *in_len, uint32_t *out_cap,
                                    uint32_t *win_len, uint32_t *resume, int32_t &status, uint64_t &bad_index)
{
    return chip_inflate_index_units_host(format, len, n_points, pt_bit, pt_out, pt_check, total_out, in_off, in_len, out_cap, win_len, resume, &status,
                                         &bad_index);
}
// chip_zstd_plan_host: the zstd frame walk over host memory (no device needed); the arrays are what chip_decode_batch_host / _multi take.
inline int zstd_plan_host(const uint8_t *in, uint64_t len, uint64_t max_frames, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                          uint32_t *out_cap, chip_zstd_plan_summary &summary)
{
    return chip_zstd_plan_host(in, len, max_frames, in_off, in_len, out_off, out_cap, &summary);
}
// The host twins of chip_zstd_parallel_next's steps (no device needed): the walk from a block boundary, the header step, the running XXH64.
inline int zstd_slab_blocks_host(const uint8_t *in, uint64_t len, uint64_t block_max, uint64_t max_blocks, chip_zstd_block *blocks,
                                 chip_zstd_slab_summary &summary)
{
    return chip_zstd_slab_blocks_host(in, len, block_max, max_blocks, blocks, &summary);
}
inline int zstd_cursor_header_host(chip_zstd_cursor &cur, const uint8_t *in, uint64_t len, int window_log_max, uint32_t flags, uint32_t &header_bytes,
                                   uint64_t &need_state)
{
    return chip_zstd_cursor_header_host(&cur, in, len, window_log_max, flags, &header_bytes, &need_state);
}
inline int xxh64_update_host(chip_xxh64_state &st, const uint8_t *data, uint64_t len) { return chip_xxh64_update_host(&st, data, len); }
inline uint64_t xxh64_digest_host(const chip_xxh64_state &st) { return chip_xxh64_digest_host(&st); }
// htslib's 28-byte EOF marker, to be written behind the last block of a file made with chip_encode_batch(CHIP_FMT_BGZF, ..) (DeviceBuffer::
// bgzf_write does all of it)
inline const uint8_t *bgzf_eof_block(size_t &len) { return chip_bgzf_eof_block(&len); }

}  // namespace compu
