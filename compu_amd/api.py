"""Host-side mirror of compu's Decoder / Encoder surface over libcompu_hip.so (ctypes).

Names follow the reference: decoder::{Interface, Decoder, Decode, DecodeStatus, DecodeError,
Detection, ZlibMode, ZstdOptions} (src/decoder/mod.rs, zlib_common.rs, zstd.rs),
encoder::{Interface, Encoder, Encode, EncodeOp, EncodeStatus, ZlibOptions} (src/encoder/mod.rs,
zlib_common.rs) and Buffer (src/buffer.rs).  All codec work happens in the HIP library; its structures, prototypes and
lib() are in _ffi.py.
"""
import ctypes as C
import enum

from ._ffi import (  # noqa: F401
    _BgzfSummary,
    _BrotliEncoderOpts,
    _DecodeResult,
    _DecoderOpts,
    _EncodeResult,
    _EncoderOpts,
    _FileSummary,
    _GzipPlanSummary,
    _InflateCursor,
    _InflateIndexSummary,
    _InflateNextSummary,
    _InflateParallelSummary,
    _Lz4Block,
    _Lz4BlocksSummary,
    _Lz4ParallelSummary,
    _ReadSummary,
    _SelectSummary,
    _TarEntry,
    _TarPlanSummary,
    _TarSource,
    _TarWriteSummary,
    _Xxh64State,
    _ZipDecodeSummary,
    _ZipEntry,
    _ZipPlanSummary,
    _ZipSource,
    _ZipWriteSummary,
    _ZstdBlock,
    _ZstdBlocksSummary,
    _ZstdCursor,
    _ZstdEncoderOpts,
    _ZstdNextSummary,
    _ZstdParallelSummary,
    _ZstdPlanSummary,
    _ZstdSeekSummary,
    _ZstdSlabSummary,
    lib,
    lib_path,
)

# ---- enums and result types ----------------------------------------------------------------


class DecodeStatus(enum.IntEnum):
    """src/decoder/mod.rs:139-146"""

    NeedInput = 0
    NeedOutput = 1
    Finished = 2


class DecodeError(Exception):
    """src/decoder/mod.rs:117-135: transparent wrapper of the backend's i32 code."""

    def __init__(self, code=0):
        super().__init__(code)
        self.code = int(code)

    @classmethod
    def no_error(cls):
        return cls(0)

    def as_raw(self):
        return self.code

    def __eq__(self, other):
        return isinstance(other, DecodeError) and other.code == self.code

    def __hash__(self):
        return hash(("DecodeError", self.code))

    def __repr__(self):
        return f"DecodeError({self.code})"


class Decode:
    """src/decoder/mod.rs:150-157; ``status`` is a DecodeStatus (Ok) or a DecodeError (Err)."""

    __slots__ = ("input_remain", "output_remain", "status")

    def __init__(self, input_remain, output_remain, status):
        self.input_remain = input_remain
        self.output_remain = output_remain
        self.status = status

    def is_ok(self):
        return isinstance(self.status, DecodeStatus)

    def __repr__(self):
        return f"Decode(input_remain={self.input_remain}, output_remain={self.output_remain}, status={self.status!r})"


class ZlibMode(enum.IntEnum):
    """src/decoder/zlib_common.rs:4-15 (decoder default Auto) / src/encoder/zlib_common.rs:28-37"""

    Deflate = -15
    Zlib = 15
    Gzip = 31
    Auto = 47


FMT_ZSTD = 100
FMT_BROTLI = 101  # Interface::brotli_c decoder and encoder
FMT_LZ4_BLOCK = 102  # CHIP_FMT_LZ4_BLOCK: one raw LZ4 block per unit (the batch calls, decode and encode)
FMT_LZ4 = 103  # CHIP_FMT_LZ4: one LZ4 frame per unit (the batch calls, decode and encode; encode_file writes one frame)


class ZstdOptions:
    """src/decoder/zstd.rs:22-74"""

    def __init__(self):
        self._window_log = 0

    def window_log(self, window_log):
        assert 10 <= window_log <= 31  # ZSTD_WINDOWLOG_MIN .. ZSTD_WINDOWLOG_MAX_64, zstd.rs:40-47
        self._window_log = window_log
        return self


class EncodeOp(enum.IntEnum):
    """src/encoder/mod.rs:12-23"""

    Process = 0
    Flush = 1
    Finish = 2


class EncodeStatus(enum.IntEnum):
    """src/encoder/mod.rs:27-38"""

    Continue = 0
    NeedOutput = 1
    Finished = 2
    Error = 3


class Encode:
    """src/encoder/mod.rs:42-49"""

    __slots__ = ("input_remain", "output_remain", "status")

    def __init__(self, input_remain, output_remain, status):
        self.input_remain = input_remain
        self.output_remain = output_remain
        self.status = status

    def __repr__(self):
        return f"Encode(input_remain={self.input_remain}, output_remain={self.output_remain}, status={self.status!r})"


class ZlibStrategy(enum.IntEnum):
    """src/encoder/zlib_common.rs:5-24"""

    Default = 0
    Filtered = 1
    HuffmanOnly = 2
    Rle = 3
    Fixed = 4


class ZstdStrategy(enum.IntEnum):
    """src/encoder/zstd.rs:33-56"""

    Default = 0
    Fast = 1
    DFast = 2
    Greedy = 3
    Lazy = 4
    Lazy2 = 5
    BtLazy2 = 6
    BtOpt = 7
    BtUltra = 8
    BtUltra2 = 9


class ZstdEncoderOptions:
    """The encoder's ZstdOptions, src/encoder/zstd.rs:62-126 (defaults: level 3, strategy Default, window_log 27).  The decoder's
    options are ZstdOptions."""

    def __init__(self):
        self._level = 3
        self._strategy = ZstdStrategy.Default
        self._window_log = 27

    def level(self, level):
        assert -131072 <= level <= 131072  # +-ZSTD_TARGETLENGTH_MAX, zstd.rs:82-83
        self._level = level
        return self

    def strategy(self, strategy):
        self._strategy = strategy
        return self

    def window_log(self, window_log):
        assert 10 <= window_log <= 31  # ZSTD_WINDOWLOG_MIN .. ZSTD_WINDOWLOG_MAX_64, zstd.rs:96-101
        self._window_log = window_log
        return self


class BrotliEncoderMode(enum.IntEnum):
    """src/encoder/brotli_common.rs: compu's raw mode byte, handed to BROTLI_PARAM_MODE unchanged"""

    Generic = 1
    Text = 2
    Font = 3


class BrotliOptions:
    """The encoder's BrotliOptions, src/encoder/brotli_common.rs (defaults: quality and mode unset, i.e. libbrotlienc's quality
    11).  The GPU encoder accepts and records the mode; it has no mode-dependent modelling."""

    def __init__(self):
        self._quality = 0
        self._mode = 0

    def quality(self, quality):
        assert quality > 0
        assert quality <= 11
        self._quality = quality
        return self

    def mode(self, mode):
        self._mode = int(mode)
        return self


class ZlibOptions:
    """src/encoder/zlib_common.rs:47-103 (defaults: Gzip, Default strategy, mem_level 8, level 9: zlib_common.rs:59-66)"""

    def __init__(self):
        self._mode = ZlibMode.Gzip
        self._compression = 9
        self._strategy = ZlibStrategy.Default
        self._mem_level = 8

    def strategy(self, strategy):
        self._strategy = ZlibStrategy(strategy)
        return self

    def mem_level(self, mem_level):
        # the reference's setter asserts `mem_level > MAX_MEM_LEVEL` (an inverted check, zlib_common.rs:88); the value that
        # reaches deflateInit2_ must be 1..9, which is what the backend accepts
        assert 0 < mem_level <= 9
        self._mem_level = mem_level
        return self

    def mode(self, mode):
        assert mode in (ZlibMode.Deflate, ZlibMode.Zlib, ZlibMode.Gzip)
        self._mode = ZlibMode(mode)
        return self

    def compression(self, level):
        assert -1 <= level <= 9  # -1 = zlib's default (zlib_common.rs:96-103)
        self._compression = level
        return self


class Detection(enum.IntEnum):
    """src/decoder/mod.rs:9-21; detect() returns None when there are too few bytes (mod.rs:97-104)."""

    Zstd = 0
    Gzip = 1
    Zlib = 2
    Unknown = 3

    @staticmethod
    def detect(data):
        data = bytes(data)
        k = lib().chip_detect(data if data else b"\0", len(data))
        return None if k < 0 else Detection(k)


# ---- Vec<u8> stand-in so decode_vec / decode_vec_full read like the reference -----------------


class Vec:
    """A byte vector with explicit capacity (Rust's Vec<u8>: len() <= capacity())."""

    def __init__(self, capacity=0):
        import numpy as np

        self._buf = np.zeros(capacity, np.uint8)
        self._len = 0

    @classmethod
    def with_capacity(cls, capacity):
        return cls(capacity)

    def __len__(self):
        return self._len

    def capacity(self):
        return self._buf.size

    def try_reserve_exact(self, additional):
        import numpy as np

        need = self._len + additional
        if need > self._buf.size:
            grown = np.zeros(need, np.uint8)
            grown[: self._len] = self._buf[: self._len]
            self._buf = grown

    reserve = try_reserve_exact

    def spare_capacity_len(self):
        return self._buf.size - self._len

    def set_len(self, n):
        assert n <= self._buf.size
        self._len = n

    def clear(self):
        self._len = 0

    def truncate(self, n):
        self._len = min(self._len, n)

    def extend_from_slice(self, data):
        import numpy as np

        self.try_reserve_exact(len(data))
        self._buf[self._len : self._len + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
        self._len += len(data)

    def __bytes__(self):
        return self._buf[: self._len].tobytes()

    def __eq__(self, other):
        return bytes(self) == bytes(other)


def _in_ptr(data):
    """(keepalive, pointer, length) for a read-only bytes-like; never a NULL pointer (mod.rs:283)."""
    import numpy as np

    if not isinstance(data, (bytes, bytearray)):
        data = bytes(memoryview(data).cast("B"))
    n = len(data)
    if n == 0:
        keep = np.zeros(1, np.uint8)
        return keep, C.c_void_p(keep.ctypes.data), 0
    keep = np.frombuffer(data, dtype=np.uint8)
    return keep, C.c_void_p(keep.ctypes.data), n


def _out_ptr(buf, offset, length):
    import numpy as np

    if length == 0:
        keep = np.zeros(1, np.uint8)
        return keep, C.c_void_p(keep.ctypes.data)
    keep = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, dtype=np.uint8)
    assert keep.flags.writeable and offset + length <= keep.size
    return keep, C.c_void_p(keep.ctypes.data + offset)


# ---- Decoder ---------------------------------------------------------------------------------


class Decoder:
    """src/decoder/mod.rs:269-455 over a chip_decoder instance."""

    def __init__(self, handle, fmt):
        self._h = handle
        self._fmt = fmt

    # raw_decode / decode, mod.rs:290-317
    def decode(self, input, output, out_offset=0, out_len=None):
        """Decode `input` into the writable buffer `output[out_offset : out_offset+out_len]`."""
        if out_len is None:
            out_len = len(output) - out_offset
        k1, ip, n = _in_ptr(input)
        k2, op = _out_ptr(output, out_offset, out_len)
        r = lib().chip_decode(self._h, ip, n, op, out_len)
        del k1, k2
        st = DecodeError(r.err) if r.err else DecodeStatus(r.status)
        return Decode(r.input_remain, r.output_remain, st)

    # mod.rs:323-335
    def decode_vec(self, input, output):
        spare = output.spare_capacity_len()
        result = self.decode(input, output._buf, len(output), spare)
        if result.is_ok():
            output.set_len(len(output) + spare - result.output_remain)
        return result

    # mod.rs:360-385
    def decode_vec_full(self, input, output):
        RESERVE_DEFAULT = 1024
        input = bytes(input)
        input_len = len(input)
        if input_len < RESERVE_DEFAULT:
            output.try_reserve_exact(input_len)
            reserve_size = input_len // 3
        elif input_len < RESERVE_DEFAULT * 16:
            output.try_reserve_exact(input_len + input_len // 3)
            reserve_size = RESERVE_DEFAULT
        else:
            output.try_reserve_exact(input_len * 2)
            reserve_size = RESERVE_DEFAULT * 8
        while True:
            result = self.decode_vec(input, output)
            if result.status == DecodeStatus.NeedOutput:
                input = input[len(input) - result.input_remain :]
                output.try_reserve_exact(reserve_size)
                continue
            return result

    # mod.rs:433-441
    def reset(self):
        h = lib().chip_decoder_reset(self._h)
        if h:
            self._h = h
            return True
        return False

    def footprint(self):
        """(pinned host bytes, device bytes) this decoder holds right now (chip_decoder_footprint)."""
        a, b = C.c_size_t(0), C.c_size_t(0)
        lib().chip_decoder_footprint(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    # mod.rs:445-447
    def describe_error(self, error):
        s = lib().chip_decoder_strerror(self._fmt, error.as_raw())
        return None if s is None else s.decode()

    def close(self):
        if self._h:
            lib().chip_decoder_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class decoder_interface:
    """decoder::Interface constructors of the `hip` variant."""

    @staticmethod
    def zlib_hip(mode=ZlibMode.Auto, device=-1):
        """Interface::zlib_ng(mode), src/decoder/zlib_ng.rs:61-90; None on failure."""
        opts = _DecoderOpts(0, device)
        h = lib().chip_decoder_new(int(mode), C.byref(opts))
        return Decoder(h, int(mode)) if h else None

    @staticmethod
    def zstd_hip(opts=None, device=-1):
        """Interface::zstd(opts), src/decoder/zstd.rs:81-94; None on failure."""
        o = _DecoderOpts(opts._window_log if opts else 0, device)
        h = lib().chip_decoder_new(FMT_ZSTD, C.byref(o))
        return Decoder(h, FMT_ZSTD) if h else None

    @staticmethod
    def brotli_hip(device=-1):
        """Interface::brotli_c(), src/decoder/brotli_c.rs:17-27; None on failure."""
        o = _DecoderOpts(0, device)
        h = lib().chip_decoder_new(FMT_BROTLI, C.byref(o))
        return Decoder(h, FMT_BROTLI) if h else None


# ---- Encoder ---------------------------------------------------------------------------------


class Encoder:
    """src/encoder/mod.rs:148-323 over a chip_encoder instance."""

    def __init__(self, handle):
        self._h = handle

    # raw_encode / encode, mod.rs:171-199
    def encode(self, input, output, op, out_offset=0, out_len=None):
        if out_len is None:
            out_len = len(output) - out_offset
        k1, ip, n = _in_ptr(input)
        k2, outp = _out_ptr(output, out_offset, out_len)
        r = lib().chip_encode(self._h, ip, n, outp, out_len, int(op))
        del k1, k2
        return Encode(r.input_remain, r.output_remain, EncodeStatus(r.status))

    # mod.rs:203-213 (sets the length even on Error)
    def encode_vec(self, input, output, op):
        spare = output.spare_capacity_len()
        result = self.encode(input, output._buf, op, len(output), spare)
        output.set_len(len(output) + spare - result.output_remain)
        return result

    # mod.rs:239-267: reserve policy, then loop on NeedOutput (and on Continue while finishing)
    def encode_vec_full(self, input, output, op):
        RESERVE_DEFAULT = 1024
        input = bytes(input)
        input_len = len(input)
        if input_len < RESERVE_DEFAULT:
            output.try_reserve_exact(input_len)
            reserve_size = input_len // 3
        elif input_len < RESERVE_DEFAULT * 16:
            output.try_reserve_exact(input_len // 2)
            reserve_size = RESERVE_DEFAULT
        else:
            output.try_reserve_exact(input_len // 3)
            reserve_size = RESERVE_DEFAULT * 8
        while True:
            result = self.encode_vec(input, output, op)
            if result.status == EncodeStatus.NeedOutput:
                input = input[len(input) - result.input_remain :]
                # the reference reserves `reserve_size` (0 for inputs under 3 bytes, where it would
                # spin); keep at least one byte of progress
                output.try_reserve_exact(max(reserve_size, 1))
                continue
            if result.status == EncodeStatus.Continue and op == EncodeOp.Finish:
                input = input[len(input) - result.input_remain :]
                continue
            return result

    # mod.rs:314-321
    def reset(self):
        h = lib().chip_encoder_reset(self._h)
        if h:
            self._h = h
            return True
        return False

    def close(self):
        if self._h:
            lib().chip_encoder_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class encoder_interface:
    @staticmethod
    def zlib_hip(opts=None, device=-1):
        """Interface::zlib_ng(opts), src/encoder/zlib_ng.rs:50-87; None on failure."""
        opts = opts or ZlibOptions()
        o = _EncoderOpts(int(opts._mode), opts._compression, device, int(opts._strategy), opts._mem_level)
        h = lib().chip_encoder_new(C.byref(o))
        return Encoder(h) if h else None

    @staticmethod
    def zstd_hip(opts=None, device=-1):
        """Interface::zstd(opts), src/encoder/zstd.rs:138-160; None when an option is out of range (apply() failing)."""
        opts = opts or ZstdEncoderOptions()
        o = _ZstdEncoderOpts(int(opts._level), int(opts._strategy), int(opts._window_log), device)
        h = lib().chip_encoder_new_zstd(C.byref(o))
        return Encoder(h) if h else None

    @staticmethod
    def brotli_hip(opts=None, device=-1, lgwin=22):
        """Interface::brotli_c(opts), src/encoder/brotli_c.rs:38-50 (lgwin: libbrotlienc's default 22, which compu never
        changes); None on failure."""
        opts = opts or BrotliOptions()
        o = _BrotliEncoderOpts(int(opts._quality), int(opts._mode), int(lgwin), device)
        h = lib().chip_encoder_new_brotli(C.byref(o))
        return Encoder(h) if h else None


# ---- Buffer<N>, src/buffer.rs ---------------------------------------------------------------


class Buffer:
    """Fixed-size buffer with a cursor (src/buffer.rs:1-49)."""

    def __init__(self, n):
        import numpy as np

        self._buf = np.zeros(n, np.uint8)
        self.cursor = 0

    def data(self):
        return self._buf[: self.cursor].tobytes()

    def consume(self):
        self.cursor = 0

    # decoder/mod.rs:507-531
    def decode(self, decoder, input):
        spare = len(self._buf) - self.cursor
        result = decoder.decode(input, self._buf, self.cursor, spare)
        if isinstance(result.status, DecodeError):
            raise result.status
        self.cursor = self.cursor + spare - result.output_remain
        return len(input) - result.input_remain, result.status

    # encoder/mod.rs:395-412
    def encode(self, encoder, input, op):
        spare = len(self._buf) - self.cursor
        result = encoder.encode(input, self._buf, op, self.cursor, spare)
        self.cursor = self.cursor + spare - result.output_remain
        return len(input) - result.input_remain, result.status


class PinnedBuffer(Buffer):
    """Buffer<N>'s cursor API (src/buffer.rs:1-49) over page-locked host memory (chip_pinned_alloc = hipHostMalloc): the
    north star's pinned-host buffer type.  Used like Buffer with the streaming Decoder / Encoder."""

    def __init__(self, n):
        import numpy as np

        self._ptr = lib().chip_pinned_alloc(n)
        if not self._ptr:
            raise MemoryError("chip_pinned_alloc failed")
        self._buf = np.ctypeslib.as_array((C.c_uint8 * n).from_address(self._ptr))
        self.cursor = 0

    def close(self):
        if getattr(self, "_ptr", None):
            self._buf = None
            lib().chip_pinned_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """The north star's device buffer type: GPU memory (chip_device_alloc = hipMalloc, where src/mem.rs routes device
    allocations) with Buffer<N>'s cursor.  upload() appends host bytes, decode_batch() appends decoded units behind the
    cursor without the data touching the host, download() reads back."""

    def __init__(self, n):
        self._cap = n
        self._ptr = lib().chip_device_alloc(n + 16)
        if not self._ptr:
            raise MemoryError("chip_device_alloc failed")
        self.cursor = 0

    def ptr(self, offset=0):
        return self._ptr + offset

    def __len__(self):
        return self.cursor

    def capacity(self):
        return self._cap

    def spare_capacity_len(self):
        return self._cap - self.cursor

    def consume(self):
        self.cursor = 0

    def upload(self, data):
        k, ip, n = _in_ptr(data)
        if n > self._cap - self.cursor:
            raise ValueError("does not fit")
        L = lib()
        if n and (L.chip_memcpy_h2d(self._ptr + self.cursor, ip, n, None) != 0 or L.chip_stream_sync(None) != 0):
            raise RuntimeError("upload failed")
        self.cursor += n
        return n

    def download(self, offset=0, n=None):
        import numpy as np

        n = self.cursor - offset if n is None else n
        assert offset + n <= self.cursor
        out = np.empty(n, np.uint8)
        L = lib()
        if n and (L.chip_memcpy_d2h(out.ctypes.data, self._ptr + offset, n, None) != 0 or L.chip_stream_sync(None) != 0):
            raise RuntimeError("download failed")
        return out

    def decode_batch(self, fmt, src, in_off, in_len, out_off, out_cap, span):
        """chip_decode_batch from DeviceBuffer `src` into this buffer's spare capacity (out_off relative to it); the
        per-unit arrays are host sequences, uploaded here.  Returns (out_len, in_used, status) as numpy arrays."""
        import numpy as np

        n = len(in_len)
        if span > self._cap - self.cursor:
            raise ValueError("does not fit")
        host = np.zeros(n * 10 + 16, np.uint32)
        host[: 2 * n].view(np.uint64)[:] = np.asarray(in_off, np.uint64)
        host[2 * n : 4 * n].view(np.uint64)[:] = np.asarray(out_off, np.uint64)
        host[4 * n : 5 * n] = np.asarray(in_len, np.uint32)
        host[5 * n : 6 * n] = np.asarray(out_cap, np.uint32)
        arr = DeviceBuffer(host.nbytes)
        arr.upload(host)
        a = arr.ptr()
        L = lib()
        rc = L.chip_decode_batch(int(fmt), n, src.ptr(), a, a + 16 * n, self._ptr + self.cursor, a + 8 * n, a + 20 * n, a + 24 * n, a + 28 * n,
                                 a + 32 * n, None)
        if rc != 0 or L.chip_stream_sync(None) != 0:
            raise RuntimeError(f"chip_decode_batch failed: {rc}")
        self.cursor += span
        res = arr.download(24 * n, 12 * n).view(np.uint32)
        arr.close()
        return res[:n].copy(), res[n : 2 * n].copy(), res[2 * n :].view(np.int32).copy()

    def close(self):
        if getattr(self, "_ptr", None):
            lib().chip_device_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- batched entry points on torch CUDA tensors -----------------------------------------------


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _stream_ptr(stream):
    if stream is None:
        import torch

        stream = torch.cuda.current_stream()
    return C.c_void_p(getattr(stream, "cuda_stream", stream))


def _check_tensors(pairs):
    """Every tensor handed to a device batch call: on one GPU, contiguous, of the dtype the kernel reads it as (a CPU
    tensor or int32 offsets would otherwise be read as device u64 offsets: a GPU fault instead of a Python error)."""
    dev = pairs[0][0].device
    for t, dt in pairs:
        if not (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.device == dev):
            raise TypeError(f"expected a contiguous {dt} tensor on {dev}, got {t.dtype} on {t.device} (contiguous={t.is_contiguous()})")
    return dev


F_COMPU_STATUS = 1  # CHIP_F_COMPU_STATUS
F_MEMBERS = 2  # CHIP_F_MEMBERS: a unit is a series of gzip members / zstd frames (gzip, auto, zstd and detect batches; not with F_COMPU_STATUS)


def decode_batch(fmt, in_buf, in_off, in_len, out_buf, out_off, out_cap, out_len=None, in_used=None, status=None, stream=None, flags=0):
    """chip_decode_batch[_ex] on device tensors: in_buf/out_buf uint8, *_off int64 (read as u64),
    in_len/out_cap/out_len/in_used int32 (read as u32), status int32.  Only enqueues."""
    import torch

    n = in_len.numel()
    dev = in_buf.device
    if out_len is None:
        out_len = torch.empty(n, dtype=torch.int32, device=dev)
    if in_used is None:
        in_used = torch.empty(n, dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    _check_tensors(((in_buf, torch.uint8), (out_buf, torch.uint8), (in_off, torch.int64), (out_off, torch.int64), (in_len, torch.int32),
                    (out_cap, torch.int32), (out_len, torch.int32), (in_used, torch.int32), (status, torch.int32)))
    with torch.cuda.device(dev):  # scratch and the stream come from the tensors' device, not whatever is current
        rc = lib().chip_decode_batch_ex(int(fmt), int(flags), n, _dp(in_buf), _dp(in_off), _dp(in_len), _dp(out_buf), _dp(out_off), _dp(out_cap),
                                        _dp(out_len), _dp(in_used), _dp(status), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_decode_batch failed: {rc}")
    return out_len, in_used, status


def decode_batch_sizes(fmt, in_buf, in_off, in_len, out_size=None, in_used=None, status=None, stream=None, flags=0):
    """chip_decode_batch_sizes on device tensors: the decoded length of every unit without decoding it (no output buffer).
    in_buf uint8, in_off int64 (read as u64), in_len / in_used int32 (read as u32), out_size int64 (read as u64), status int32.
    Only enqueues.  Returns (out_size, in_used, status)."""
    import torch

    n = in_len.numel()
    dev = in_buf.device
    if out_size is None:
        out_size = torch.empty(n, dtype=torch.int64, device=dev)
    if in_used is None:
        in_used = torch.empty(n, dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    _check_tensors(((in_buf, torch.uint8), (in_off, torch.int64), (in_len, torch.int32), (out_size, torch.int64), (in_used, torch.int32),
                    (status, torch.int32)))
    with torch.cuda.device(dev):
        rc = lib().chip_decode_batch_sizes(int(fmt), int(flags), n, _dp(in_buf), _dp(in_off), _dp(in_len), _dp(out_size), _dp(in_used),
                                           _dp(status), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_decode_batch_sizes failed: {rc}")
    return out_size, in_used, status


def decode_batch_host(fmt, in_buf, in_off, in_len, out_buf, out_off, out_cap, device=-1, slice_bytes=0):
    """chip_decode_batch_host over numpy arrays in host memory (pinned or not): returns (out_len, in_used, status)."""
    import numpy as np

    n = len(in_len)
    in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
    in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_len = np.zeros(n, np.uint32)
    in_used = np.zeros(n, np.uint32)
    status = np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().chip_decode_batch_host(int(fmt), n, p(in_buf), p(in_off), p(in_len), p(out_buf), p(out_off), p(out_cap), p(out_len), p(in_used),
                                      p(status), int(device), int(slice_bytes))
    if rc != 0:
        raise RuntimeError(f"chip_decode_batch_host failed: {rc}")
    return out_len, in_used, status


def decode_batch_multi(fmt, in_buf, in_off, in_len, out_buf, out_off, out_cap, devices=None, slice_bytes=0):
    """chip_decode_batch_multi: host-memory units partitioned over `devices` (None = every visible GPU), one host
    thread and two streams per device, a CHIP_FMT_DETECT batch bucketed by format first.  Returns (out_len, in_used, status)."""
    import numpy as np

    n = len(in_len)
    in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
    in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_len = np.zeros(n, np.uint32)
    in_used = np.zeros(n, np.uint32)
    status = np.zeros(n, np.int32)
    devs = np.ascontiguousarray(devices if devices is not None else [], dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().chip_decode_batch_multi(int(fmt), n, p(in_buf), p(in_off), p(in_len), p(out_buf), p(out_off), p(out_cap), p(out_len), p(in_used),
                                       p(status), p(devs) if len(devs) else None, len(devs), int(slice_bytes))
    if rc != 0:
        raise RuntimeError(f"chip_decode_batch_multi failed: {rc}")
    return out_len, in_used, status


def encode_batch_host(fmt, level, in_buf, in_off, in_len, out_buf, out_off, out_cap, device=-1, slice_bytes=0):
    """chip_encode_batch_host over numpy arrays in host memory: returns (out_len, status)."""
    import numpy as np

    n = len(in_len)
    in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
    in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.uint32)
    out_len = np.zeros(n, np.uint32)
    status = np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().chip_encode_batch_host(int(fmt), int(level), n, p(in_buf), p(in_off), p(in_len), p(out_buf), p(out_off), p(out_cap), p(out_len),
                                      p(status), int(device), int(slice_bytes))
    if rc != 0:
        raise RuntimeError(f"chip_encode_batch_host failed: {rc}")
    return out_len, status


def trim():
    """Give the inflate kernel's cached token scratch of the current device back (chip_trim)."""
    rc = lib().chip_trim()
    if rc != 0:
        raise RuntimeError(f"chip_trim failed: {rc}")


def detect_batch(in_buf, in_off, in_len, kind=None, stream=None):
    import torch

    n = in_len.numel()
    if kind is None:
        kind = torch.empty(n, dtype=torch.int32, device=in_buf.device)
    dev = _check_tensors(((in_buf, torch.uint8), (in_off, torch.int64), (in_len, torch.int32), (kind, torch.int32)))
    with torch.cuda.device(dev):
        rc = lib().chip_detect_batch(n, _dp(in_buf), _dp(in_off), _dp(in_len), _dp(kind), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_detect_batch failed: {rc}")
    return kind


def encode_bound(fmt, in_len):
    return lib().chip_encode_bound(int(fmt), int(in_len))


def encode_batch(fmt, level, in_buf, in_off, in_len, out_buf, out_off, out_cap, out_len=None, status=None, stream=None, strategy=0):
    """chip_encode_batch_ex over device tensors: level 0 stored, 1 fixed Huffman, 2..9 (-1 = 6) dynamic Huffman blocks; FMT_ZSTD:
    zstd levels and ZstdStrategy values; FMT_BROTLI: level = quality 0..11 (0 = 11), strategy = mode 0..3, lgwin 22; FMT_BGZF: levels and
    strategies as ZlibMode.Gzip, one BGZF block per unit, a unit above 65280 bytes is EncodeStatus.Error with out_len 0;
    FMT_LZ4_BLOCK / FMT_LZ4: levels -1 .. 12, one raw block / one frame per unit, strategy 0 for blocks and LZ4_S_* bits for frames."""
    import torch

    n = in_len.numel()
    dev = in_buf.device
    if out_len is None:
        out_len = torch.empty(n, dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    _check_tensors(((in_buf, torch.uint8), (out_buf, torch.uint8), (in_off, torch.int64), (out_off, torch.int64), (in_len, torch.int32),
                    (out_cap, torch.int32), (out_len, torch.int32), (status, torch.int32)))
    with torch.cuda.device(dev):
        rc = lib().chip_encode_batch_ex(int(fmt), int(level), int(strategy), n, _dp(in_buf), _dp(in_off), _dp(in_len), _dp(out_buf), _dp(out_off),
                                        _dp(out_cap), _dp(out_len), _dp(status), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_encode_batch failed: {rc}")
    return out_len, status


# ---- summaries: a chip_*_summary structure as Python values ------------------------------------
#
# A summary class is its docstring and `__slots__ = FIELDS = _fields(_TheStructure)` (FIELDS alone: its values can be
# assigned), ENUMS for the fields that are wrapped in an enum and FORMATS for those that repr() prints in another base.


def _fields(raw_cls):
    """The field names of a ctypes structure, in its order, without the padding."""
    return tuple(name for name, _ in raw_cls._fields_ if name != "pad")


class _Record:
    """__init__(raw) and __repr__ over FIELDS: int() of every field, or the enum ENUMS names for it; repr() prints an enum by
    its name and a field of FORMATS with that format."""

    __slots__ = ()
    ENUMS, FORMATS = {}, {}

    def __init__(self, raw):
        for name in self.FIELDS:
            setattr(self, name, self.ENUMS.get(name, int)(getattr(raw, name)))

    def __repr__(self):
        show = lambda name, v: v.name if name in self.ENUMS else format(v, self.FORMATS.get(name, ""))  # noqa: E731
        return f"{type(self).__name__}(" + ", ".join(f"{name}={show(name, getattr(self, name))}" for name in self.FIELDS) + ")"


class _Summary(_Record):
    """A _Record with as_tuple(): the fields in order, enums as int."""

    __slots__ = ()

    def as_tuple(self):
        return tuple(int(getattr(self, name)) for name in self.FIELDS)


# ---- BGZF: from a file to a batch and back (include/compu_hip.h, "BGZF") ------------------------

FMT_BGZF = 131  # CHIP_FMT_BGZF: encode_batch / encode_batch_host / encode_bound only, one BGZF block per unit


class BgzfStatus(enum.IntEnum):
    Ok = 0
    Truncated = 1
    BadHeader = 2


class BgzfSummary(_Summary):
    """chip_bgzf_summary: n_blocks and total_out of the whole walk, in_used where it stopped, status why, eof = the last block
    has ISIZE 0."""

    __slots__ = FIELDS = _fields(_BgzfSummary)
    ENUMS = {"status": BgzfStatus}


def bgzf_eof_block():
    """htslib's 28-byte EOF marker (chip_bgzf_eof_block)."""
    n = C.c_size_t(0)
    p = lib().chip_bgzf_eof_block(C.byref(n))
    return C.string_at(p, n.value)


def _count_then_fill(fn, call, count, alloc, ptr, max_units):
    """The protocol of every plan.  `call(m, *pointers)` makes the C call `fn` with room for m units, `count()` reads how many there
    are from what the call answered, `alloc(m)` makes the arrays of m units and `ptr` turns one into the call's argument.
    max_units None: a counting call with null arrays, then the fill; a number: the one call.  No room (m == 0) passes null
    pointers.  Returns the arrays, cut to the first min(m, count) units."""

    def run(m):
        arrays = alloc(m)
        rc = call(m, *[ptr(a) if m else None for a in arrays])
        if rc != 0:
            raise RuntimeError(f"{fn} failed: {rc}")
        return arrays

    if max_units is None:
        run(0)
        max_units = count()
    m = int(max_units)
    arrays = run(m)
    k = min(m, int(count()))
    return [a[:k] for a in arrays]


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def _host_input(data):
    """bytes / a numpy array as a contiguous uint8 array, and its pointer (None when it is empty)"""
    import numpy as np

    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    return buf, _np_ptr(buf)


def _device_input(in_buf, length):
    """(device, length, base pointer) of a uint8 device tensor holding `length` bytes; the base of no bytes is None"""
    import torch

    dev = _check_tensors(((in_buf, torch.uint8),))
    length = int(length)
    if length < 0 or length > in_buf.numel():
        raise ValueError(f"length {length} outside the buffer of {in_buf.numel()} bytes")
    return dev, length, (_dp(in_buf) if length else None)


def _plan_arrays(m):
    """a plan's four arrays in host memory, zeroed: in_off, in_len, out_off, out_cap"""
    import numpy as np

    return np.zeros(m, np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint64), np.zeros(m, np.uint32)


def _plan_tensors(m, dev):
    """a plan's four arrays in device memory: in_off, in_len, out_off, out_cap"""
    import torch

    return tuple(torch.empty(m, dtype=dt, device=dev) for dt in (torch.int64, torch.int32, torch.int64, torch.int32))


def _record_array(dtype):
    """alloc of _plan_host for a plan of records: one zeroed numpy record array"""
    import numpy as np

    return lambda m: (np.zeros(m, dtype),)


def _record_rows(struct, make="empty"):
    """alloc of _plan_device for a plan of records: one uint8 tensor of shape (m, sizeof(struct))"""

    def alloc(m, dev):
        import torch

        return (getattr(torch, make)((m, C.sizeof(struct)), dtype=torch.uint8, device=dev),)

    return alloc


def _plan_host(fn, raw_cls, wrap, count_field, data, max_units, alloc=_plan_arrays):
    """A chip_*_plan_host / chip_*_blocks_host call over bytes / a uint8 numpy array: count (max_units None), then fill.  Returns
    the arrays of `alloc` and the summary."""
    buf, base = _host_input(data)
    raw, call = raw_cls(), getattr(lib(), fn)
    arrays = _count_then_fill(fn, lambda m, *out: call(base, buf.size, m, *out, C.byref(raw)), lambda: getattr(raw, count_field), alloc,
                              _np_ptr, max_units)
    return (*arrays, wrap(raw))


def _plan_device(fn, raw_cls, wrap, count_field, in_buf, length, stream, max_units, alloc=_plan_tensors):
    """A chip_*_plan / chip_*_blocks call over a uint8 device tensor: count (max_units None), then fill.  Returns the tensors of
    `alloc` and the summary."""
    import torch

    dev, length, base = _device_input(in_buf, length)
    raw, sp, call = raw_cls(), _stream_ptr(stream), getattr(lib(), fn)
    with torch.cuda.device(dev):
        arrays = _count_then_fill(fn, lambda m, *out: call(base, length, m, *out, C.byref(raw), sp), lambda: getattr(raw, count_field),
                                  lambda m: alloc(m, dev), _dp, max_units)
    return (*arrays, wrap(raw))


def _whole_plan(plan, ok, refusal, in_buf, length, stream):
    """plan(in_buf, length) of a whole file: its five results, or ValueError(`refusal` and the summary) when the status is not `ok`."""
    planned = plan(in_buf, length, stream=stream)
    if planned[4].status != ok:
        raise ValueError(f"{refusal}: {planned[4]!r}")
    return planned


def _decode_planned(fmt, noun, in_buf, in_off, in_len, out_off, out_cap, total, stream):
    """decode_batch of a planned batch into a new tensor of max(total, 4) bytes, trimmed to `total`.  RuntimeError names the first
    `noun` (a unit of the plan) that did not end Finished with out_len == out_cap."""
    import torch

    out = torch.empty(max(total, 4), dtype=torch.uint8, device=in_buf.device)
    if in_off.numel():
        out_len, _, status = decode_batch(fmt, in_buf, in_off, in_len, out, out_off, out_cap, stream=stream)
        bad = ((status != int(DecodeStatus.Finished)) | (out_len != out_cap)).nonzero()
        if bad.numel():
            i = int(bad[0])
            raise RuntimeError(f"{noun} {i} did not decode: status {int(status[i])}, {int(out_len[i])} of {int(out_cap[i])} bytes")
    return out[:total]


def _plan_read(what, plan, ok, refusal, fmt, in_buf, length, ranges, stream):
    """What bgzf_read, zstd_frames_read and gzip_members_read do: the whole file's plan, read_ranges over it, _read_checked."""
    in_off, in_len, out_off, out_cap, _ = _whole_plan(plan, ok, refusal, in_buf, length, stream)
    lo, ln = _ranges_to_device(ranges, in_buf.device)
    out, dst_off, status, rs = read_ranges(fmt, in_buf, in_off, in_len, out_off, out_cap, lo, ln, stream=stream)
    return _read_checked(what, out, status, rs), dst_off


def bgzf_plan_host(data, max_blocks=None):
    """chip_bgzf_plan_host over bytes / a uint8 numpy array in host memory: (in_off u64, in_len u32, out_off u64, out_cap u32,
    summary) of the first min(n_blocks, max_blocks) blocks (None = all of them: one call to count, one to fill)."""
    return _plan_host("chip_bgzf_plan_host", _BgzfSummary, BgzfSummary, "n_blocks", data, max_blocks)


def bgzf_plan(in_buf, length, stream=None, max_blocks=None):
    """chip_bgzf_plan over a uint8 device tensor holding `length` bytes of BGZF (4-byte aligned, padded to a multiple of 4):
    returns (in_off int64, in_len int32, out_off int64, out_cap int32, summary) -- device tensors of the first
    min(n_blocks, max_blocks) blocks, ready for decode_batch(ZlibMode.Gzip, ..).  Synchronous on `stream`.  max_blocks None: all
    of them (one call to count, one to fill)."""
    return _plan_device("chip_bgzf_plan", _BgzfSummary, BgzfSummary, "n_blocks", in_buf, length, stream, max_blocks)


def bgzf_decode(in_buf, length, stream=None):
    """Decode a whole BGZF buffer on the device: plan, allocate total_out bytes, decode_batch(ZlibMode.Gzip).  Raises ValueError
    when the file is no whole BGZF file (the summary says where) and RuntimeError with the first bad block's index and status
    when a block does not decode to its ISIZE.  Returns the uint8 output tensor.  Waits for the decode."""
    in_off, in_len, out_off, out_cap, summ = _whole_plan(bgzf_plan, BgzfStatus.Ok, "not a whole BGZF file", in_buf, length, stream)
    return _decode_planned(ZlibMode.Gzip, "BGZF block", in_buf, in_off, in_len, out_off, out_cap, summ.total_out, stream)


# ---- zstd frames: from a file to a batch (include/compu_hip.h, "zstd frames") -------------------

ZPLAN_UNSIZED = 0xFFFFFFFF  # CHIP_ZPLAN_UNSIZED: out_cap of a frame without Frame_Content_Size (-1 in an int32 tensor)


class ZstdPlanStatus(enum.IntEnum):
    Ok = 0
    Truncated = 1
    BadHeader = 2
    TooLarge = 3


class ZstdPlanSummary(_Summary):
    """chip_zstd_plan_summary: n_frames, n_skippable, n_unsized and total_out of the whole walk, in_used where it stopped (the
    start of the frame it stopped at), status why."""

    __slots__ = FIELDS = _fields(_ZstdPlanSummary)
    ENUMS = {"status": ZstdPlanStatus}


def zstd_plan_host(data, max_frames=None):
    """chip_zstd_plan_host over bytes / a uint8 numpy array in host memory: (in_off u64, in_len u32, out_off u64, out_cap u32,
    summary) of the first min(n_frames, max_frames) frames (None = all of them: one call to count, one to fill)."""
    return _plan_host("chip_zstd_plan_host", _ZstdPlanSummary, ZstdPlanSummary, "n_frames", data, max_frames)


def zstd_plan(in_buf, length, stream=None, max_frames=None):
    """chip_zstd_plan over a uint8 device tensor holding `length` bytes of zstd frames (4-byte aligned, padded to a multiple of
    4): returns (in_off int64, in_len int32, out_off int64, out_cap int32, summary) -- device tensors of the first
    min(n_frames, max_frames) frames; with summary.n_unsized == 0 they are ready for decode_batch(FMT_ZSTD, ..).  Synchronous
    on `stream`.  max_frames None: all of them (one call to count, one to fill)."""
    return _plan_device("chip_zstd_plan", _ZstdPlanSummary, ZstdPlanSummary, "n_frames", in_buf, length, stream, max_frames)


ZBLOCKS_UNSIZED = 0xFFFFFFFFFFFFFFFF  # CHIP_ZBLOCKS_UNSIZED: content_size of a frame without Frame_Content_Size
ZBLOCK_LAST, ZBLOCK_MALFORMED = 1, 2  # chip_zstd_block.flags
ZSRC_HUF, ZSRC_LL, ZSRC_OF, ZSRC_ML = 0, 1, 2, 3  # the columns of chip_zstd_block.src


def zstd_block_dtype():
    """chip_zstd_block as a numpy record: offset, size, lit_regen, lit_comp, n_seq, type, flags, lit_type, mode[3], src[4]."""
    import numpy as np

    dt = np.dtype(_ZstdBlock)
    assert dt.itemsize == 48
    return dt


class ZstdBlocksSummary(_Summary):
    """chip_zstd_blocks_summary: n_blocks the walk counted, in_used (the frame's end, 0 when the walk stopped early), content_size
    (ZBLOCKS_UNSIZED without Frame_Content_Size), window_size, status why the walk stopped, the frame header descriptor and the
    frame header's length."""

    __slots__ = FIELDS = _fields(_ZstdBlocksSummary)
    ENUMS, FORMATS = {"status": ZstdPlanStatus}, {"descriptor": "#x"}


def zstd_blocks_host(data, max_blocks=None):
    """chip_zstd_blocks_host over bytes / a uint8 numpy array in host memory: (blocks, summary) of the FIRST frame -- blocks a
    numpy record array (zstd_block_dtype) of the first min(n_blocks, max_blocks) blocks (None = all of them: one call to count,
    one to fill).  Read from headers alone; nothing is decoded."""
    return _plan_host("chip_zstd_blocks_host", _ZstdBlocksSummary, ZstdBlocksSummary, "n_blocks", data, max_blocks, _record_array(zstd_block_dtype()))


def zstd_blocks(in_buf, length, stream=None, max_blocks=None):
    """chip_zstd_blocks over a uint8 device tensor holding `length` bytes that begin with a zstd frame (4-byte aligned, padded to
    a multiple of 4): (blocks, summary), blocks a uint8 device tensor of shape (k, 48) holding the chip_zstd_block records of the
    first k = min(n_blocks, max_blocks) blocks (`.cpu().numpy().view(zstd_block_dtype())` reads them).  Synchronous on `stream`.
    max_blocks None: all of them (one call to count, one to fill)."""
    return _plan_device("chip_zstd_blocks", _ZstdBlocksSummary, ZstdBlocksSummary, "n_blocks", in_buf, length, stream, max_blocks,
                        _record_rows(_ZstdBlock))


ZPAR_SERIAL, ZPAR_PARALLEL, ZPAR_REFUSED = 0, 1, 2  # chip_zstd_parallel_summary.path
ZPAR_NO_CHECKSUM = 1  # CHIP_ZPAR_NO_CHECKSUM
ZPAR_ROUNDS_MAX = 40


class ZstdParallelSummary(_Summary):
    """chip_zstd_parallel_summary: n_blocks and n_sequences of the frame (parallel path), out_len, in_used, total_out (the size to
    come back with on NeedOutput), status, path (ZPAR_*), rounds of the jump pass, check."""

    __slots__ = FIELDS = _fields(_ZstdParallelSummary)

    def as_tuple(self):
        """everything but `rounds`, which may differ from call to call"""
        return tuple(getattr(self, name) for name in self.FIELDS if name != "rounds")


def zstd_parallel(in_buf, length, out_buf=None, window_log_max=0, checksum=True, stream=None):
    """chip_zstd_parallel over a uint8 device tensor holding `length` bytes that begin with ONE zstd frame (4-byte aligned, padded
    to a multiple of 4): (out, summary).  With `out_buf` (a uint8 device tensor) the content goes there and `out` is its first
    out_len bytes.  Without, the call is made with no room first, then with a new tensor of total_out bytes; a frame that takes the
    serial path states no size that way (the batch decode's NeedOutput carries none), so it is sized by decode_batch_sizes as one
    unit and decoded with that room -- a frame that is refused, or in error, comes back as the empty tensor and its summary.
    checksum=False waives the comparison of Content_Checksum on the parallel path.  Synchronous on `stream`."""
    import torch

    dev = _check_tensors(((in_buf, torch.uint8),) + (((out_buf, torch.uint8),) if out_buf is not None else ()))
    length = int(length)
    if length < 0 or length > in_buf.numel():
        raise ValueError(f"length {length} outside the buffer of {in_buf.numel()} bytes")
    raw = _ZstdParallelSummary()
    flags = 0 if checksum else ZPAR_NO_CHECKSUM
    base, sp = (_dp(in_buf) if length else None), _stream_ptr(stream)

    def call(out):
        cap = out.numel() if out is not None else 0
        rc = lib().chip_zstd_parallel(base, length, _dp(out) if cap else None, cap, int(window_log_max), flags, C.byref(raw), sp)
        if rc != 0:
            raise RuntimeError(f"chip_zstd_parallel failed: {rc}")

    with torch.cuda.device(dev):
        if out_buf is None:
            call(None)
            need = int(raw.total_out) if raw.status == int(DecodeStatus.NeedOutput) else 0
            if raw.status == int(DecodeStatus.NeedOutput) and raw.path == ZPAR_SERIAL and length <= 1 << 28:
                one = lambda v, dt: torch.tensor([v], dtype=torch.int64, device=dev).to(dt)  # noqa: E731
                size, _, st = decode_batch_sizes(FMT_ZSTD, in_buf, one(0, torch.int64), one(length, torch.int32), stream=stream)
                need = int(size[0]) if int(st[0]) == int(DecodeStatus.Finished) and int(size[0]) <= 0xFFFFFFFF else 0
            out_buf = torch.empty(need, dtype=torch.uint8, device=dev)
            if need:
                call(out_buf)
        else:
            call(out_buf)
    return out_buf[:int(raw.out_len)], ZstdParallelSummary(raw)


ZCUR_HEADER, ZCUR_BLOCKS, ZCUR_CHECKSUM, ZCUR_DONE, ZCUR_ERROR = range(5)  # chip_zstd_cursor::phase
ZCUR_SLOT_BYTES = 131088  # CHIP_ZCUR_SLOT_BYTES
ZCUR_CARRY_BYTES = 4 * ZCUR_SLOT_BYTES  # CHIP_ZCUR_CARRY_BYTES


class ZstdCursor:
    """chip_zstd_cursor and its device state (the four carry slots and the window ring): where a slabbed decode of ONE zstd frame
    stands.  A fresh one is the beginning of a frame; its state is allocated by zstd_parallel_next once the frame header has said
    how large the window is (need_state).  The scalar fields read and write the C struct `raw`; copy() is an independent cursor at
    the same place."""

    FIELDS = ("in_total", "out_total", "window_size", "content_size", "hist", "ring", "phase", "descriptor", "waived", "error")

    def __init__(self, device=None):
        import torch

        self.raw = _ZstdCursor()
        self.device = torch.device(device if device is not None else "cuda")
        self.state = torch.zeros(ZCUR_CARRY_BYTES, dtype=torch.uint8, device=self.device)

    def __getattr__(self, name):
        if name in ZstdCursor.FIELDS:
            return int(getattr(self.raw, name))
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in ZstdCursor.FIELDS:
            setattr(self.raw, name, int(value))
        else:
            object.__setattr__(self, name, value)

    def copy(self):
        other = ZstdCursor(self.device)
        C.memmove(C.byref(other.raw), C.byref(self.raw), C.sizeof(_ZstdCursor))
        other.state = self.state.clone()
        return other

    def __repr__(self):
        return "ZstdCursor(" + ", ".join(f"{name}={getattr(self, name)}" for name in self.FIELDS) + f", rep={list(self.raw.rep)})"


class ZstdNextSummary(_Record):
    """chip_zstd_next_summary: in_used bytes of the slab lie in front of the new cursor, out_len bytes were delivered, need_out is the
    decoded size of the block that did not fit, need_state the state bytes to come back with, n_blocks / n_sequences / rounds
    describe the blocks taken, status says why the call stopped (a DecodeStatus value or a negative error)."""

    FIELDS = _fields(_ZstdNextSummary)


def zstd_parallel_next(cursor, in_buf, out_buf, window_log_max=0, checksum=True, stream=None, grow_state=True):
    """chip_zstd_parallel_next: decode the next part of the frame `cursor` stands in.  in_buf (uint8 device tensor, any alignment)
    holds the frame from byte cursor.in_total on, out_buf the room.  The cursor moves; the bytes are out_buf[:summary.out_len] and
    the next slab begins summary.in_used bytes further.  grow_state: a call that stops behind the frame header because the state is
    too small for the window (need_state) gets a state of that size and is made again over the rest of the slab, its in_used added.
    Synchronous on `stream`."""
    import torch

    dev = _check_tensors([(in_buf, torch.uint8), (out_buf, torch.uint8), (cursor.state, torch.uint8)])
    flags = 0 if checksum else ZPAR_NO_CHECKSUM
    done = 0
    while True:
        raw = _ZstdNextSummary()
        part = in_buf[done:]
        with torch.cuda.device(dev):
            rc = lib().chip_zstd_parallel_next(C.byref(cursor.raw), _dp(cursor.state), cursor.state.numel(), _dp(part) if part.numel() else None, part.numel(),
                                               _dp(out_buf) if out_buf.numel() else None, out_buf.numel(), int(window_log_max), flags, C.byref(raw),
                                               _stream_ptr(stream))
        if rc != 0:
            raise RuntimeError(f"chip_zstd_parallel_next failed: {rc}")
        summ = ZstdNextSummary(raw)
        summ.in_used += done
        if not (grow_state and summ.need_state > cursor.state.numel()):
            return summ
        done = summ.in_used
        state = torch.zeros(summ.need_state, dtype=torch.uint8, device=dev)
        state[:ZCUR_CARRY_BYTES] = cursor.state[:ZCUR_CARRY_BYTES]
        cursor.state = state


class ZstdSlabSummary(_Summary):
    """chip_zstd_slab_summary: the whole blocks in front of where the walk from a block boundary stopped, their bytes, why it stopped
    (ZstdPlanStatus; Truncated is a cut block, no error) and whether the frame's last block is among them."""

    __slots__ = FIELDS = _fields(_ZstdSlabSummary)
    ENUMS = {"status": ZstdPlanStatus}


def zstd_slab_blocks_host(data, block_max=131072):
    """chip_zstd_slab_blocks_host over bytes that begin at a block boundary of a frame whose Block_Maximum_Size is block_max:
    (blocks, summary), the records as zstd_blocks_host's with slab-relative offsets and sources."""
    buf, base = _host_input(data)
    raw, call = _ZstdSlabSummary(), lib().chip_zstd_slab_blocks_host
    blocks, = _count_then_fill("chip_zstd_slab_blocks_host", lambda m, out: call(base, buf.size, int(block_max), m, out, C.byref(raw)),
                               lambda: raw.n_blocks, _record_array(zstd_block_dtype()), _np_ptr, None)
    return blocks, ZstdSlabSummary(raw)


def zstd_cursor_header_host(data, window_log_max=0, checksum=True):
    """chip_zstd_cursor_header_host on the first bytes of a frame in host memory: (status, raw cursor, header_bytes, need_state).
    status is DecodeStatus.Finished with the cursor at the first block, NeedInput for a cut header, or the negative code."""
    import numpy as np

    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cur, hb, need = _ZstdCursor(), C.c_uint32(0), C.c_uint64(0)
    rc = lib().chip_zstd_cursor_header_host(C.byref(cur), buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, int(window_log_max),
                                            0 if checksum else ZPAR_NO_CHECKSUM, C.byref(hb), C.byref(need))
    return rc, cur, int(hb.value), int(need.value)


class Xxh64:
    """A running XXH64 (seed 0) over chip_xxh64_state: update(bytes), digest(), copy()."""

    def __init__(self):
        self.raw = _Xxh64State()

    def update(self, data):
        import numpy as np

        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        rc = lib().chip_xxh64_update_host(C.byref(self.raw), buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size)
        if rc != 0:
            raise RuntimeError(f"chip_xxh64_update_host failed: {rc}")
        return self

    def digest(self):
        return int(lib().chip_xxh64_digest_host(C.byref(self.raw)))

    def copy(self):
        other = Xxh64()
        C.memmove(C.byref(other.raw), C.byref(self.raw), C.sizeof(_Xxh64State))
        return other


class _Slabs:
    """What _slab_stream asks of a format.  The format's own: slab_max and room_max (the limits of one call), eof_text, spare and
    alloc_in (the input tensor), new_cursor, step, room_now, grow_room and after_finished.  Shared: the two device buffers and the
    copies to and from them -- new_cursor, upload, room, step and download are all that touches the device."""

    spare = 0  # bytes the input tensor has behind the slab

    def __init__(self, device):
        import torch

        self.dev = torch.device(device if device is not None else "cuda")
        self.d_in = self.d_out = None

    def upload(self, pending, n, slab):
        """pending[:n] in device memory; the tensor is kept from call to call and replaced when it is too small"""
        import numpy as np
        import torch

        if self.d_in is None or self.d_in.numel() < n + self.spare:
            self.d_in = self.alloc_in(n, slab)
        if n:  # straight from the pending bytes (the copy from pageable memory has ended when copy_ returns)
            self.d_in[:n].copy_(torch.from_numpy(np.frombuffer(pending, dtype=np.uint8, count=n)))
        return self.d_in[:n]

    def room(self, k):
        import torch

        if self.d_out is None or self.d_out.numel() < k:
            self.d_out = torch.empty(k, dtype=torch.uint8, device=self.dev)
        return self.d_out[:k]

    def download(self, out, k):
        return out[:k].cpu().numpy().tobytes()

    def room_now(self, cur, pending, room):
        return room


def _slab_stream(slabs, source, sink, slab_bytes, out_bytes):
    """The loop of zstd_parallel_stream and inflate_parallel_stream over `slabs`, a _Slabs: `source` (bytes-like, or a binary file
    object) is read into `pending`, a slab of it uploaded, the cursor stepped, the call's bytes downloaded and written to `sink`
    (None: collected), what the call used cut from `pending`.  Then: a finished unit ends the loop unless slabs.after_finished begins
    another; an error raises DecodeError; a call that used and gave nothing grows the room (NeedOutput), doubles the slab while the
    source has more, and is EOFError at its end.  Returns the bytes, or with a sink their number."""
    read = source.read if hasattr(source, "read") else None
    view, taken = (None, 0) if read else (memoryview(source).cast("B"), 0)
    pending, eof = bytearray(), False
    slab, room = max(int(slab_bytes), 1), max(int(out_bytes), 1)
    parts, written = [], 0

    def fill(want):  # (a short read is not the end: an empty one is)
        nonlocal eof, taken
        while not eof and len(pending) < want:
            if read:
                piece = read(want - len(pending))
            else:
                piece = view[taken : taken + want - len(pending)]
                taken += len(piece)
            if not len(piece):
                eof = True
            pending.extend(piece)

    cur = slabs.new_cursor()
    while True:
        slab, room = min(slab, slabs.slab_max), min(room, slabs.room_max)
        fill(slab)
        n = min(len(pending), slab)  # (below the slab only where the source has ended: the buffers are as large as what there is)
        out = slabs.room(slabs.room_now(cur, pending, room))
        s = slabs.step(cur, slabs.upload(pending, n, slab), out)
        if s.out_len:
            got = slabs.download(out, s.out_len)
            written += len(got)
            if sink is None:
                parts.append(got)
            else:
                sink.write(got)
        del pending[: s.in_used]
        if s.status == int(DecodeStatus.Finished):
            cur = slabs.after_finished(cur, pending, fill)
            if cur is None:
                break
            continue
        if s.status not in (int(DecodeStatus.NeedInput), int(DecodeStatus.NeedOutput)):
            raise DecodeError(s.status)
        if s.in_used == 0 and s.out_len == 0:
            if s.status == int(DecodeStatus.NeedOutput):
                room = slabs.grow_room(room, s.need_out)
            elif n < len(pending) or not eof:
                if slab >= slabs.slab_max:
                    raise DecodeError(-5)  # a block beyond a call's slab
                slab *= 2
            else:
                raise EOFError(slabs.eof_text)
    return b"".join(parts) if sink is None else written


class _ZstdSlabs(_Slabs):
    """zstd_parallel_stream's side of _slab_stream"""

    slab_max, room_max = 1 << 31, (1 << 31) - 1
    eof_text = "the source ends inside the frame"

    def __init__(self, device, frames, checksum, window_log_max):
        super().__init__(device)
        self.frames, self.checksum, self.window_log_max = frames, checksum, window_log_max

    def new_cursor(self):
        return ZstdCursor(self.dev)

    def alloc_in(self, n, slab):  # uninitialised, exactly what there is
        import torch

        return torch.empty(max(n, 1), dtype=torch.uint8, device=self.dev)

    def step(self, cur, d_in, d_out):
        return zstd_parallel_next(cur, d_in, d_out, self.window_log_max, self.checksum)

    def room_now(self, cur, pending, room):
        left = cur.content_size - cur.out_total if cur.phase and cur.content_size != ZBLOCKS_UNSIZED else ZBLOCKS_UNSIZED
        if not cur.phase:  # a new frame: what its header says of its size, so that a small frame gets a small room
            rc, head, _, _ = zstd_cursor_header_host(pending[:18], 31)
            left = int(head.content_size) if rc == int(DecodeStatus.Finished) else ZBLOCKS_UNSIZED
        return min(room, max(left, 1)) if 0 <= left < ZBLOCKS_UNSIZED else room

    def grow_room(self, room, need_out):
        if need_out > (1 << 31) - 1:
            raise DecodeError(-5)
        return max(room, need_out)

    def after_finished(self, cur, pending, fill):
        """frames=True: a new cursor when a zstd magic follows, skippable frames stepped over; else None"""
        while self.frames:
            fill(8)
            magic = int.from_bytes(bytes(pending[:4]), "little") if len(pending) >= 4 else 0
            if magic & 0xFFFFFFF0 != 0x184D2A50:
                return self.new_cursor() if magic == 0xFD2FB528 else None
            if len(pending) < 8:  # a skippable frame: 8 bytes and what they announce
                raise EOFError("the source ends inside a skippable frame")
            size = 8 + int.from_bytes(bytes(pending[4:8]), "little")
            fill(size)
            if len(pending) < size:
                raise EOFError("the source ends inside a skippable frame")
            del pending[:size]
        return None


def zstd_parallel_stream(source, sink=None, slab_bytes=64 << 20, out_bytes=256 << 20, frames=False, checksum=True, window_log_max=0, device=None):
    """One zstd frame of ANY length through zstd_parallel_next: `source` (bytes-like, or a binary file object) is uploaded slab after
    slab, every call's bytes are downloaded and written to `sink` (a binary file object; None: they are returned as bytes).  The
    slab doubles when a call finds no whole block in it, the room goes to need_out when the next block does not fit, the state is
    allocated from need_state.  frames=True: behind a finished frame the loop goes on while a zstd or skippable magic follows, as
    `zstd -d` does, and steps over skippable frames itself.  Raises DecodeError(code) on an error in the frame and EOFError when
    the source ends inside it.  Returns the bytes, or with a sink the number of bytes written."""
    return _slab_stream(_ZstdSlabs(device, frames, checksum, window_log_max), source, sink, slab_bytes, out_bytes)


def layout_units(out_size, stream=None):
    """chip_layout_units over the int64 device tensor a size pass filled (read as u64): returns (out_off int64, out_cap int32,
    total, n_over) -- out_off the exclusive sum of the sizes, out_cap the sizes clipped to 0xFFFFFFFF, n_over how many were
    clipped.  Synchronous on `stream`."""
    import torch

    dev = _check_tensors(((out_size, torch.int64),))
    n = out_size.numel()
    out_off, out_cap = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    total, n_over = C.c_uint64(0), C.c_uint64(0)
    q = lambda t: _dp(t) if n else None  # noqa: E731
    with torch.cuda.device(dev):
        rc = lib().chip_layout_units(n, q(out_size), q(out_off), q(out_cap), C.byref(total), C.byref(n_over), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_layout_units failed: {rc}")
    return out_off, out_cap, int(total.value), int(n_over.value)


def zstd_frames_decode(in_buf, length, stream=None):
    """Decode a whole buffer of zstd frames on the device, one unit per frame: plan; when frames lack Frame_Content_Size, the
    size pass over the plan's units and layout_units; allocate; decode_batch(FMT_ZSTD).  Raises ValueError when the buffer is
    no whole series of frames (the summary says where) or a frame decodes to more than a unit can hold, and RuntimeError with
    the first bad frame's index and status when a frame does not decode to its size.  Returns (the uint8 output tensor,
    (in_off, in_len, out_off, out_cap) as used for the decode, summary).  Waits for the decode."""
    in_off, in_len, out_off, out_cap, summ = _whole_plan(zstd_plan, ZstdPlanStatus.Ok, "not a whole series of zstd frames", in_buf, length, stream)
    total = summ.total_out
    if summ.n_unsized:
        out_size, _, _ = decode_batch_sizes(FMT_ZSTD, in_buf, in_off, in_len, stream=stream)
        out_off, out_cap, total, n_over = layout_units(out_size, stream=stream)
        if n_over:
            raise ValueError(f"{n_over} frames decode to more than 4 GiB - 1: {summ!r}")
    out = _decode_planned(FMT_ZSTD, "zstd frame", in_buf, in_off, in_len, out_off, out_cap, total, stream)
    return out, (in_off, in_len, out_off, out_cap), summ


# ---- gzip members: from a file to a batch (include/compu_hip.h, "gzip members") -----------------

GZPLAN_WINDOW = (1 << 29) - 64  # CHIP_GZPLAN_WINDOW: input bytes a member may take


class GzipPlanStatus(enum.IntEnum):
    Ok = 0
    Truncated = 1
    BadHeader = 2
    TooLarge = 3
    BadMember = 4


class GzipPlanSummary(_Summary):
    """chip_gzip_plan_summary: n_members and total_out of the whole walk, in_used where it stopped (the start of the member it
    stopped at), status why, member_status the size pass's status of that member when status is BadMember (else 0)."""

    __slots__ = FIELDS = _fields(_GzipPlanSummary)
    ENUMS = {"status": GzipPlanStatus}


def gzip_plan(in_buf, length, stream=None, max_members=None):
    """chip_gzip_plan over a uint8 device tensor holding `length` bytes of gzip members (4-byte aligned, padded to a multiple of
    4): returns (in_off int64, in_len int32, out_off int64, out_cap int32, summary) -- device tensors of the first
    min(n_members, max_members) members, ready for decode_batch(ZlibMode.Gzip, ..) and read_ranges(ZlibMode.Gzip, ..).
    Synchronous on `stream`.  max_members None: all of them (one call to count, one to fill)."""
    return _plan_device("chip_gzip_plan", _GzipPlanSummary, GzipPlanSummary, "n_members", in_buf, length, stream, max_members)


def gzip_members_decode(in_buf, length, stream=None):
    """Decode a whole buffer of gzip members on the device, one unit per member: plan, allocate total_out bytes,
    decode_batch(ZlibMode.Gzip).  Raises ValueError when the buffer is no whole series of members (the summary says where) and
    RuntimeError with the first bad member's index and status when a member does not decode to its size (a wrong CRC-32: the
    plan does not see it).  Returns (the uint8 output tensor, (in_off, in_len, out_off, out_cap), summary).  Waits for the
    decode."""
    in_off, in_len, out_off, out_cap, summ = _whole_plan(gzip_plan, GzipPlanStatus.Ok, "not a whole series of gzip members", in_buf, length, stream)
    out = _decode_planned(ZlibMode.Gzip, "gzip member", in_buf, in_off, in_len, out_off, out_cap, summ.total_out, stream)
    return out, (in_off, in_len, out_off, out_cap), summ


# ---- writing files: from a batch to a file (include/compu_hip.h, "writing files") ---------------

W_SEEK_TABLE = 1  # CHIP_W_SEEK_TABLE: the seek table of zstd's seekable format behind the last frame (FMT_ZSTD only)


class FileStatus(enum.IntEnum):
    Ok = 0
    NeedOutput = 1


class FileSummary(_Summary):
    """chip_file_summary: n_units encoded, out_len the file's length (the exact size needed on NeedOutput), table_off where the
    seek table starts (out_len without one), status."""

    __slots__ = FIELDS = _fields(_FileSummary)
    ENUMS = {"status": FileStatus}


def pack_units(src, src_off, src_len, dst=None, stream=None):
    """chip_pack_units over device tensors: the ranges src[src_off[i] .. + src_len[i]) (src uint8, src_off int64 read as u64,
    src_len int32 read as u32) end to end.  dst None: a tensor of exactly `total` bytes is allocated (one call to size it, one to
    fill).  With a dst that is too small nothing is written; compare the returned total with dst.numel().  Returns (dst, dst_off
    int64, total).  Synchronous on `stream`."""
    import torch

    pairs = [(src, torch.uint8), (src_off, torch.int64), (src_len, torch.int32)] + ([(dst, torch.uint8)] if dst is not None else [])
    dev = _check_tensors(pairs)
    n = src_len.numel()
    if src_off.numel() != n:
        raise ValueError(f"{src_off.numel()} offsets for {n} lengths")
    dst_off = torch.empty(n, dtype=torch.int64, device=dev)
    total = C.c_uint64(0)
    q = lambda t: _dp(t) if t is not None and t.numel() else None  # noqa: E731
    sp = _stream_ptr(stream)

    def call(d):
        rc = lib().chip_pack_units(n, q(src) if n else None, q(src_off), q(src_len), q(d), d.numel() if d is not None else 0, q(dst_off),
                                   C.byref(total), sp)
        if rc != 0:
            raise RuntimeError(f"chip_pack_units failed: {rc}")

    with torch.cuda.device(dev):
        call(dst)
        if dst is None:
            dst = torch.empty(int(total.value), dtype=torch.uint8, device=dev)
            if total.value:
                call(dst)
    return dst, dst_off, int(total.value)


def encode_file_bound(fmt, length, unit_bytes=0, flags=0):
    """chip_encode_file_bound: the output size that is always enough; 0 for arguments encode_file refuses."""
    return int(lib().chip_encode_file_bound(int(fmt), int(unit_bytes), int(flags), int(length)))


def encode_file(fmt, level, in_buf, length, unit_bytes=0, flags=0, stream=None, out=None):
    """chip_encode_file over a uint8 device tensor holding `length` bytes (4-byte aligned, padded to a multiple of 4): cut into
    units of unit_bytes (0: 65280 for FMT_BGZF, 262144 for ZlibMode.Gzip and FMT_ZSTD), encoded, packed, trailer appended -- a
    BGZF file, a file of gzip members, a file of zstd frames (flags W_SEEK_TABLE: with the seekable format's seek table).
    FMT_LZ4: ONE LZ4 frame with a block per unit (unit_bytes 0 = 65536, or 65536, 262144, 1048576, 4194304; levels -1 .. 12; flags
    W_LZ4_CONTENT_CHECKSUM, W_LZ4_BLOCK_CHECKSUM), the file lz4_parallel reads with a wave per block.
    out None: a tensor of encode_file_bound bytes is allocated and the result is a view of its first out_len bytes.  With an
    `out` that is too small the summary says NeedOutput with the exact out_len and nothing is written.  Returns (the uint8
    output tensor trimmed to out_len -- None on NeedOutput --, summary).  Synchronous on `stream`."""
    import torch

    dev = _check_tensors(((in_buf, torch.uint8),) + (((out, torch.uint8),) if out is not None else ()))
    length = int(length)
    if length < 0 or length > in_buf.numel():
        raise ValueError(f"length {length} outside the buffer of {in_buf.numel()} bytes")
    if out is None:
        bound = encode_file_bound(fmt, length, unit_bytes, flags)
        if bound == 0:
            raise ValueError(f"encode_file refuses format {int(fmt)}, unit_bytes {unit_bytes}, flags {flags}, length {length}")
        out = torch.empty(bound, dtype=torch.uint8, device=dev)
    raw = _FileSummary()
    with torch.cuda.device(dev):
        rc = lib().chip_encode_file(int(fmt), int(level), int(unit_bytes), int(flags), _dp(in_buf) if length else None, length,
                                    _dp(out) if out.numel() else None, out.numel(), C.byref(raw), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_encode_file failed: {rc}")
    summ = FileSummary(raw)
    return (out[: summ.out_len] if summ.status == FileStatus.Ok else None), summ


def bgzf_write(in_buf, length, level=6, stream=None):
    """A whole BGZF file of the first `length` bytes of in_buf: encode_file(FMT_BGZF, level, ..) with htslib's block payload."""
    return encode_file(FMT_BGZF, level, in_buf, length, stream=stream)


# ---- reading ranges: random access on a plan (include/compu_hip.h, "reading ranges") ------------


class ReadStatus(enum.IntEnum):
    Ok = 0
    NeedOutput = 1
    BadLayout = 2


class RangeStatus(enum.IntEnum):
    Ok = 0
    Outside = 1
    BadUnit = 2


class SelectSummary(_Summary):
    """chip_select_summary: n_sel units selected, scratch_bytes their decoded size, out_len the ranges' bytes, n_outside ranges
    outside the content, status (BadLayout: bad_index is the first unit that does not follow its predecessor)."""

    __slots__ = FIELDS = _fields(_SelectSummary)
    ENUMS = {"status": ReadStatus}


class ReadSummary(_Summary):
    """chip_read_summary: n_units decoded, out_len bytes of ranges (the exact size needed on NeedOutput), n_outside, n_bad
    selected units that did not decode to their size with first_bad the lowest one's index and bad_status its status, status
    (BadLayout: bad_index says where)."""

    __slots__ = FIELDS = _fields(_ReadSummary)
    ENUMS = {"status": ReadStatus}


def select_units_host(in_off, in_len, out_off, out_cap, range_lo, range_len, max_sel=None):
    """chip_select_units_host over numpy arrays (or sequences) in host memory: the plan's four arrays and the ranges.  Returns
    (sel_unit u32, sel_in_off u64, sel_in_len u32, sel_out_off u64, sel_out_cap u32, src_off u64, dst_off u64, range_status i32,
    summary): the sub-batch of the first min(n_sel, max_sel) selected units (None = all of them: one call to count, one to
    fill) and the three per-range arrays.  On BadLayout every array is empty."""
    import numpy as np

    arr = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    in_off, in_len, out_off, out_cap = arr(in_off, np.uint64), arr(in_len, np.uint32), arr(out_off, np.uint64), arr(out_cap, np.uint32)
    range_lo, range_len = arr(range_lo, np.uint64), arr(range_len, np.uint32)
    n, m = int(out_cap.size), int(range_len.size)
    if not (in_off.size == in_len.size == out_off.size == n) or range_lo.size != m:
        raise ValueError("the plan's arrays, and the ranges' arrays, must have one length each")
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    raw = _SelectSummary()
    plan = (n, p(in_off), p(in_len), p(out_off), p(out_cap), m, p(range_lo), p(range_len))
    if max_sel is None:
        rc = lib().chip_select_units_host(*plan, 0, None, None, None, None, None, None, None, None, C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"chip_select_units_host failed: {rc}")
        max_sel = int(raw.n_sel)
    k = int(max_sel)
    sel_unit, sel_in_len, sel_out_cap = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    sel_in_off, sel_out_off = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
    src_off, dst_off, status = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.int32)
    rc = lib().chip_select_units_host(*plan, k, p(sel_unit), p(sel_in_off), p(sel_in_len), p(sel_out_off), p(sel_out_cap), p(src_off), p(dst_off),
                                      p(status), C.byref(raw))
    if rc != 0:
        raise RuntimeError(f"chip_select_units_host failed: {rc}")
    summ = SelectSummary(raw)
    k = min(k, summ.n_sel)
    if summ.status != ReadStatus.Ok:
        k = m = 0
    return sel_unit[:k], sel_in_off[:k], sel_in_len[:k], sel_out_off[:k], sel_out_cap[:k], src_off[:m], dst_off[:m], status[:m], summ


def _ranges_to_device(ranges, dev):
    """(range_lo int64, range_len int32) device tensors of a sequence of (lo, len) pairs or a pair of tensors."""
    import torch

    if isinstance(ranges, tuple) and len(ranges) == 2 and all(isinstance(t, torch.Tensor) for t in ranges):
        return ranges
    import numpy as np

    lo = np.array([r[0] for r in ranges], dtype=np.uint64).view(np.int64)
    ln = np.array([r[1] for r in ranges], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(lo).to(dev), torch.from_numpy(ln).to(dev)


def select_units(in_off, in_len, out_off, out_cap, range_lo, range_len, stream=None, max_sel=None):
    """chip_select_units on device tensors: the plan (in_off / out_off int64 read as u64, in_len / out_cap int32 read as u32)
    and the ranges (range_lo int64 read as u64, range_len int32 read as u32).  Returns what select_units_host returns, as device
    tensors (int64 / int32).  Synchronous on `stream`.  max_sel None: all selected units (one call to count, one to fill)."""
    import torch

    dev = _check_tensors(((in_off, torch.int64), (in_len, torch.int32), (out_off, torch.int64), (out_cap, torch.int32),
                          (range_lo, torch.int64), (range_len, torch.int32)))
    n, m = out_cap.numel(), range_len.numel()
    if not (in_off.numel() == in_len.numel() == out_off.numel() == n) or range_lo.numel() != m:
        raise ValueError("the plan's arrays, and the ranges' arrays, must have one length each")
    q = lambda t: _dp(t) if t.numel() else None  # noqa: E731
    raw = _SelectSummary()
    plan = (n, q(in_off), q(in_len), q(out_off), q(out_cap), m, q(range_lo), q(range_len))
    sp = _stream_ptr(stream)
    with torch.cuda.device(dev):
        if max_sel is None:
            rc = lib().chip_select_units(*plan, 0, None, None, None, None, None, None, None, None, C.byref(raw), sp)
            if rc != 0:
                raise RuntimeError(f"chip_select_units failed: {rc}")
            max_sel = int(raw.n_sel)
        k = int(max_sel)
        i64 = lambda c: torch.zeros(c, dtype=torch.int64, device=dev)  # noqa: E731
        i32 = lambda c: torch.zeros(c, dtype=torch.int32, device=dev)  # noqa: E731
        sel_unit, sel_in_off, sel_in_len, sel_out_off, sel_out_cap = i32(k), i64(k), i32(k), i64(k), i32(k)
        src_off, dst_off, status = i64(m), i64(m), i32(m)
        rc = lib().chip_select_units(*plan, k, q(sel_unit), q(sel_in_off), q(sel_in_len), q(sel_out_off), q(sel_out_cap), q(src_off), q(dst_off),
                                     q(status), C.byref(raw), sp)
    if rc != 0:
        raise RuntimeError(f"chip_select_units failed: {rc}")
    summ = SelectSummary(raw)
    k = min(k, summ.n_sel)
    if summ.status != ReadStatus.Ok:
        k = m = 0
    return sel_unit[:k], sel_in_off[:k], sel_in_len[:k], sel_out_off[:k], sel_out_cap[:k], src_off[:m], dst_off[:m], status[:m], summ


def _dp_or_none(t):
    return _dp(t) if t is not None and t.numel() else None


def _read_call(name, pairs, mismatch, m, dst, stream, call):
    """What read_ranges and inflate_index_read share.  `pairs` (and dst) go through _check_tensors, `mismatch` (the message, when the
    caller's arrays do not fit each other) raises ValueError; dst_off and the status of the m ranges are allocated; `call` makes
    the C call, given its last six arguments (dst, its size, dst_off, range_status, summary, stream), once, or with dst None twice:
    a first call with no room sizes dst.  Returns what the two return."""
    import torch

    dev = _check_tensors(pairs + ([(dst, torch.uint8)] if dst is not None else []))
    if mismatch:
        raise ValueError(mismatch)
    q = _dp_or_none
    dst_off, status = torch.zeros(m, dtype=torch.int64, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
    raw = _ReadSummary()
    sp = _stream_ptr(stream)

    def run(d):
        rc = call(q(d), d.numel() if d is not None else 0, q(dst_off), q(status), C.byref(raw), sp)
        if rc != 0:
            raise RuntimeError(f"{name} failed: {rc}")

    with torch.cuda.device(dev):
        run(dst)
        if dst is None and raw.status == int(ReadStatus.NeedOutput):
            dst = torch.empty(int(raw.out_len), dtype=torch.uint8, device=dev)
            run(dst)
        elif dst is None:
            dst = torch.empty(0, dtype=torch.uint8, device=dev)
    summ = ReadSummary(raw)
    return (dst[: summ.out_len] if summ.status == ReadStatus.Ok else None), dst_off, status, summ


def read_ranges(fmt, in_buf, in_off, in_len, out_off, out_cap, range_lo, range_len, dst=None, stream=None):
    """chip_read_ranges on device tensors: the bytes of every range (range_lo int64 read as u64, range_len int32 read as u32, in
    the coordinates of out_off) of the plan (in_off, in_len, out_off, out_cap) over in_buf, end to end in dst.  Only the units
    the ranges touch are decoded, each once.  dst None: a tensor of exactly out_len bytes is allocated (a first call with no
    room sizes it).  With a dst that is too small the summary says NeedOutput with the exact out_len and nothing is written.
    Returns (dst trimmed to out_len -- None on NeedOutput or BadLayout --, dst_off int64, range_status int32, summary).
    Synchronous on `stream`."""
    import torch

    pairs = [(in_buf, torch.uint8), (in_off, torch.int64), (in_len, torch.int32), (out_off, torch.int64), (out_cap, torch.int32),
             (range_lo, torch.int64), (range_len, torch.int32)]
    n, m = out_cap.numel(), range_len.numel()
    mismatch = not (in_off.numel() == in_len.numel() == out_off.numel() == n) or range_lo.numel() != m
    q = _dp_or_none
    return _read_call("chip_read_ranges", pairs, mismatch and "the plan's arrays, and the ranges' arrays, must have one length each", m, dst, stream,
                      lambda *out: lib().chip_read_ranges(int(fmt), n, q(in_buf) if n else None, q(in_off), q(in_len), q(out_off), q(out_cap), m,
                                                          q(range_lo), q(range_len), *out))


def _read_checked(what, out, status, summ):
    if summ.status != ReadStatus.Ok:
        raise ValueError(f"{what}: the plan's layout is broken: {summ!r}")
    if summ.n_outside:
        raise ValueError(f"{what}: {summ.n_outside} ranges lie outside the content: {summ!r}")
    if summ.n_bad:
        raise RuntimeError(f"{what}: unit {summ.first_bad} did not decode: status {summ.bad_status} ({summ.n_bad} bad units)")
    return out


def bgzf_read(in_buf, length, ranges, stream=None):
    """Bytes of a BGZF buffer on the device without decoding all of it: plan, then read_ranges(ZlibMode.Gzip).  `ranges` is a
    sequence of (lo, len) pairs in decoded coordinates, or a pair of device tensors (int64, int32).  Raises ValueError when
    the file is no whole BGZF file or a range lies outside its content, RuntimeError with the first bad block's index and
    status when a block a range touches does not decode to its ISIZE.  Returns (the uint8 tensor of the ranges end to end,
    dst_off int64).  Waits for the result."""
    return _plan_read("bgzf_read", bgzf_plan, BgzfStatus.Ok, "not a whole BGZF file", ZlibMode.Gzip, in_buf, length, ranges, stream)


def zstd_frames_read(in_buf, length, ranges, stream=None):
    """The same for a buffer of zstd frames (a seekable file): plan, then read_ranges(FMT_ZSTD).  Every frame must state its
    Frame_Content_Size (a frame without one breaks the layout: ValueError; decode such a file with zstd_frames_decode).
    Returns (the uint8 tensor of the ranges end to end, dst_off int64).  Waits for the result."""
    return _plan_read("zstd_frames_read", zstd_plan, ZstdPlanStatus.Ok, "not a whole series of zstd frames", FMT_ZSTD, in_buf, length, ranges, stream)


def gzip_members_read(in_buf, length, ranges, stream=None):
    """The same for a buffer of gzip members (WARC records, a file encode_file(ZlibMode.Gzip) wrote): gzip_plan, then
    read_ranges(ZlibMode.Gzip).  Returns (the uint8 tensor of the ranges end to end, dst_off int64).  Waits for the result."""
    return _plan_read("gzip_members_read", gzip_plan, GzipPlanStatus.Ok, "not a whole series of gzip members", ZlibMode.Gzip, in_buf, length, ranges,
                      stream)


# ---- seekable zstd files: the seek table as a plan (include/compu_hip.h, "seekable zstd files") ---


class ZstdSeekStatus(enum.IntEnum):
    Ok = 0
    NoTable = 1
    NeedTail = 2
    BadTable = 3
    TooLarge = 4
    BadLayout = 5


class ZstdSeekSummary(_Summary):
    """chip_zstd_seek_summary: n_frames entries in a table of table_bytes (on NeedTail: the tail to come back with), frames_bytes
    and total_out the sums of the compressed and content sizes, bad_index the lowest entry without a size on TooLarge, checksums
    whether the entries carry them, status."""

    __slots__ = FIELDS = _fields(_ZstdSeekSummary)
    ENUMS = {"status": ZstdSeekStatus}


def zstd_seek_plan_host(tail, file_len=None, max_frames=None):
    """chip_zstd_seek_plan_host over bytes / a uint8 numpy array holding the last bytes of a file of file_len bytes (None: the
    tail is the file): (in_off u64, in_len u32, out_off u64, out_cap u32, checksum u32, summary) of the first min(n_frames,
    max_frames) entries (None = all of them: one call to count, one to fill).  With a status other than Ok the arrays are empty."""
    import numpy as np

    buf, base = _host_input(tail)
    file_len = buf.size if file_len is None else int(file_len)
    raw, call = _ZstdSeekSummary(), lib().chip_zstd_seek_plan_host
    arrays = _count_then_fill("chip_zstd_seek_plan_host", lambda m, *out: call(base, buf.size, file_len, m, *out, C.byref(raw)),
                              lambda: raw.n_frames if raw.status == int(ZstdSeekStatus.Ok) else 0,
                              lambda m: (*_plan_arrays(m), np.zeros(m, np.uint32)), _np_ptr, max_frames)
    return (*arrays, ZstdSeekSummary(raw))


def zstd_seek_plan(tail, file_len=None, stream=None, max_frames=None):
    """chip_zstd_seek_plan over a uint8 device tensor (a view at any alignment) holding the last bytes of a file of file_len bytes
    (None: the tail is the file): (in_off int64, in_len int32, out_off int64, out_cap int32, checksum int32, summary), device
    tensors of the first min(n_frames, max_frames) entries (None = all of them: one call to count, one to fill), in_off in FILE
    coordinates.  With a status other than Ok the tensors are empty.  Synchronous on `stream`."""
    import torch

    dev = _check_tensors(((tail, torch.uint8),))
    tail_len = tail.numel()
    file_len = tail_len if file_len is None else int(file_len)
    raw, call = _ZstdSeekSummary(), lib().chip_zstd_seek_plan
    base, sp = (_dp(tail) if tail_len else None), _stream_ptr(stream)
    with torch.cuda.device(dev):
        arrays = _count_then_fill("chip_zstd_seek_plan", lambda m, *out: call(base, tail_len, file_len, m, *out, C.byref(raw), sp),
                                  lambda: raw.n_frames if raw.status == int(ZstdSeekStatus.Ok) else 0,
                                  lambda m: (*_plan_tensors(m, dev), torch.empty(m, dtype=torch.int32, device=dev)), _dp, max_frames)
    return (*arrays, ZstdSeekSummary(raw))


def zstd_seek_table_write_host(c_len, d_len, checksum=None):
    """chip_zstd_seek_table_write_host: the seek table of the entries (c_len[i], d_len[i][, checksum[i]]) as bytes."""
    import numpy as np

    arr = lambda a: np.ascontiguousarray(a, dtype=np.uint32)  # noqa: E731
    c_len, d_len = arr(c_len), arr(d_len)
    n = int(c_len.size)
    if d_len.size != n or (checksum is not None and arr(checksum).size != n):
        raise ValueError("the entries' arrays must have one length")
    # (an empty checksum array still means 12-byte entries: a one-word stand-in keeps the pointer non-NULL)
    cs = None if checksum is None else (arr(checksum) if n else np.zeros(1, np.uint32))
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None  # noqa: E731
    size = C.c_uint64(0)
    out = np.zeros(17 + (8 if cs is None else 12) * n, np.uint8)
    rc = lib().chip_zstd_seek_table_write_host(n, p(c_len), p(d_len), p(cs), p(out), out.size, C.byref(size))
    if rc != 0 or size.value != out.size:
        raise RuntimeError(f"chip_zstd_seek_table_write_host failed: {rc}")
    return out.tobytes()


def zstd_seek_table_write(c_len, d_len, checksum=None, out=None, stream=None):
    """chip_zstd_seek_table_write on device tensors (int32 read as u32): the table goes to `out` (a uint8 device tensor, a view at
    any alignment; None: a tensor of exactly the table's size).  Returns (out trimmed to the table -- None when `out` is too small,
    nothing is written then --, table_bytes).  Only enqueues on `stream`."""
    import torch

    pairs = [(c_len, torch.int32), (d_len, torch.int32)] + ([(checksum, torch.int32)] if checksum is not None else [])
    dev = _check_tensors(pairs + ([(out, torch.uint8)] if out is not None else []))
    n = c_len.numel()
    if d_len.numel() != n or (checksum is not None and checksum.numel() != n):
        raise ValueError("the entries' arrays must have one length")
    if out is None:
        out = torch.empty(17 + (8 if checksum is None else 12) * n, dtype=torch.uint8, device=dev)
    cs = None if checksum is None else (checksum if n else torch.zeros(1, dtype=torch.int32, device=dev))
    size = C.c_uint64(0)
    with torch.cuda.device(dev):
        rc = lib().chip_zstd_seek_table_write(n, _dp_or_none(c_len), _dp_or_none(d_len), _dp_or_none(cs), _dp_or_none(out), out.numel(),
                                              C.byref(size), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_zstd_seek_table_write failed: {rc}")
    return (out[: size.value] if size.value <= out.numel() else None), int(size.value)


def xxh64_batch(buf, off, length, stream=None):
    """chip_xxh64_batch on device tensors: XXH64 (seed 0) of buf[off[i] : off[i] + length[i]] for every i.  buf uint8, off int64
    (read as u64), length int32 (read as u32).  Returns an int64 device tensor (read it as u64; a seek table's entry is its low
    32 bits).  One wave per range.  Only enqueues on `stream`."""
    import torch

    dev = _check_tensors(((buf, torch.uint8), (off, torch.int64), (length, torch.int32)))
    n = off.numel()
    if length.numel() != n:
        raise ValueError("off and length must have one length")
    digest = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return digest
    with torch.cuda.device(dev):
        rc = lib().chip_xxh64_batch(n, _dp(buf), _dp(off), _dp(length), _dp(digest), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_xxh64_batch failed: {rc}")
    return digest


def zstd_seek_read(in_buf, in_off, in_len, out_off, out_cap, checksum, range_lo, range_len, dst=None, stream=None):
    """chip_zstd_seek_read on device tensors: read_ranges(FMT_ZSTD, ..) over the plan of a seek table, with the low 32 bits of
    every selected unit's XXH64 compared with checksum[unit] (int32 read as u32; None: read_ranges itself).  A unit that differs
    is a bad unit with bad_status -22.  Returns what read_ranges returns.  Synchronous on `stream`."""
    import torch

    pairs = [(in_buf, torch.uint8), (in_off, torch.int64), (in_len, torch.int32), (out_off, torch.int64), (out_cap, torch.int32),
             (range_lo, torch.int64), (range_len, torch.int32)] + ([(checksum, torch.int32)] if checksum is not None else [])
    n, m = out_cap.numel(), range_len.numel()
    mismatch = (not (in_off.numel() == in_len.numel() == out_off.numel() == n) or range_lo.numel() != m
                or (checksum is not None and checksum.numel() != n))
    q = _dp_or_none
    return _read_call("chip_zstd_seek_read", pairs, mismatch and "the plan's arrays, and the ranges' arrays, must have one length each", m, dst, stream,
                      lambda *out: lib().chip_zstd_seek_read(n, q(in_buf) if n else None, q(in_off), q(in_len), q(out_off), q(out_cap), q(checksum),
                                                             m, q(range_lo), q(range_len), *out))


def seekable_write(data, length, level=3, unit_bytes=0, checksums=True, out=None, stream=None):
    """A seekable zstd file of the first `length` bytes of the uint8 device tensor `data` (4-byte aligned, padded to a multiple
    of 4), with the seek table behind the last frame and, with `checksums`, the low 32 bits of every frame's content XXH64 in it:
    xxh64_batch over the chunks, encode_file(FMT_ZSTD, flags=0), zstd_plan of the frames for their sizes, zstd_seek_table_write.
    unit_bytes 0: 262144.  out None: a tensor of the bound is allocated.  Returns (the file as a uint8 device tensor -- None when
    `out` is too small --, FileSummary with n_units, out_len, table_off and the status)."""
    import torch

    dev = _check_tensors(((data, torch.uint8),) + (((out, torch.uint8),) if out is not None else ()))
    length, unit = int(length), int(unit_bytes) or 262144
    n = max(1, -(-length // unit))
    table = 17 + (12 if checksums else 8) * n
    if out is None:
        bound = encode_file_bound(FMT_ZSTD, length, unit, 0)
        if bound == 0:
            raise ValueError(f"seekable_write refuses unit_bytes {unit_bytes}, length {length}")
        out = torch.empty(bound + table, dtype=torch.uint8, device=dev)
    low = None
    with torch.cuda.device(dev):
        if checksums and length == 0:  # (no buffer to hash: the one frame of empty content)
            low = torch.tensor([0x51D8E999], dtype=torch.int32, device=dev)
        elif checksums:
            off = torch.arange(n, dtype=torch.int64, device=dev) * unit
            ln = torch.clamp(length - off, min=0, max=unit).to(torch.int32)
            low = xxh64_batch(data, off, ln, stream=stream).view(torch.int32)[::2].contiguous()  # (little endian: the low words)
    frames, summ = encode_file(FMT_ZSTD, level, data, length, unit, 0, stream=stream, out=out)
    raw = _FileSummary(summ.n_units, summ.out_len + table, summ.out_len, int(summ.status), 0)
    if frames is None or summ.out_len + table > out.numel():
        raw.status = int(FileStatus.NeedOutput)
        return None, FileSummary(raw)
    _, c_len, _, d_len, plan = zstd_plan(out, summ.out_len, stream=stream)
    if plan.status != ZstdPlanStatus.Ok or plan.n_frames != n or plan.n_unsized:
        raise RuntimeError(f"seekable_write: the frames just written do not plan as {n} sized frames: {plan!r}")
    _, size = zstd_seek_table_write(c_len, d_len, low, out=out[summ.out_len:], stream=stream)
    assert size == table
    return out[: summ.out_len + table], FileSummary(raw)


def _read_exact(f, pos, view):
    """seek + readinto until `view` (a writable memoryview of bytes) is full; EOFError when the source ends first"""
    f.seek(pos)
    got = 0
    while got < len(view):
        k = f.readinto(view[got:])
        if not k:
            raise EOFError(f"the source ended {len(view) - got} bytes short at {pos + got}")
        got += k


class SeekableZstd:
    """A reader of seekable zstd files that fetches the table and the frames its ranges touch, nothing else.
    open() plans the table; n_frames, size (the content's length), has_checksums and the plan (in_off, in_len, out_off, out_cap,
    checksum: numpy arrays, in_off in file coordinates) are its attributes; bytes_fetched counts what was read from the source."""

    def __init__(self, src, file_len, plan, summary, bytes_fetched, device_plan=None):
        self._src, self.file_len, self.summary, self.bytes_fetched = src, file_len, summary, bytes_fetched
        self.in_off, self.in_len, self.out_off, self.out_cap, self.checksum = plan
        self.n_frames, self.size, self.has_checksums = summary.n_frames, summary.total_out, bool(summary.checksums)
        self._dev = device_plan  # the plan as device tensors, once a read has needed it

    @classmethod
    def open(cls, src, length=None, tail_bytes=65536):
        """src: bytes, a seekable binary file object, or a uint8 device tensor holding the file (4-byte aligned, padded to a
        multiple of 4).  length: the file's length (None: all of src).  The last min(length, tail_bytes) bytes are read and
        planned (bytes and files: on the host; a tensor: on the device); a table that is larger costs a second read of exactly
        table_bytes.  ValueError, naming the status, for every status but Ok."""
        import io

        try:
            import torch

            on_device = isinstance(src, torch.Tensor)
        except ImportError:  # pragma: no cover - the host walk needs no torch
            on_device = False
        if on_device:
            file_len = src.numel() if length is None else int(length)
            if file_len < 0 or file_len > src.numel():
                raise ValueError(f"length {file_len} outside the buffer of {src.numel()} bytes")
            plan_of = lambda k: zstd_seek_plan(src[file_len - k:file_len], file_len)  # noqa: E731
        else:
            if isinstance(src, (bytes, bytearray, memoryview)):
                src = io.BytesIO(src)
            file_len = src.seek(0, 2) if length is None else int(length)
            fetched = [0]

            def plan_of(k):
                tail = bytearray(k)
                if k:
                    _read_exact(src, file_len - k, memoryview(tail))
                fetched[0] += k
                return zstd_seek_plan_host(tail, file_len)

        planned = plan_of(min(file_len, max(0, int(tail_bytes))))
        if planned[5].status == ZstdSeekStatus.NeedTail and planned[5].table_bytes <= file_len:
            planned = plan_of(planned[5].table_bytes)
        summ = planned[5]
        if summ.status != ZstdSeekStatus.Ok:
            raise ValueError(f"no usable seek table ({summ.status.name}): {summ!r}")
        if on_device:
            import numpy as np

            host = tuple(t.cpu().numpy().view(dt) for t, dt in zip(planned[:5], (np.uint64, np.uint32, np.uint64, np.uint32, np.uint32)))
            return cls(src, file_len, host, summ, 0, device_plan=planned[:5])
        return cls(src, file_len, planned[:5], summ, fetched[0])

    def _device_plan(self, dev):
        import numpy as np
        import torch

        if self._dev is None or self._dev[1].device != dev:
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
            self._dev = (up(self.in_off, np.int64), up(self.in_len, np.int32), up(self.out_off, np.int64), up(self.out_cap, np.int32),
                         up(self.checksum, np.int32))
        return self._dev

    def read(self, ranges, verify=True, stream=None):
        """The bytes of `ranges`, a sequence of (lo, len) pairs in content coordinates: (the uint8 device tensor of the ranges end
        to end, dst_off int64).  From a file or bytes, the frames the ranges touch are read -- runs of frames that are adjacent in
        the file with one seek + readinto each, into pinned memory -- and uploaded; zstd_seek_read decodes them, with the table's
        checksums verified unless `verify` is false or the table has none.  Raises ValueError for a range outside the content,
        RuntimeError with the first bad frame's index and status (-22: its checksum) when a frame does not decode to its entry."""
        import numpy as np
        import torch

        ranges = [(int(lo), int(ln)) for lo, ln in ranges]
        if isinstance(self._src, torch.Tensor):
            dev = self._src.device
            in_off, in_len, out_off, out_cap, checksum = self._device_plan(dev)
            buf = self._src
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
            _, in_len, out_off, out_cap, checksum = self._device_plan(dev)
            sel = select_units_host(self.in_off, self.in_len, self.out_off, self.out_cap, [r[0] for r in ranges], [r[1] for r in ranges])
            units, s_off, s_len = sel[0], sel[1], sel[2]
            runs, at = [], 0  # (file offset, bytes, offset in the buffer) of every run of adjacent frames
            rebased = np.zeros(self.n_frames, np.int64)
            for u, o, ln in zip(units.tolist(), s_off.tolist(), s_len.tolist()):
                if runs and runs[-1][0] + runs[-1][1] == o:
                    runs[-1][1] += ln
                else:
                    runs.append([o, ln, at])
                rebased[u] = at
                at += ln
            if at > self.file_len or any(o + ln > self.file_len for o, ln, _ in runs):
                raise ValueError("the seek table names bytes behind the end of the file")
            pinned = torch.zeros(max(4, (at + 3) // 4 * 4), dtype=torch.uint8).pin_memory()
            view = memoryview(pinned.numpy())
            for o, ln, b in runs:
                _read_exact(self._src, o, view[b:b + ln])
            self.bytes_fetched += at
            buf = pinned.to(dev)
            in_off = torch.from_numpy(rebased).to(dev)
        lo, ln = _ranges_to_device(ranges, dev)
        cs = checksum if verify and self.has_checksums else None
        out, dst_off, status, summ = zstd_seek_read(buf, in_off, in_len, out_off, out_cap, cs, lo, ln, stream=stream)
        return _read_checked("SeekableZstd.read", out, status, summ), dst_off

    def read_bytes(self, lo, n, verify=True):
        """bytes [lo, lo + n) of the content, as bytes"""
        out, _ = self.read([(lo, n)], verify=verify)
        return bytes(out.cpu().numpy())


# ---- one large stream: the checkpoint index (include/compu_hip.h, "one large stream") ------------

INDEX_WINDOW = 32768  # bytes of a window slot


class InflateIndexSummary(_Summary):
    """chip_inflate_index_summary: n_points of the whole walk; out_len, in_used and status as decode_batch answers them for the
    unit; wrap 0 raw / 1 zlib / 2 gzip; with status Finished, check = the content's CRC-32 / Adler-32 and end_bit = the bit behind
    the final block."""

    __slots__ = FIELDS = _fields(_InflateIndexSummary)
    FORMATS = {"check": "#010x"}


class InflateIndex:
    """The checkpoint index of one stream in device memory: pt_bit / pt_out int64 (read as u64), pt_check int32 (read as u32),
    windows uint8 (32 768 bytes per point), the stream's length `length`, its decoded length `total_out` and its format (the
    build's wrap: ZlibMode.Deflate, Zlib or Gzip)."""

    __slots__ = ("fmt", "length", "total_out", "pt_bit", "pt_out", "pt_check", "windows")

    def __init__(self, fmt, length, total_out, pt_bit, pt_out, pt_check, windows):
        self.fmt, self.length, self.total_out = int(fmt), int(length), int(total_out)
        self.pt_bit, self.pt_out, self.pt_check, self.windows = pt_bit, pt_out, pt_check, windows

    @property
    def n_points(self):
        return self.pt_bit.numel()


_WRAP_FMT = (-15, 15, 31)  # the format of a wrap: CHIP_FMT_DEFLATE, CHIP_FMT_ZLIB, CHIP_FMT_GZIP


def inflate_index_build(fmt, in_buf, length, out_buf, spacing=0, max_points=None, stream=None):
    """chip_inflate_index_build: decode the ONE unit in_buf[:length] (uint8 device tensor, 4-byte aligned, padded to a multiple of
    4) into out_buf and record a point every `spacing` decoded bytes (0 = 1 MiB).  Returns (index, summary): an InflateIndex of the
    first min(n_points, max_points) points -- max_points None: all of them, sized by the worst case of one point per `spacing`
    bytes of room, or by a counting pass first where that would be more than 1 GiB of windows -- and the InflateIndexSummary.  The decode's answers are decode_batch's for the same unit and room.
    Synchronous on `stream`."""
    import torch

    dev = _check_tensors(((in_buf, torch.uint8), (out_buf, torch.uint8)))
    step = int(spacing) if spacing else 1 << 20
    q = lambda t: _dp(t) if t.numel() else None  # noqa: E731
    raw = _InflateIndexSummary()

    def call(k, pt_bit, pt_out, pt_check, windows):
        with torch.cuda.device(dev):
            rc = lib().chip_inflate_index_build(int(fmt), _dp(in_buf), int(length), _dp(out_buf), out_buf.numel(), int(spacing), k, pt_bit, pt_out,
                                                pt_check, windows, C.byref(raw), _stream_ptr(stream))
        if rc != 0:
            raise RuntimeError(f"chip_inflate_index_build failed: {rc}")

    if max_points is not None:
        k = int(max_points)
    else:
        k = out_buf.numel() // step + 1  # a point needs `spacing` new bytes: no walk has more
        if k * INDEX_WINDOW > 1 << 30:   # small spacings: a first pass counts instead of a gigabyte of window slots
            call(0, None, None, None, None)
            k = int(raw.n_points)
    pt_bit, pt_out = torch.zeros(k, dtype=torch.int64, device=dev), torch.zeros(k, dtype=torch.int64, device=dev)
    pt_check, windows = torch.zeros(k, dtype=torch.int32, device=dev), torch.empty(k * INDEX_WINDOW, dtype=torch.uint8, device=dev)
    call(k, q(pt_bit), q(pt_out), q(pt_check), q(windows))
    summ = InflateIndexSummary(raw)
    n = min(k, summ.n_points)
    index = InflateIndex(_WRAP_FMT[summ.wrap] if summ.wrap < 3 else int(fmt), length, summ.out_len, pt_bit[:n], pt_out[:n], pt_check[:n],
                         windows[: n * INDEX_WINDOW])
    return index, summ


def inflate_index_units_host(fmt, length, pt_bit, pt_out, pt_check, total_out):
    """chip_inflate_index_units_host over numpy arrays (or sequences): the chunks of an index by host arithmetic.  Returns
    (in_off u64, in_len u32, out_cap u32, win_len u32, resume u32[n, 6], status ReadStatus, bad_index); on BadLayout the arrays
    are empty."""
    import numpy as np

    arr = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    pt_bit, pt_out, pt_check = arr(pt_bit, np.uint64), arr(pt_out, np.uint64), arr(pt_check, np.uint32)
    n = int(pt_bit.size)
    if pt_out.size != n or pt_check.size != n:
        raise ValueError("the index's arrays must have one length")
    in_off, in_len, out_cap, win_len = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    resume = np.zeros((n, 6), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    status, bad = C.c_int32(0), C.c_uint64(0)
    rc = lib().chip_inflate_index_units_host(int(fmt), int(length), n, p(pt_bit), p(pt_out), p(pt_check), int(total_out), p(in_off), p(in_len),
                                             p(out_cap), p(win_len), p(resume), C.byref(status), C.byref(bad))
    if rc != 0:
        raise RuntimeError(f"chip_inflate_index_units_host failed: {rc}")
    if status.value != int(ReadStatus.Ok):
        n = 0
    return in_off[:n], in_len[:n], out_cap[:n], win_len[:n], resume[:n], ReadStatus(status.value), int(bad.value)


def inflate_index_read(index, in_buf, range_lo, range_len, dst=None, stream=None):
    """chip_inflate_index_read on device tensors: the bytes of every range (range_lo int64 read as u64, range_len int32 read as
    u32, in content coordinates) of the stream in_buf[:index.length], end to end in dst.  Only the chunks the ranges touch are
    decoded, each once, and each is verified against the next point's check value.  dst as in read_ranges.  Returns (dst trimmed
    to out_len -- None on NeedOutput or BadLayout --, dst_off int64, range_status int32, ReadSummary).  Synchronous on `stream`."""
    import torch

    pairs = [(in_buf, torch.uint8), (index.pt_bit, torch.int64), (index.pt_out, torch.int64), (index.pt_check, torch.int32),
             (index.windows, torch.uint8), (range_lo, torch.int64), (range_len, torch.int32)]
    n, m = index.pt_bit.numel(), range_len.numel()
    mismatch = index.pt_out.numel() != n or index.pt_check.numel() != n or index.windows.numel() < n * INDEX_WINDOW or range_lo.numel() != m
    q = _dp_or_none
    return _read_call("chip_inflate_index_read", pairs, mismatch and "the index's arrays, and the ranges' arrays, must have one length each", m, dst,
                      stream, lambda *out: lib().chip_inflate_index_read(index.fmt, _dp(in_buf), index.length, n, q(index.pt_bit), q(index.pt_out),
                                                                         q(index.pt_check), q(index.windows), index.total_out, m, q(range_lo),
                                                                         q(range_len), *out))


def gzip_index_decode(index, in_buf, stream=None):
    """The whole content of an indexed stream (gzip, zlib or raw deflate), every chunk on a wave of its own: inflate_index_read of
    [0, total_out) in pieces of at most 2^31 bytes.  With every chunk good the stream's own CRC-32 / Adler-32 is verified.  Raises
    ValueError on a broken index layout, RuntimeError with the first bad chunk.  Returns the uint8 tensor.  Waits for the result."""
    piece = 1 << 31
    ranges = [(lo, min(piece, index.total_out - lo)) for lo in range(0, index.total_out, piece)]
    lo, ln = _ranges_to_device(ranges, in_buf.device)
    out, _, status, rs = inflate_index_read(index, in_buf, lo, ln, stream=stream)
    return _read_checked("gzip_index_decode", out, status, rs)


def gzip_index_read(index, in_buf, ranges, stream=None):
    """Bytes of an indexed stream without decoding all of it.  `ranges` is a sequence of (lo, len) pairs in decoded coordinates,
    or a pair of device tensors (int64, int32).  Raises as bgzf_read does.  Returns (the uint8 tensor of the ranges end to end,
    dst_off int64).  Waits for the result."""
    lo, ln = _ranges_to_device(ranges, in_buf.device)
    out, dst_off, status, rs = inflate_index_read(index, in_buf, lo, ln, stream=stream)
    return _read_checked("gzip_index_read", out, status, rs), dst_off


# ---- ZIP archives (include/compu_hip.h, "ZIP archives") ---------------------------------------------


class ZipStatus(enum.IntEnum):
    Ok = 0
    NoEocd = 1
    BadDirectory = 2
    Unsupported = 3


class ZipEntryStatus(enum.IntEnum):
    """chip_zip_entry.status, and what zip_decode answers beside the decode statuses (DecodeStatus, negative codec errors)."""

    Ok = 0
    Unsupported = 16
    Encrypted = 17
    BadLocal = 18
    TooLarge = 19
    BadSize = 20
    BadCrc = 21
    BadIndex = 22


CRC_PIECE = 65536  # CHIP_CRC_PIECE: the piece a range of crc32_batch is cut into


def zip_entry_dtype():
    """chip_zip_entry as a numpy record: header_off, data_off, comp_size, size, name_off, crc32, name_len, method, flags, pad, status."""
    import numpy as np

    dt = np.dtype(_ZipEntry)
    assert dt.itemsize == 56
    return dt


class ZipPlanSummary(_Summary):
    """chip_zip_plan_summary: n_entries, n_ok and total_size (decoded bytes of the OK entries) of the whole walk, the directory's
    place (cd_off, cd_size), the end record's (eocd_off), bad_index (the entry a BadDirectory walk stopped at), status, zip64."""

    __slots__ = FIELDS = _fields(_ZipPlanSummary)
    ENUMS = {"status": ZipStatus}


class ZipDecodeSummary(_Summary):
    """chip_zip_decode_summary: n_sel, n_ok (entries that are Finished), n_bad, first_bad (position in the selection), total_out,
    status (ReadStatus.Ok or NeedOutput)."""

    __slots__ = FIELDS = _fields(_ZipDecodeSummary)
    ENUMS = {"status": ReadStatus}


def zip_plan_host(data, max_entries=None):
    """chip_zip_plan_host over bytes / a uint8 numpy array in host memory: (entries, summary), entries a numpy record array
    (zip_entry_dtype) of the first min(n_entries, max_entries) entries (None = all of them: one call to count, one to fill).  Read
    from the directory and the local headers alone; nothing is decoded."""
    return _plan_host("chip_zip_plan_host", _ZipPlanSummary, ZipPlanSummary, "n_entries", data, max_entries, _record_array(zip_entry_dtype()))


def zip_plan(in_buf, length, stream=None, max_entries=None):
    """chip_zip_plan over a uint8 device tensor holding a ZIP archive of `length` bytes (4-byte aligned, padded to a multiple of 4):
    (entries, summary), entries a uint8 device tensor of shape (k, 56) holding the chip_zip_entry records of the first
    k = min(n_entries, max_entries) entries (`.cpu().numpy().view(zip_entry_dtype())` reads them; zip_decode takes the tensor).
    Synchronous on `stream`.  max_entries None: all of them (one call to count, one to fill)."""
    return _plan_device("chip_zip_plan", _ZipPlanSummary, ZipPlanSummary, "n_entries", in_buf, length, stream, max_entries, _record_rows(_ZipEntry))


def zip_names(entries, summary, directory):
    """The names of a plan's entries, as bytes: `entries` the records (the numpy record array of zip_plan_host, or the device
    tensor of zip_plan, which is copied to the host), `directory` a bytes copy of the archive's
    [summary.cd_off, summary.cd_off + summary.cd_size), which is where the names lie."""
    import numpy as np

    if not isinstance(entries, np.ndarray):
        entries = entries.cpu().numpy().reshape(-1).view(zip_entry_dtype())
    directory = bytes(directory)
    if len(directory) != summary.cd_size:
        raise ValueError(f"the directory has {summary.cd_size} bytes, got {len(directory)}")
    names = []
    for e in entries:
        at = int(e["name_off"]) - summary.cd_off
        names.append(directory[at:at + int(e["name_len"])])
    return names


def crc32_batch(buf, off, length, stream=None):
    """chip_crc32_batch on device tensors: the CRC-32 (zlib.crc32) of buf[off[i] : off[i] + length[i]] for every i.  buf uint8, off and
    length int64 (read as u64).  Returns an int32 device tensor (read it as u32: `& 0xFFFFFFFF`).  Enqueues on `stream`; waits once
    in between to size its scratch, not for the result."""
    import torch

    dev = _check_tensors(((buf, torch.uint8), (off, torch.int64), (length, torch.int64)))
    n = off.numel()
    if length.numel() != n:
        raise ValueError("off and length must have one length")
    crc = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return crc
    with torch.cuda.device(dev):
        rc = lib().chip_crc32_batch(n, _dp(buf), _dp(off), _dp(length), _dp(crc), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_crc32_batch failed: {rc}")
    return crc


def zip_decode(in_buf, length, names_or_indices=None, stream=None):
    """Entries of a ZIP archive in device memory, planned by chip_zip_plan and decoded, copied and verified by chip_zip_decode.
    in_buf is a uint8 device tensor holding the archive's `length` bytes (4-byte aligned, padded to a multiple of 4).
    names_or_indices: None for every entry in order, else a sequence of entry indices and / or names (str, matched as UTF-8, or
    bytes; the LAST entry of that name, as zipfile does; the names are read from a host copy of the directory), or an int32 device
    tensor of indices (read as u32).  The output tensor is allocated here: one call for total_out, one to decode.
    Raises ValueError when the archive's directory is refused (the summary says why), KeyError for an unknown name.  Damaged
    entries do not raise: returns (out, out_off int64, sizes int64, status int32, summary), device tensors of one row per selected
    entry; status is DecodeStatus.Finished (2) for an entry whose bytes are out[out_off : out_off + size] and verified; sizes is the
    room each entry takes in `out`, 0 for one that did not take part (its plan status says why).  Waits for the result."""
    import numpy as np
    import torch

    dev = _check_tensors(((in_buf, torch.uint8),))
    length = int(length)
    entries, summ = zip_plan(in_buf, length, stream=stream)
    if summ.status != ZipStatus.Ok:
        raise ValueError(f"not a ZIP archive this library reads: {summ!r}")
    n_entries = entries.shape[0]
    sel = None
    if names_or_indices is None:
        n_sel = n_entries
    elif isinstance(names_or_indices, torch.Tensor):
        sel = names_or_indices
        _check_tensors(((in_buf, torch.uint8), (sel, torch.int32)))
        n_sel = sel.numel()
    else:
        wanted = list(names_or_indices)
        if any(not isinstance(w, (int, np.integer)) for w in wanted):
            directory = in_buf[summ.cd_off:summ.cd_off + summ.cd_size].cpu().numpy().tobytes()
            index = {name: i for i, name in enumerate(zip_names(entries, summ, directory))}
            wanted = [w if isinstance(w, (int, np.integer)) else index[w.encode("utf-8") if isinstance(w, str) else bytes(w)] for w in wanted]
        sel = torch.tensor(np.asarray(wanted, dtype=np.int64).astype(np.uint32).view(np.int32), dtype=torch.int32, device=dev)
        n_sel = len(wanted)
    out_off = torch.empty(n_sel, dtype=torch.int64, device=dev)
    status = torch.empty(n_sel, dtype=torch.int32, device=dev)
    raw = _ZipDecodeSummary()
    sp = _stream_ptr(stream)

    def call(o):
        with torch.cuda.device(dev):
            rc = lib().chip_zip_decode(_dp(in_buf) if length else None, length, _dp(entries) if n_entries else None, n_entries, n_sel,
                                       _dp(sel) if sel is not None and n_sel else None, _dp(o) if o.numel() else None, o.numel(),
                                       _dp(out_off) if n_sel else None, _dp(status) if n_sel else None, C.byref(raw), sp)
        if rc != 0:
            raise RuntimeError(f"chip_zip_decode failed: {rc}")

    out = torch.empty(0, dtype=torch.uint8, device=dev)
    call(out)  # sizes only: NeedOutput with the exact total, or an empty result
    if raw.status == ReadStatus.NeedOutput:
        out = torch.empty(int(raw.total_out), dtype=torch.uint8, device=dev)
        call(out)
    summary = ZipDecodeSummary(raw)
    # the sizes of the entries that took part: the differences of the layout
    ends = torch.cat((out_off[1:], torch.tensor([summary.total_out], dtype=torch.int64, device=dev))) if n_sel else out_off
    return out, out_off, ends - out_off, status, summary


# ---- ZIP archives: writing (include/compu_hip.h, "ZIP archives: writing") ---------------------------

ZIP_STORE, ZIP_DEFLATE = 0, 8  # CHIP_ZIP_STORE, CHIP_ZIP_DEFLATE: chip_zip_source.method
ZW_ZIP64, ZW_UTF8 = 1, 2  # CHIP_ZW_ZIP64 (every record in its ZIP64 form), CHIP_ZW_UTF8 (gp flag bit 11: the names are UTF-8)
ZIPW_DEFLATE_MAX = 1 << 30  # CHIP_ZIPW_DEFLATE_MAX: zip_write stores a larger entry


class ZipWriteStatus(enum.IntEnum):
    Ok = 0
    NeedOutput = 1
    BadSource = 2


def zip_source_dtype():
    """chip_zip_source as a numpy record: data_off, size, name_off, name_len, method, dos_time, dos_date."""
    import numpy as np

    dt = np.dtype(_ZipSource)
    assert dt.itemsize == 32
    return dt


class ZipWriteSummary(_Summary):
    """chip_zip_write_summary: n_entries, n_deflated (entries written with method 8), out_len (the archive's length; the exact room
    to come back with on NeedOutput), the directory's place (cd_off, cd_size), the end record's (eocd_off), bad_index (the lowest
    bad record on BadSource), status, zip64."""

    __slots__ = FIELDS = _fields(_ZipWriteSummary)
    ENUMS = {"status": ZipWriteStatus}


# what the archive writers' two-call protocol is told of a format: the raw summary, its wrapper, the entry record and the status
# enum (with Ok and NeedOutput)
_ZIP_ARCHIVE = (_ZipWriteSummary, ZipWriteSummary, _ZipEntry, ZipWriteStatus)


def zip_write_bound(n, names_total, content_total):
    """chip_zip_write_bound: the room that is always enough for n entries with names_total bytes of names and content_total bytes of
    content; 0 when it overflows 64 bits."""
    return int(lib().chip_zip_write_bound(int(n), int(names_total), int(content_total)))


def zip_assemble_host(sources, names, content, crc, comp=None, comp_off=None, comp_len=None, flags=0, out_cap=None, content_len=None):
    """chip_zip_assemble_host: `sources` a numpy record array (zip_source_dtype), names / content / comp bytes or uint8 arrays, crc a
    uint32 array, comp_off uint64 and comp_len uint32 arrays (comp, comp_off, comp_len all None: every entry is stored).  out_cap
    None: one call for the size, one to write.  content_len overrides len(content) for a call that only sizes (out_cap smaller than
    the archive: the content is never read).  Returns (the archive as bytes -- b"" unless status is Ok --, entries as a numpy record
    array of zip_entry_dtype, ZipWriteSummary)."""
    import numpy as np

    u8 = lambda b: None if b is None else (np.ascontiguousarray(b, dtype=np.uint8) if isinstance(b, np.ndarray) else np.frombuffer(bytes(b), np.uint8))  # noqa: E731
    src = np.ascontiguousarray(sources, dtype=zip_source_dtype())
    n = src.size
    names, content, comp = u8(names), u8(content), u8(comp)
    crc = np.ascontiguousarray(crc, dtype=np.uint32)
    if crc.size != n:
        raise ValueError("one CRC per source")
    if comp is not None:
        comp_off, comp_len = np.ascontiguousarray(comp_off, dtype=np.uint64), np.ascontiguousarray(comp_len, dtype=np.uint32)
        if comp_off.size != n or comp_len.size != n:
            raise ValueError("one comp_off and one comp_len per source")
        comp_all = comp.size
        if comp.size == 0:
            comp = np.zeros(1, np.uint8)  # (an empty stream buffer still has an address)
    else:
        comp_off = comp_len = None
        comp_all = 0
    p = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pc = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    clen = content.size if content_len is None else int(content_len)

    def call(out, cap, ent, raw):
        return lib().chip_zip_assemble_host(n, p(src), p(names), names.size, pc(content) if clen else None, clen, pc(comp), comp_all, pc(comp_off),
                                            pc(comp_len), p(crc), flags, out, cap, ent, raw)

    return _archive_host_call("chip_zip_assemble_host", _ZIP_ARCHIVE, call, n, out_cap)


def _archive_host_call(what, kind, call, n, out_cap):
    """the two-call protocol of zip_assemble_host / tar_write_host: `call` makes the C call `what`, given its last four arguments (out,
    its size, the n entries, summary).  out_cap None: one call for the size, one to write"""
    import numpy as np

    raw_cls, wrap, entry, status = kind
    raw, entries = raw_cls(), np.zeros(n, np.dtype(entry))

    def once(out):
        rc = call(_np_ptr(out), out.size, _np_ptr(entries), C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    out = np.zeros(0 if out_cap is None else int(out_cap), np.uint8)
    once(out)
    if out_cap is None and raw.status == status.NeedOutput:
        out = np.zeros(int(raw.out_len), np.uint8)
        once(out)
    summ = wrap(raw)
    return (out[:summ.out_len].tobytes() if summ.status == status.Ok else b""), entries, summ


def _archive_device_call(what, kind, call, n, dev, out, stream):
    """the two-call protocol of zip_assemble / zip_write / tar_write: `call` makes the C call `what`, given its last five arguments (out,
    its size, the n entries, summary, stream).  `out` None allocates the exact room after a sizing call"""
    import torch

    raw_cls, wrap, entry, status = kind
    raw = raw_cls()
    entries = torch.empty((n, C.sizeof(entry)), dtype=torch.uint8, device=dev)

    def once(o):
        with torch.cuda.device(dev):
            rc = call(_dp(o) if o.numel() else None, o.numel(), _dp(entries) if n else None, C.byref(raw), _stream_ptr(stream))
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    if out is None:
        out = torch.empty(0, dtype=torch.uint8, device=dev)
        once(out)
        if raw.status == status.NeedOutput:
            out = torch.empty(int(raw.out_len), dtype=torch.uint8, device=dev)
            once(out)
    else:
        once(out)
    summ = wrap(raw)
    return (out[:summ.out_len] if summ.status == status.Ok else out[:0]), entries, summ


def zip_assemble(sources, names, content, crc, comp=None, comp_off=None, comp_len=None, flags=0, out=None, stream=None):
    """chip_zip_assemble on device tensors: sources uint8 of shape (n, 32) holding chip_zip_source records
    (`torch.from_numpy(records.view(np.uint8).reshape(-1, 32)).cuda()`), names / content / comp uint8, crc int32 (read as u32), comp_off
    int64, comp_len int32 (comp, comp_off, comp_len all None: every entry is stored).  out None: the exact room is allocated after a
    sizing call; else a uint8 tensor, and too little room is status NeedOutput with nothing written.  Returns (the archive: a view of
    `out`, empty unless status is Ok; entries: uint8 of shape (n, 56), what zip_plan would answer; ZipWriteSummary).  Synchronous on
    `stream`."""
    import torch

    pairs = [(sources, torch.uint8), (names, torch.uint8), (content, torch.uint8), (crc, torch.int32)]
    if comp is not None or comp_off is not None or comp_len is not None:
        pairs += [(comp, torch.uint8), (comp_off, torch.int64), (comp_len, torch.int32)]
    if out is not None:
        pairs.append((out, torch.uint8))
    dev = _check_tensors(pairs)
    n = sources.numel() // C.sizeof(_ZipSource)
    if sources.numel() != n * C.sizeof(_ZipSource) or crc.numel() != n or (comp is not None and (comp_off.numel() != n or comp_len.numel() != n)):
        raise ValueError("sources holds 32-byte records; crc, comp_off and comp_len one value per record")
    q = lambda t: _dp(t) if t is not None and t.numel() else None  # noqa: E731
    have = comp is not None
    if have and comp.numel() == 0:
        comp = torch.zeros(16, dtype=torch.uint8, device=dev)  # (an empty stream buffer still has an address)
        comp_all = 0
    else:
        comp_all = comp.numel() if have else 0

    def call(o, cap, ent, raw, sp):
        return lib().chip_zip_assemble(n, q(sources), q(names), names.numel(), q(content), content.numel(), _dp(comp) if have else None, comp_all,
                                       _dp(comp_off) if have else None, _dp(comp_len) if have else None, q(crc), flags, o, cap, ent, raw, sp)

    return _archive_device_call("chip_zip_assemble", _ZIP_ARCHIVE, call, n, dev, out, stream)


def zip_write(sources, names, content, level=6, flags=0, out=None, stream=None):
    """chip_zip_write on device tensors: content to archive in one call -- the CRC-32 of every entry, the deflate-eligible entries
    encoded at `level` (one wave each), the assembly.  sources / names / out as for zip_assemble; content a uint8 tensor, 4-byte aligned
    and padded to a multiple of 4, the sources' data_off at any alignment.  Returns (archive, entries, ZipWriteSummary) as
    zip_assemble does.  Synchronous on `stream`."""
    import torch

    pairs = [(sources, torch.uint8), (names, torch.uint8), (content, torch.uint8)] + ([(out, torch.uint8)] if out is not None else [])
    dev = _check_tensors(pairs)
    n = sources.numel() // C.sizeof(_ZipSource)
    if sources.numel() != n * C.sizeof(_ZipSource):
        raise ValueError("sources holds 32-byte records")
    q = lambda t: _dp(t) if t.numel() else None  # noqa: E731

    def call(o, cap, ent, raw, sp):
        return lib().chip_zip_write(level, flags, n, q(sources), q(names), names.numel(), q(content), content.numel(), o, cap, ent, raw, sp)

    return _archive_device_call("chip_zip_write", _ZIP_ARCHIVE, call, n, dev, out, stream)


def zip_write_items(items, level=6, flags=0, stream=None, device=None):
    """A ZIP archive of (name, content) pairs on the device.  name: str (encoded as UTF-8, and ZW_UTF8 is set for the archive) or
    bytes; content: bytes-like, or a uint8 device tensor.  Every entry asks for method 8 (zip_write stores what does not shrink);
    the contents land at 4-byte aligned offsets of one device buffer, the DOS date is 1980-01-01.  Returns (the archive as a uint8
    device tensor, entries, ZipWriteSummary) as zip_write does."""
    import numpy as np

    items = list(items)
    src = np.zeros(len(items), zip_source_dtype())
    names, at = bytearray(), 0
    for i, (name, c) in enumerate(items):
        if isinstance(name, str):
            name, flags = name.encode("utf-8"), flags | ZW_UTF8
        if len(name) > 65535:
            raise ValueError("a name has at most 65535 bytes")
        size = _item_size(c)
        src[i] = (at, size, len(names), len(name), ZIP_DEFLATE, 0, 0x21)
        names += name
        at += (size + 3) // 4 * 4
    d_src, d_names, content = _upload_items(src, names, [c for _, c in items], at, device)
    return zip_write(d_src, d_names, content, level=level, flags=flags, stream=stream)


def _item_size(c):
    """the bytes of an item's content: bytes-like, or a uint8 device tensor"""
    import torch

    return c.numel() if isinstance(c, torch.Tensor) else len(memoryview(c).cast("B"))


def _upload_items(src, names, contents, total, device):
    """What zip_write_items and tar_write_items share behind their source records: the contents laid into one zeroed device buffer
    of `total` bytes at the records' data_off, the records and the names uploaded.  The device is that of the first content that is
    a tensor, else `device` (None: "cuda").  Returns (the records as a uint8 tensor of one row each, names, content)."""
    import numpy as np
    import torch

    tensors = [c for c in contents if isinstance(c, torch.Tensor)]
    dev = tensors[0].device if tensors else torch.device("cuda" if device is None else device)
    content = torch.zeros(total, dtype=torch.uint8, device=dev)
    for row, c in zip(src, contents):
        o, size = int(row["data_off"]), int(row["size"])
        if size:
            if isinstance(c, torch.Tensor):
                _check_tensors(((content, torch.uint8), (c, torch.uint8)))
                content[o:o + size] = c.reshape(-1)
            else:
                content[o:o + size] = torch.from_numpy(np.frombuffer(memoryview(c).cast("B"), np.uint8).copy()).to(dev)
    d_src = torch.from_numpy(src.view(np.uint8).reshape(-1, src.dtype.itemsize).copy()).to(dev)
    d_names = torch.from_numpy(np.frombuffer(bytes(names), np.uint8).copy()).to(dev)
    return d_src, d_names, content


# ---- one large stream: block starts (include/compu_hip.h, "block starts") -------------------------


def inflate_find_starts_host(data, first_bit, chunk_bytes, max_starts=None):
    """chip_inflate_find_starts_host over bytes / a uint8 numpy array in host memory: per chunk of `chunk_bytes` behind the first,
    the least bit position behind `first_bit` (the bit of the stream's first block header) at which a dynamic block header the
    decoder accepts begins.  Returns (starts u64, ascending: the first min(n, max_starts) of them, None = all: one call to count,
    one to fill; n).  A start is a candidate, not a confirmed boundary."""
    import numpy as np

    buf, base = _host_input(data)
    n, call = C.c_uint64(0), lib().chip_inflate_find_starts_host
    starts, = _count_then_fill("chip_inflate_find_starts_host",
                               lambda m, out: call(base, buf.size, int(first_bit), int(chunk_bytes), m, out, C.byref(n)), lambda: n.value,
                               lambda m: (np.zeros(m, np.uint64),), _np_ptr, max_starts)
    return starts, int(n.value)


def inflate_find_starts(in_buf, length, first_bit, chunk_bytes, stream=None, max_starts=None):
    """chip_inflate_find_starts over a uint8 device tensor holding `length` bytes of one deflate stream: the same answer as
    inflate_find_starts_host, one wave per chunk.  Returns (starts int64 device tensor read as u64, n).  Synchronous on `stream`."""
    import torch

    dev, length, base = _device_input(in_buf, length)
    sp, n, call = _stream_ptr(stream), C.c_uint64(0), lib().chip_inflate_find_starts
    with torch.cuda.device(dev):
        starts, = _count_then_fill("chip_inflate_find_starts",
                                   lambda m, out: call(base, length, int(first_bit), int(chunk_bytes), m, out, C.byref(n), sp), lambda: n.value,
                                   lambda m: (torch.empty(m, dtype=torch.int64, device=dev),), _dp, max_starts)
    return starts, int(n.value)


PAR_SERIAL, PAR_PARALLEL = 0, 1  # chip_inflate_parallel_summary::path
PAR_DEFAULT_CHUNK = 128 << 10


class InflateParallelSummary(_Summary):
    """chip_inflate_parallel_summary: the index build's fields; total_out (with status NeedOutput and out_len 0: the size to come
    back with); n_starts the finder's count, n_false those that were no boundaries; path PAR_SERIAL or PAR_PARALLEL."""

    __slots__ = FIELDS = _fields(_InflateParallelSummary)


def inflate_parallel(fmt, in_buf, length, out_buf=None, chunk_bytes=0, index=False, stream=None):
    """chip_inflate_parallel: decode the ONE stream in_buf[:length] (uint8 device tensor, 4-byte aligned, padded to a multiple of 4)
    with a wave per chunk of `chunk_bytes` (0 = 128 KiB) that holds a block start.  out_buf None: a first call asks for the size, a
    tensor of that size is allocated and the second call decodes.  Returns (out trimmed to out_len, summary), or with index=True
    (out, InflateIndex of the chain's chunks -- what gzip_index_read takes --, summary).  Synchronous on `stream`."""
    import torch

    pairs = [(in_buf, torch.uint8)] + ([(out_buf, torch.uint8)] if out_buf is not None else [])
    dev = _check_tensors(pairs)
    length = int(length)
    raw = _InflateParallelSummary()

    def call(out, k, pt_bit, pt_out, pt_check, windows):
        with torch.cuda.device(dev):
            rc = lib().chip_inflate_parallel(int(fmt), _dp(in_buf), length, _dp(out) if out is not None and out.numel() else None,
                                             out.numel() if out is not None else 0, int(chunk_bytes), k, pt_bit, pt_out, pt_check, windows,
                                             C.byref(raw), _stream_ptr(stream))
        if rc != 0:
            raise RuntimeError(f"chip_inflate_parallel failed: {rc}")

    if out_buf is None:
        call(None, 0, None, None, None, None)
        out_buf = torch.empty(int(raw.total_out) if raw.status == int(DecodeStatus.NeedOutput) else 0, dtype=torch.uint8, device=dev)
    k = -(-max(length, 1) // (int(chunk_bytes) or PAR_DEFAULT_CHUNK)) if index else 0  # a chunk has at most one point
    pt_bit, pt_out = torch.zeros(k, dtype=torch.int64, device=dev), torch.zeros(k, dtype=torch.int64, device=dev)
    pt_check, windows = torch.zeros(k, dtype=torch.int32, device=dev), torch.empty(k * INDEX_WINDOW, dtype=torch.uint8, device=dev)
    q = lambda t: _dp(t) if t.numel() else None  # noqa: E731
    call(out_buf, k, q(pt_bit), q(pt_out), q(pt_check), q(windows))
    summ = InflateParallelSummary(raw)
    if not index:
        return out_buf[: summ.out_len], summ
    n = min(k, summ.n_points) if summ.status != int(DecodeStatus.NeedOutput) else 0
    idx = InflateIndex(_WRAP_FMT[summ.wrap] if summ.wrap < 3 else int(fmt), length, summ.out_len, pt_bit[:n], pt_out[:n], pt_check[:n],
                       windows[: n * INDEX_WINDOW])
    return out_buf[: summ.out_len], idx, summ


CUR_HEADER, CUR_BLOCKS, CUR_TRAILER, CUR_DONE, CUR_ERROR = range(5)  # chip_inflate_cursor::phase
FMT_AUTO = 47  # CHIP_FMT_AUTO: zlib or gzip


class InflateCursor:
    """chip_inflate_cursor and its 32 KiB device window: where a slabbed decode of ONE stream stands.  A fresh one is the beginning of
    a stream of format `fmt` (-15 raw, 15 zlib, 31 gzip, 47 either wrapper).  The fields (in_total, out_total, bit, phase, wrap,
    check, hist, error) read and write the C struct `raw`; copy() is an independent cursor at the same place."""

    FIELDS = tuple(name for name, _ in _InflateCursor._fields_)

    def __init__(self, fmt=FMT_AUTO, device=None):
        import torch

        self.fmt = int(fmt)
        self.raw = _InflateCursor()
        self.window = torch.zeros(INDEX_WINDOW, dtype=torch.uint8, device=device if device is not None else "cuda")

    def __getattr__(self, name):
        if name in InflateCursor.FIELDS:
            return int(getattr(self.raw, name))
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in InflateCursor.FIELDS:
            setattr(self.raw, name, int(value))
        else:
            object.__setattr__(self, name, value)

    def copy(self):
        other = InflateCursor(self.fmt, self.window.device)
        C.memmove(C.byref(other.raw), C.byref(self.raw), C.sizeof(_InflateCursor))
        other.window.copy_(self.window)
        return other

    def __repr__(self):
        return "InflateCursor(" + ", ".join(f"{name}={getattr(self, name)}" for name in self.FIELDS) + ")"


class InflateNextSummary(_Record):
    """chip_inflate_next_summary: in_used bytes of the slab lie in front of the new cursor byte, out_len bytes were delivered, need_out
    is the size of the piece that did not fit (0: not known), n_chunks / n_starts / n_false describe the slab, status says why the
    call stopped (a DecodeStatus value, 3 = needs a dictionary, or a negative error) and path which path decoded."""

    FIELDS = _fields(_InflateNextSummary)


def inflate_parallel_next(cursor, in_buf, out_buf, chunk_bytes=0, stream=None):
    """chip_inflate_parallel_next: decode the next part of the stream `cursor` stands in.  in_buf (uint8 device tensor, any alignment;
    the bytes up to the next multiple of 4 behind it must belong to an allocation) holds the stream from byte cursor.in_total on,
    out_buf the room.  The cursor moves; the bytes are out_buf[:summary.out_len] and the next slab begins summary.in_used bytes
    further.  Synchronous on `stream`."""
    import torch

    dev = _check_tensors([(in_buf, torch.uint8), (out_buf, torch.uint8), (cursor.window, torch.uint8)])
    raw = _InflateNextSummary()
    with torch.cuda.device(dev):
        rc = lib().chip_inflate_parallel_next(cursor.fmt, C.byref(cursor.raw), _dp(cursor.window), _dp(in_buf) if in_buf.numel() else None, in_buf.numel(),
                                              _dp(out_buf) if out_buf.numel() else None, out_buf.numel(), int(chunk_bytes), C.byref(raw),
                                              _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_inflate_parallel_next failed: {rc}")
    return InflateNextSummary(raw)


class _InflateSlabs(_Slabs):
    """inflate_parallel_stream's side of _slab_stream"""

    slab_max, room_max = GZPLAN_WINDOW, 0xFFFFFFF0
    eof_text = "the source ends inside the stream"
    spare = 4

    def __init__(self, device, fmt, members, chunk_bytes):
        super().__init__(device)
        self.fmt, self.members, self.chunk_bytes = fmt, members, chunk_bytes

    def new_cursor(self, fmt=None):
        return InflateCursor(self.fmt if fmt is None else fmt, self.dev)

    def alloc_in(self, n, slab):  # zero-initialised, 4 spare bytes behind the slab
        import torch

        return torch.zeros(max(slab, n) + 4, dtype=torch.uint8, device=self.dev)

    def step(self, cur, d_in, d_out):
        return inflate_parallel_next(cur, d_in, d_out, self.chunk_bytes)

    def grow_room(self, room, need_out):
        if room >= 0xFFFFFFF0:
            raise DecodeError(-5)  # a piece beyond a call's room
        return max(2 * room, need_out)

    def after_finished(self, cur, pending, fill):
        """members=True behind a gzip member: a new gzip cursor when 1f 8b follows; else None"""
        if self.members and cur.wrap == 2:
            fill(2)  # (two bytes decide; a short read is not the end)
            if bytes(pending[:2]) == b"\x1f\x8b":
                return self.new_cursor(31)
        return None


def inflate_parallel_stream(source, sink=None, slab_bytes=64 << 20, out_bytes=256 << 20, chunk_bytes=0, members=False, fmt=FMT_AUTO, device=None):
    """One gzip / zlib / raw deflate stream of ANY length through inflate_parallel_next: `source` (bytes-like, or a binary file object)
    is uploaded slab after slab, every call's bytes are downloaded and written to `sink` (a binary file object; None: they are
    returned as bytes).  The slab doubles when a call finds no whole step in it, the room doubles (or goes to need_out) when the
    next piece does not fit.  members=True: behind a finished gzip member a new one is begun while 1f 8b follows, as gzip -d does.
    Raises DecodeError(code) on an error in the stream and EOFError when the source ends inside the stream.  Returns the bytes, or
    with a sink the number of bytes written."""
    return _slab_stream(_InflateSlabs(device, fmt, members, chunk_bytes), source, sink, slab_bytes, out_bytes)


# ---- tar archives (include/compu_hip.h, "tar archives") ---------------------------------------------


class TarStatus(enum.IntEnum):
    Ok = 0
    Truncated = 1
    BadHeader = 2
    Unsupported = 3


TAR_EXT_MAX, TAR_EXT_BYTES = 16, 1 << 20  # CHIP_TAR_EXT_MAX, CHIP_TAR_EXT_BYTES
TARF_NAME_GNU, TARF_NAME_PAX, TARF_LINK_GNU, TARF_LINK_PAX, TARF_SIZE_PAX, TARF_SIZE_BASE256 = 1, 2, 4, 8, 16, 32  # CHIP_TARF_*


def tar_entry_dtype():
    """chip_tar_entry as a numpy record: group_off, header_off, data_off, size, name_off, link_off, mtime, name_len, link_len, mode,
    prefix_len, typeflag, flags."""
    import numpy as np

    dt = np.dtype(_TarEntry)
    assert dt.itemsize == 72
    return dt


class TarPlanSummary(_Summary):
    """chip_tar_plan_summary: n_entries (members), n_global (global pax headers stepped over) and total_size (the members' sizes) of
    the whole walk, stop_off (the group or position where the walk stopped), bad_off (the offending header), status, zero_blocks
    (the all-zero blocks seen at the stop: 0, 1 or 2)."""

    __slots__ = FIELDS = _fields(_TarPlanSummary)
    ENUMS = {"status": TarStatus}


def tar_plan_host(data, max_entries=None):
    """chip_tar_plan_host over bytes / a uint8 numpy array in host memory holding a tar image: (entries, summary), entries a numpy
    record array (tar_entry_dtype) of the first min(n_entries, max_entries) members (None = all of them: one call to count, one to
    fill).  Nothing is copied or decoded: the records say where content and names lie in the image."""
    return _plan_host("chip_tar_plan_host", _TarPlanSummary, TarPlanSummary, "n_entries", data, max_entries, _record_array(tar_entry_dtype()))


def tar_plan(in_buf, length, stream=None, max_entries=None):
    """chip_tar_plan over a uint8 device tensor holding a tar image of `length` bytes (4-byte aligned, padded to a multiple of 4):
    (entries, summary), entries a uint8 device tensor of shape (k, 72) holding the chip_tar_entry records of the first
    k = min(n_entries, max_entries) members (`.cpu().numpy().view(tar_entry_dtype())` reads them).  Synchronous on `stream`.
    max_entries None: all of them (one call to count, one to fill)."""
    return _plan_device("chip_tar_plan", _TarPlanSummary, TarPlanSummary, "n_entries", in_buf, length, stream, max_entries, _record_rows(_TarEntry))


def tar_names(entries, source, stream=None):
    """The full names of a plan's members, as a list of bytes (prefix + b"/" + name where the header has a prefix): `entries` the
    records (the numpy record array of tar_plan_host, or the device tensor of tar_plan, which is copied to the host), `source` the
    tar image as host bytes, or the uint8 device tensor it lies in: the prefix and name bytes of all members then come over in ONE
    packed copy (chip_pack_units), not in a copy per member."""
    import numpy as np

    if not isinstance(entries, np.ndarray):
        entries = entries.cpu().numpy().reshape(-1).view(tar_entry_dtype())
    n = len(entries)
    pre_off = entries["header_off"].astype(np.int64) + 345
    pre_len, name_off, name_len = entries["prefix_len"].astype(np.int64), entries["name_off"].astype(np.int64), entries["name_len"].astype(np.int64)
    if isinstance(source, (bytes, bytearray, memoryview, np.ndarray)):
        image = bytes(source)
        pick = lambda off, ln: image[off:off + ln]  # noqa: E731
        pre = [pick(int(o), int(k)) for o, k in zip(pre_off, pre_len)]
        name = [pick(int(o), int(k)) for o, k in zip(name_off, name_len)]
    else:
        import torch

        # unit 2 i is member i's prefix, unit 2 i + 1 its name
        off, ln = np.empty(2 * n, np.int64), np.empty(2 * n, np.int64)
        off[0::2], off[1::2], ln[0::2], ln[1::2] = pre_off, name_off, pre_len, name_len
        d_off = torch.from_numpy(off).to(source.device)
        d_len = torch.from_numpy(ln.astype(np.int32)).to(source.device)
        packed, _, total = pack_units(source, d_off, d_len, stream=stream)
        flat = packed.cpu().numpy().tobytes()
        at = np.concatenate(([0], np.cumsum(ln)))
        assert int(at[-1]) == total == len(flat)
        pre = [flat[at[2 * i]:at[2 * i + 1]] for i in range(n)]
        name = [flat[at[2 * i + 1]:at[2 * i + 2]] for i in range(n)]
    return [p + b"/" + m if p else m for p, m in zip(pre, name)]


class TarArchive:
    """A tar archive in device memory, planned: `content` the tar image (a uint8 device tensor), `entries` the members' records on
    the host (tar_entry_dtype), `summary` the plan's, `names` the members' full names (bytes)."""

    def __init__(self, content, entries, summary, names):
        self.content, self.entries, self.summary, self.names = content, entries, summary, names
        self._index = {name: i for i, name in enumerate(names)}  # a repeated name: its last member, as tarfile.extract resolves it

    def __len__(self):
        return len(self.entries)

    def member(self, index_or_name):
        """The content of one member, content[data_off : data_off + size], as a zero-copy uint8 view.  A name (str, matched as UTF-8,
        or bytes) resolves to the LAST member of that name; KeyError for an unknown one, IndexError for an index out of range."""
        if isinstance(index_or_name, (str, bytes, bytearray)):
            i = self._index[index_or_name.encode("utf-8") if isinstance(index_or_name, str) else bytes(index_or_name)]
        else:
            i = int(index_or_name)
            if not 0 <= i < len(self.entries):
                raise IndexError(f"member {i} of {len(self.entries)}")
        e = self.entries[i]
        return self.content[int(e["data_off"]):int(e["data_off"]) + int(e["size"])]


def tar_open(in_buf, length, fmt=None, stream=None):
    """A .tar, .tar.gz or .tar.zst in device memory (in_buf a uint8 device tensor holding its `length` bytes, 4-byte aligned and
    padded to a multiple of 4) as a TarArchive: decoded on the device where it is compressed, planned by chip_tar_plan, the names
    fetched in one packed copy.  fmt None sniffs the first bytes (chip_detect): gzip and zlib go through inflate_parallel, zstd
    through zstd_parallel, anything else is taken as a plain tar image (which then stays in in_buf: no copy).  A zlib verdict rests
    on two bytes, which a plain tar's first member name can spell ("XG", "HK", "x^"): it is trusted only when bytes 257..261 are not
    `ustar`.  A .tar.lz4 is known by the LZ4 frame magic (the sniff is made here: chip_detect knows no LZ4) and goes through
    lz4_parallel: its first frame is the archive.  fmt may also be given, and is then not questioned: Detection.Gzip / Zlib / Zstd /
    Unknown (= plain), or the string "lz4".
    Limits are those of the one-shot decodes: a gzip / zlib stream of at most 2^29 - 64 bytes that decodes to at most 2^32 - 16; a
    zstd frame of at most 2^32 - 1 bytes, below 2^31 decoded bytes on the parallel path and within a unit (2^28 input bytes) on the
    serial one.  A larger archive belongs to the slab loops (inflate_parallel_stream, zstd_parallel_stream).
    Raises ValueError when the decode does not finish (the message carries its status and in_used) or when the plan's status is
    not Ok (the message carries the status, stop_off and bad_off).  Waits for the result."""
    length = int(length)
    if fmt is None:
        head = in_buf[:min(length, 262)].cpu().numpy().tobytes()
        fmt = Detection.detect(head[:4])
        if fmt == Detection.Zlib and head[257:262] == b"ustar":
            fmt = Detection.Unknown  # a member name that begins like a zlib header ("XGBoost-1.0/": 58 47), not a zlib stream
        if head[:4] == LZ4_MAGIC.to_bytes(4, "little"):
            fmt = "lz4"  # (chip_detect knows no LZ4: the sniff is made here; no member name begins with 04 22 4d 18)
    content, n = in_buf, length
    if fmt == "lz4":
        content, s = lz4_parallel(in_buf, length, stream=stream)
        if s.status != int(DecodeStatus.Finished):
            raise ValueError(f"tar_open: the LZ4 frame did not finish: status {s.status} at input byte {s.in_used}")
        n = s.out_len
    elif fmt in (Detection.Gzip, Detection.Zlib):
        content, s = inflate_parallel(ZlibMode.Gzip if fmt == Detection.Gzip else ZlibMode.Zlib, in_buf, length, stream=stream)
        if s.status != int(DecodeStatus.Finished):
            raise ValueError(f"tar_open: the {Detection(fmt).name} stream did not finish: status {s.status} at input byte {s.in_used}")
        n = s.out_len
    elif fmt == Detection.Zstd:
        content, s = zstd_parallel(in_buf, length, stream=stream)
        if s.status != int(DecodeStatus.Finished):
            raise ValueError(f"tar_open: the zstd frame did not finish: status {s.status} at input byte {s.in_used}")
        n = s.out_len
    entries, summ = tar_plan(content, n, stream=stream)
    if summ.status != TarStatus.Ok:
        raise ValueError(f"tar_open: not a tar image this library reads: status {summ.status.name} at stop_off {summ.stop_off} "
                         f"(bad_off {summ.bad_off}); {summ!r}")
    host = entries.cpu().numpy().reshape(-1).view(tar_entry_dtype())
    return TarArchive(content[:n], host, summ, tar_names(host, content, stream=stream))


# ---- tar archives: writing (include/compu_hip.h, "tar archives: writing") ----------------------------


class TarWriteStatus(enum.IntEnum):
    Ok = 0
    NeedOutput = 1
    BadSource = 2


TW_GNU, TW_FORCE_EXT = 1, 2  # CHIP_TW_GNU (L / K headers and base-256 sizes instead of pax records), CHIP_TW_FORCE_EXT (every size goes the long way)
TARW_NAME_MAX = 65535        # CHIP_TARW_NAME_MAX


def tar_source_dtype():
    """chip_tar_source as a numpy record: data_off, size, name_off, link_off, mtime, name_len, link_len, mode, uid, gid, typeflag
    (the character's code, ord("0") for a file), pad (three bytes, 0)."""
    import numpy as np

    dt = np.dtype(_TarSource)
    assert dt.itemsize == 64
    return dt


class TarWriteSummary(_Summary):
    """chip_tar_write_summary: n_entries, n_ext (extension headers written), out_len (the whole image; the exact room to come back
    with on NeedOutput), end_off (where the two zero blocks start), total_size (the sum of the sizes), bad_index (the lowest bad
    record on BadSource), status."""

    __slots__ = FIELDS = _fields(_TarWriteSummary)
    ENUMS = {"status": TarWriteStatus}


_TAR_ARCHIVE = (_TarWriteSummary, TarWriteSummary, _TarEntry, TarWriteStatus)  # for _archive_host_call / _archive_device_call


def tar_write_bound(n, names_total, content_total, record_bytes=0):
    """chip_tar_write_bound: the room that is always enough for n members with names_total bytes of names and link names and
    content_total bytes of content; 0 when it overflows 64 bits or record_bytes is refused."""
    return int(lib().chip_tar_write_bound(int(n), int(names_total), int(content_total), int(record_bytes)))


def tar_write_host(sources, names, content, flags=0, record_bytes=0, out_cap=None, content_len=None):
    """chip_tar_write_host: `sources` a numpy record array (tar_source_dtype), names / content bytes or uint8 arrays.  out_cap None:
    one call for the size, one to write.  content_len overrides len(content) for a call that only sizes (out_cap smaller than the
    image: the content is never read).  Returns (the image as bytes -- b"" unless status is Ok --, entries as a numpy record array
    of tar_entry_dtype, TarWriteSummary)."""
    import numpy as np

    u8 = lambda b: np.ascontiguousarray(b, dtype=np.uint8) if isinstance(b, np.ndarray) else np.frombuffer(bytes(b), np.uint8)  # noqa: E731
    src = np.ascontiguousarray(sources, dtype=tar_source_dtype())
    n = src.size
    names, content = u8(names), u8(content)
    clen = content.size if content_len is None else int(content_len)

    def call(out, cap, ent, raw):
        return lib().chip_tar_write_host(n, _np_ptr(src), _np_ptr(names), names.size, content.ctypes.data_as(C.c_void_p) if clen else None, clen,
                                         flags, record_bytes, out, cap, ent, raw)

    return _archive_host_call("chip_tar_write_host", _TAR_ARCHIVE, call, n, out_cap)


def tar_write(sources, names, content, flags=0, record_bytes=0, out=None, stream=None):
    """chip_tar_write on device tensors: sources uint8 of shape (n, 64) holding chip_tar_source records
    (`torch.from_numpy(records.view(np.uint8).reshape(-1, 64)).cuda()`), names / content uint8.  out None: the exact room is allocated
    after a sizing call; else a uint8 tensor, and too little room is status NeedOutput with nothing written.  Returns (the image: a
    view of `out`, empty unless status is Ok; entries: uint8 of shape (n, 72), what tar_plan would answer; TarWriteSummary).
    Synchronous on `stream`."""
    import torch

    pairs = [(sources, torch.uint8), (names, torch.uint8), (content, torch.uint8)] + ([(out, torch.uint8)] if out is not None else [])
    dev = _check_tensors(pairs)
    n = sources.numel() // C.sizeof(_TarSource)
    if sources.numel() != n * C.sizeof(_TarSource):
        raise ValueError("sources holds 64-byte records")
    q = lambda t: _dp(t) if t.numel() else None  # noqa: E731

    def call(o, cap, ent, raw, sp):
        return lib().chip_tar_write(n, q(sources), q(names), names.numel(), q(content), content.numel(), flags, record_bytes, o, cap, ent, raw, sp)

    return _archive_device_call("chip_tar_write", _TAR_ARCHIVE, call, n, dev, out, stream)


def tar_write_items(items, flags=0, stream=None, device=None):
    """A tar image of (name, content[, mode, mtime]) items on the device, the counterpart of zip_write_items.  name: str (encoded as
    UTF-8) or bytes, a name that ends in "/" is a directory (typeflag 5, its content must be empty); content: bytes-like, or a uint8
    device tensor; mode defaults to 0644 (0755 for a directory), mtime to 0.  The contents land at 16-byte aligned offsets of one
    device buffer.  Returns (the image as a uint8 device tensor, entries, TarWriteSummary) as tar_write does; tar_open reads it back."""
    import numpy as np

    items = [tuple(it) for it in items]
    src = np.zeros(len(items), tar_source_dtype())
    names, at = bytearray(), 0
    for i, it in enumerate(items):
        name, c = it[0], it[1]
        if isinstance(name, str):
            name = name.encode("utf-8")
        if not 1 <= len(name) <= TARW_NAME_MAX:
            raise ValueError("a name has 1 to 65535 bytes")
        size = _item_size(c)
        is_dir = name.endswith(b"/")
        if is_dir and size:
            raise ValueError("a directory has no content")
        mode = int(it[2]) if len(it) > 2 and it[2] is not None else (0o755 if is_dir else 0o644)
        mtime = int(it[3]) if len(it) > 3 and it[3] is not None else 0
        src[i] = (at, size, len(names), 0, mtime, len(name), 0, mode, 0, 0, ord("5") if is_dir else ord("0"), (0, 0, 0))
        names += name
        at += (size + 15) // 16 * 16
    d_src, d_names, content = _upload_items(src, names, [it[1] for it in items], at, device)
    return tar_write(d_src, d_names, content, flags=flags, stream=stream)


# ---- LZ4: blocks and frames (include/compu_hip.h, "LZ4: blocks and frames" and "LZ4: encoding") --------


LZ4_E_HEADER, LZ4_E_DICT, LZ4_E_BLOCK_SIZE, LZ4_E_BLOCK = -200, -201, -202, -203  # CHIP_LZ4_E_*
LZ4_E_OFFSET, LZ4_E_BLOCK_CHECKSUM, LZ4_E_CONTENT_SIZE, LZ4_E_CONTENT_CHECKSUM = -204, -205, -206, -207
LZ4BLOCKS_UNSIZED = 0xFFFFFFFFFFFFFFFF  # CHIP_LZ4BLOCKS_UNSIZED: content_size of a frame without C.Size
LZ4BLOCK_STORED, LZ4BLOCK_LAST = 1, 2  # chip_lz4_block.flags
LZ4PAR_SERIAL, LZ4PAR_PARALLEL, LZ4PAR_REFUSED = 0, 1, 2  # chip_lz4_parallel_summary.path
LZ4PAR_NO_CHECKSUM = 1  # CHIP_LZ4PAR_NO_CHECKSUM
LZ4_MAGIC = 0x184D2204


def lz4_block_dtype():
    """chip_lz4_block as a numpy record: offset (of the 4-byte block header), size, flags (LZ4BLOCK_*), checksum."""
    import numpy as np

    dt = np.dtype(_Lz4Block)
    assert dt.itemsize == 24
    return dt


class Lz4BlocksSummary(_Summary):
    """chip_lz4_blocks_summary: n_blocks the walk counted, in_used (the frame's end, 0 when the walk stopped early), content_size
    (LZ4BLOCKS_UNSIZED without C.Size), block_max, the FLG and BD bytes, the header's length, the stored content checksum, status."""

    __slots__ = FIELDS = _fields(_Lz4BlocksSummary)
    ENUMS, FORMATS = {"status": ZstdPlanStatus}, {"flg": "#x", "bd": "#x", "content_checksum": "#x"}


def lz4_block_decode_host(data, out_cap):
    """chip_lz4_block_decode_host: one raw LZ4 block (bytes-like) decoded on the host into out_cap bytes of room: (out bytes --
    the first out_len --, in_used, status).  The definition of the block rules."""
    import numpy as np

    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(int(out_cap), np.uint8)
    ol, iu = C.c_uint64(0), C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    st = lib().chip_lz4_block_decode_host(p(buf), buf.size, p(out), out.size, C.byref(ol), C.byref(iu))
    if st == -101:
        raise ValueError("chip_lz4_block_decode_host refused its arguments")
    return out[:ol.value].tobytes(), int(iu.value), int(st)


def lz4_blocks_host(data, max_blocks=None):
    """chip_lz4_blocks_host over bytes / a uint8 numpy array in host memory: (blocks, summary) of the FIRST frame -- blocks a numpy
    record array (lz4_block_dtype) of the first min(n_blocks, max_blocks) blocks (None = all of them: one call to count, one to
    fill).  Read from headers alone; nothing is decoded."""
    return _plan_host("chip_lz4_blocks_host", _Lz4BlocksSummary, Lz4BlocksSummary, "n_blocks", data, max_blocks, _record_array(lz4_block_dtype()))


def lz4_blocks(in_buf, length, stream=None, max_blocks=None):
    """chip_lz4_blocks over a uint8 device tensor holding `length` bytes that begin with an LZ4 frame (4-byte aligned, padded to a
    multiple of 4): (blocks, summary), blocks a uint8 device tensor of shape (k, 24) holding the chip_lz4_block records of the first
    k = min(n_blocks, max_blocks) blocks (`.cpu().numpy().view(lz4_block_dtype())` reads them).  Synchronous on `stream`.
    max_blocks None: all of them (one call to count, one to fill)."""
    return _plan_device("chip_lz4_blocks", _Lz4BlocksSummary, Lz4BlocksSummary, "n_blocks", in_buf, length, stream, max_blocks,
                        _record_rows(_Lz4Block, "zeros"))


def xxh32_batch(buf, off, length, seed=0, stream=None):
    """chip_xxh32_batch on device tensors: XXH32 with `seed` of buf[off[i] : off[i] + length[i]] for every i.  buf uint8, off int64
    (read as u64), length int32 (read as u32).  Returns an int32 device tensor (read it as u32).  One wave per range.  Only
    enqueues on `stream`."""
    import torch

    dev = _check_tensors(((buf, torch.uint8), (off, torch.int64), (length, torch.int32)))
    n = off.numel()
    if length.numel() != n:
        raise ValueError("off and length must have one length")
    digest = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return digest
    with torch.cuda.device(dev):
        rc = lib().chip_xxh32_batch(n, _dp(buf), _dp(off), _dp(length), int(seed) & 0xFFFFFFFF, _dp(digest), _stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_xxh32_batch failed: {rc}")
    return digest


class Lz4ParallelSummary(_Summary):
    """chip_lz4_parallel_summary: n_blocks of the frame, out_len, in_used, total_out (the size to come back with on NeedOutput),
    status, path (LZ4PAR_*), check (the content checksum computed on the parallel path)."""

    __slots__ = FIELDS = _fields(_Lz4ParallelSummary)
    FORMATS = {"check": "#x"}


def lz4_parallel(in_buf, length, out_buf=None, checksum=True, stream=None):
    """chip_lz4_parallel over a uint8 device tensor holding `length` bytes that begin with ONE LZ4 frame (4-byte aligned, padded to a
    multiple of 4): (out, summary).  With `out_buf` (a uint8 device tensor) the content goes there and `out` is its first out_len
    bytes.  Without, the call is made with no room first, then with a new tensor of total_out bytes; a frame that takes the serial
    path states no size that way, so it is sized by decode_batch_sizes as one unit and decoded with that room -- a frame that is
    refused, or in error, comes back as the empty tensor and its summary.  checksum=False waives the comparison of the content
    checksum on the parallel path.  Synchronous on `stream`."""
    import torch

    dev = _check_tensors(((in_buf, torch.uint8),) + (((out_buf, torch.uint8),) if out_buf is not None else ()))
    length = int(length)
    if length < 0 or length > in_buf.numel():
        raise ValueError(f"length {length} outside the buffer of {in_buf.numel()} bytes")
    raw = _Lz4ParallelSummary()
    flags = 0 if checksum else LZ4PAR_NO_CHECKSUM
    base, sp = (_dp(in_buf) if length else None), _stream_ptr(stream)

    def call(out):
        cap = out.numel() if out is not None else 0
        rc = lib().chip_lz4_parallel(base, length, _dp(out) if cap else None, cap, flags, C.byref(raw), sp)
        if rc != 0:
            raise RuntimeError(f"chip_lz4_parallel failed: {rc}")

    with torch.cuda.device(dev):
        if out_buf is None:
            call(None)
            need = int(raw.total_out) if raw.status == int(DecodeStatus.NeedOutput) and raw.path == LZ4PAR_PARALLEL else 0
            if raw.status == int(DecodeStatus.NeedOutput) and raw.path == LZ4PAR_SERIAL and length <= 0xFFFFFFFF:
                one = lambda v, dt: torch.tensor([v], dtype=torch.int64, device=dev).to(dt)  # noqa: E731
                size, _, st = decode_batch_sizes(FMT_LZ4, in_buf, one(0, torch.int64), one(length, torch.int32), stream=stream)
                need = int(size[0]) if int(st[0]) == int(DecodeStatus.Finished) and int(size[0]) <= 0xFFFFFFFF else 0
            out_buf = torch.empty(need, dtype=torch.uint8, device=dev)
            if need:
                call(out_buf)
        else:
            call(out_buf)
    return out_buf[:int(raw.out_len)], Lz4ParallelSummary(raw)


def lz4_decode(data, checksum=True, device=None, stream=None):
    """The contents of a whole .lz4 file (bytes-like): concatenated frames are decoded one behind the other, each by lz4_parallel,
    and skippable frames (magic 0x184D2A50 .. 5F, a 4-byte length) are stepped over on the host.  Returns a uint8 device tensor.
    Raises ValueError where a frame does not finish (the message carries its offset, status and in_used), where bytes that are
    no frame follow a frame, and on a legacy frame (magic 0x184C2102), which this library does not read.  Waits for the result."""
    import numpy as np
    import torch

    data = bytes(data)
    dev = torch.device("cuda" if device is None else device)
    parts, p, n = [], 0, len(data)
    while p < n:
        if n - p < 4:
            raise ValueError(f"lz4_decode: {n - p} stray bytes at offset {p}")
        magic = int.from_bytes(data[p:p + 4], "little")
        if 0x184D2A50 <= magic <= 0x184D2A5F:
            if n - p < 8:
                raise ValueError(f"lz4_decode: a skippable frame is cut off at offset {p}")
            size = int.from_bytes(data[p + 4:p + 8], "little")
            if n - p - 8 < size:
                raise ValueError(f"lz4_decode: a skippable frame is cut off at offset {p}")
            p += 8 + size
            continue
        if magic != LZ4_MAGIC:
            raise ValueError(f"lz4_decode: no LZ4 frame at offset {p} (magic {magic:#010x})")
        rest = np.frombuffer(data, np.uint8, offset=p)
        _, walk = lz4_blocks_host(rest, 0)  # the frame's own bytes go up, where its headers say how many they are
        if walk.status == ZstdPlanStatus.Ok:
            rest = rest[:walk.in_used]
        padded = np.zeros((rest.size + 3) // 4 * 4, np.uint8)
        padded[:rest.size] = rest
        d_in = torch.from_numpy(padded).to(dev)
        out, s = lz4_parallel(d_in, rest.size, checksum=checksum, stream=stream)
        if s.status != int(DecodeStatus.Finished):
            raise ValueError(f"lz4_decode: the frame at offset {p} did not finish: status {s.status} at input byte {s.in_used}")
        parts.append(out)
        p += s.in_used
    if not parts:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    return parts[0] if len(parts) == 1 else torch.cat(parts)


# ---- LZ4: encoding (include/compu_hip.h, "LZ4: encoding") -------------------------------------------------

LZ4_S_BLOCK_CHECKSUM, LZ4_S_NO_CONTENT_CHECKSUM, LZ4_S_BLOCK_ID_SHIFT = 1, 2, 4  # CHIP_LZ4_S_*: encode_batch's strategy for FMT_LZ4
W_LZ4_CONTENT_CHECKSUM, W_LZ4_BLOCK_CHECKSUM = 2, 4  # CHIP_W_LZ4_*: encode_file's flags for FMT_LZ4


def _lz4_encode_host(what, call, data, out_cap, bound_fmt):
    import numpy as np

    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = int(lib().chip_encode_bound(bound_fmt, buf.size)) if out_cap is None else int(out_cap)
    out = np.zeros(cap, np.uint8)
    ol = C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    st = call(p(buf), buf.size, p(out), out.size, C.byref(ol))
    if st == -101:
        raise ValueError(f"{what} refused its arguments")
    return out[:ol.value].tobytes(), int(st)


def lz4_block_encode_host(data, level=1, out_cap=None):
    """chip_lz4_block_encode_host: bytes-like -> (one raw LZ4 block, status) with out_cap bytes of room (None: encode_bound).  The
    definition of the bytes the kernel writes.  status EncodeStatus.Finished, or NeedOutput / Error with an empty block."""
    call = lambda i, n, o, c, ol: lib().chip_lz4_block_encode_host(i, n, int(level), o, c, ol)  # noqa: E731
    return _lz4_encode_host("chip_lz4_block_encode_host", call, data, out_cap, FMT_LZ4_BLOCK)


def lz4_frame_encode_host(data, level=1, strategy=0, out_cap=None):
    """chip_lz4_frame_encode_host: bytes-like -> (one LZ4 frame, status); strategy carries the LZ4_S_* option bits."""
    call = lambda i, n, o, c, ol: lib().chip_lz4_frame_encode_host(i, n, int(level), int(strategy), o, c, ol)  # noqa: E731
    return _lz4_encode_host("chip_lz4_frame_encode_host", call, data, out_cap, FMT_LZ4)


def lz4_encode(data, level=1, block_bytes=0, content_checksum=False, block_checksum=False, device=None, stream=None):
    """A whole .lz4 file (bytes) of `data` (bytes-like or a uint8 device tensor): ONE frame with a block per block_bytes (0 = 65536,
    or 65536, 262144, 1048576, 4194304) through encode_file(FMT_LZ4, ..), every block encoded by its own wave.  What the `lz4`
    command writes and lz4_decode / lz4_parallel read back.  Waits for the result."""
    import numpy as np
    import torch

    if isinstance(data, torch.Tensor):
        d_in, length = data, data.numel()
    else:
        raw = np.frombuffer(bytes(data), np.uint8)
        length = raw.size
        padded = np.zeros((length + 3) // 4 * 4, np.uint8)
        padded[:length] = raw
        d_in = torch.from_numpy(padded).to(torch.device("cuda" if device is None else device))
    flags = (W_LZ4_CONTENT_CHECKSUM if content_checksum else 0) | (W_LZ4_BLOCK_CHECKSUM if block_checksum else 0)
    out, _ = encode_file(FMT_LZ4, level, d_in, length, unit_bytes=block_bytes, flags=flags, stream=stream)
    return out.cpu().numpy().tobytes()
