"""The system's libbrotlienc / libbrotlidec through ctypes: the cross-check of the GPU brotli decoder (as zstd_ref.py is for
libzstd).  Streams are written here, verdicts are libbrotlidec's BrotliDecoderDecompressStream."""
import ctypes as C

_enc = _dec = None

# BrotliEncoderParameter
P_MODE, P_QUALITY, P_LGWIN = 0, 1, 2
MODE_GENERIC, MODE_TEXT, MODE_FONT = 0, 1, 2
OP_PROCESS, OP_FLUSH, OP_FINISH = 0, 1, 2
# BrotliDecoderResult
R_ERROR, R_SUCCESS, R_NEEDS_MORE_INPUT, R_NEEDS_MORE_OUTPUT = 0, 1, 2, 3
# the per-unit statuses of compu_hip.h
NEED_INPUT, NEED_OUTPUT, FINISHED = 0, 1, 2


def libs():
    global _enc, _dec
    if _dec is None:
        _enc = C.CDLL("libbrotlienc.so.1")
        _dec = C.CDLL("libbrotlidec.so.1")
        _enc.BrotliEncoderCreateInstance.restype = C.c_void_p
        _enc.BrotliEncoderCreateInstance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _enc.BrotliEncoderSetParameter.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
        _enc.BrotliEncoderCompressStream.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.c_void_p]
        _enc.BrotliEncoderHasMoreOutput.argtypes = [C.c_void_p]
        _enc.BrotliEncoderDestroyInstance.argtypes = [C.c_void_p]
        _dec.BrotliDecoderCreateInstance.restype = C.c_void_p
        _dec.BrotliDecoderCreateInstance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _dec.BrotliDecoderDecompressStream.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                                       C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.c_void_p]
        _dec.BrotliDecoderGetErrorCode.argtypes = [C.c_void_p]
        _dec.BrotliDecoderDestroyInstance.argtypes = [C.c_void_p]
        _dec.BrotliDecoderErrorString.restype = C.c_char_p
        _dec.BrotliDecoderErrorString.argtypes = [C.c_int]
    return _enc, _dec


def compress(data, quality=5, lgwin=22, mode=MODE_GENERIC, flush_every=0):
    """One brotli stream of `data`; flush_every > 0 emits a flush (an empty metablock boundary) every that many bytes."""
    enc, _ = libs()
    s = enc.BrotliEncoderCreateInstance(None, None, None)
    enc.BrotliEncoderSetParameter(s, P_QUALITY, quality)
    enc.BrotliEncoderSetParameter(s, P_LGWIN, lgwin)
    enc.BrotliEncoderSetParameter(s, P_MODE, mode)
    out = bytearray()
    buf = C.create_string_buffer(1 << 16)
    step = flush_every if flush_every > 0 else max(1, len(data))
    pieces = [data[i:i + step] for i in range(0, len(data), step)] or [b""]
    try:
        for k, piece in enumerate(pieces):
            op = OP_FINISH if k == len(pieces) - 1 else OP_FLUSH
            src = C.create_string_buffer(bytes(piece), len(piece) + 1)
            avail_in = C.c_size_t(len(piece))
            next_in = C.c_void_p(C.addressof(src))
            while True:
                avail_out = C.c_size_t(len(buf))
                next_out = C.c_void_p(C.addressof(buf))
                if not enc.BrotliEncoderCompressStream(s, op, C.byref(avail_in), C.byref(next_in), C.byref(avail_out),
                                                       C.byref(next_out), None):
                    raise RuntimeError("BrotliEncoderCompressStream failed")
                out += buf.raw[: len(buf) - avail_out.value]
                if avail_in.value == 0 and not enc.BrotliEncoderHasMoreOutput(s):
                    break
    finally:
        enc.BrotliEncoderDestroyInstance(s)
    return bytes(out)


def decode(data, cap):
    """libbrotlidec over the whole input with `cap` bytes of output: (status, output, in_used, err) in the terms of
    compu_hip.h -- status FINISHED / NEED_INPUT / NEED_OUTPUT or the negative error code."""
    _, dec = libs()
    s = dec.BrotliDecoderCreateInstance(None, None, None)
    try:
        src = C.create_string_buffer(bytes(data), len(data) + 1)
        dst = C.create_string_buffer(cap + 1)
        avail_in = C.c_size_t(len(data))
        next_in = C.c_void_p(C.addressof(src))
        avail_out = C.c_size_t(cap)
        next_out = C.c_void_p(C.addressof(dst))
        r = dec.BrotliDecoderDecompressStream(s, C.byref(avail_in), C.byref(next_in), C.byref(avail_out), C.byref(next_out), None)
        out = dst.raw[: cap - avail_out.value]
        used = len(data) - avail_in.value
        if r == R_ERROR:
            return dec.BrotliDecoderGetErrorCode(s), out, used
        return {R_SUCCESS: FINISHED, R_NEEDS_MORE_INPUT: NEED_INPUT, R_NEEDS_MORE_OUTPUT: NEED_OUTPUT}[r], out, used
    finally:
        dec.BrotliDecoderDestroyInstance(s)


def error_string(code):
    _, dec = libs()
    return dec.BrotliDecoderErrorString(code).decode()


def stream_calls(data, cap, max_calls=100000):
    """compu's loop over BrotliDecoderDecompressStream (src/decoder/brotli_c.rs:43-60): each call gets the input the last one
    left and `cap` bytes of output.  Returns the list of (status, output bytes, input_remain) per call, up to Finished or an
    error."""
    _, dec = libs()
    s = dec.BrotliDecoderCreateInstance(None, None, None)
    calls = []
    try:
        src = C.create_string_buffer(bytes(data), len(data) + 1)
        rest = len(data)
        dst = C.create_string_buffer(cap + 1)
        for _ in range(max_calls):
            avail_in = C.c_size_t(rest)
            next_in = C.c_void_p(C.addressof(src) + len(data) - rest)
            avail_out = C.c_size_t(cap)
            next_out = C.c_void_p(C.addressof(dst))
            r = dec.BrotliDecoderDecompressStream(s, C.byref(avail_in), C.byref(next_in), C.byref(avail_out), C.byref(next_out), None)
            rest = avail_in.value
            st = dec.BrotliDecoderGetErrorCode(s) if r == R_ERROR else {R_SUCCESS: FINISHED, R_NEEDS_MORE_INPUT: NEED_INPUT,
                                                                        R_NEEDS_MORE_OUTPUT: NEED_OUTPUT}[r]
            calls.append((st, dst.raw[: cap - avail_out.value], rest))
            if st == FINISHED or st < 0 or (st == NEED_INPUT and rest == 0):
                break
        return calls
    finally:
        dec.BrotliDecoderDestroyInstance(s)
