"""Two CPU decoders for zstd frames that tests check an encoder's output with: the system libzstd (streaming, optionally under a
windowLogMax) and the oracle."""
import ctypes as C

import numpy as np

import zstd_ref

ZSTD_d_windowLogMax = 100


def _z():
    z = zstd_ref.load()
    assert z is not None, "the system libzstd is needed to cross-check the frames"
    z.ZSTD_DCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    z.ZSTD_getErrorName.restype = C.c_char_p
    z.ZSTD_getErrorName.argtypes = [C.c_size_t]
    return z


def zdec(comp, out_cap, window_log_max=None, complete=True):
    """libzstd streaming decode of `comp` (one frame); with complete=False the frame may stop at a flush point."""
    z = _z()
    ds = z.ZSTD_createDStream()
    try:
        if window_log_max is not None:
            assert not z.ZSTD_isError(z.ZSTD_DCtx_setParameter(ds, ZSTD_d_windowLogMax, window_log_max))
        src = C.create_string_buffer(bytes(comp), max(len(comp), 1))
        dst = C.create_string_buffer(max(out_cap, 1))
        ib = zstd_ref._Buf(C.cast(src, C.c_void_p), len(comp), 0)
        ob = zstd_ref._Buf(C.cast(dst, C.c_void_p), out_cap, 0)
        while True:
            ret = z.ZSTD_decompressStream(ds, C.byref(ob), C.byref(ib))
            assert not z.ZSTD_isError(ret), z.ZSTD_getErrorName(ret)
            if ret == 0 or ib.pos == ib.size:
                break
        if complete:
            assert ret == 0, "frame not complete"
        return dst.raw[: ob.pos]
    finally:
        z.ZSTD_freeDStream(ds)


def oracle_decode(frames, sizes):
    from oracle import oracle as O

    n = len(frames)
    in_len = np.array([len(f) for f in frames], np.uint32)
    in_off = np.zeros(n, np.uint64)
    in_off[1:] = np.cumsum(in_len.astype(np.uint64))[:-1]
    buf = np.frombuffer(b"".join(frames) + b"\0", np.uint8)
    caps = np.array([max(s, 1) for s in sizes], np.uint32)
    out_off = np.zeros(n, np.uint64)
    out_off[1:] = np.cumsum(caps.astype(np.uint64))[:-1]
    out, ol, st, _bad = O.zstd_units(buf, in_off, in_len, int(caps.sum()), out_off, caps, threads=8)
    return [bytes(out[out_off[i] : out_off[i] + ol[i]]) if st[i] == 2 else None for i in range(n)]
