"""Snappy decoding (include/compu_hip.h, "Snappy: blocks and framed streams"): raw blocks and streams of the
framing format.  Reached as compu_amd.snappy; the batch calls themselves are api.decode_batch and its siblings with FMT_SNAPPY_BLOCK
/ FMT_SNAPPY.  Decode only: no encode entry point takes the tags."""
import ctypes as C

from . import api
from ._ffi import _SnappyChunk, _SnappyChunksSummary, _SnappyParallelSummary, lib
from .api import DecodeStatus, ZstdPlanStatus

FMT_SNAPPY_BLOCK = 104  # CHIP_FMT_SNAPPY_BLOCK: one raw block per unit (a varint preamble, then elements)
FMT_SNAPPY = 105  # CHIP_FMT_SNAPPY: one stream of the framing format per unit (a .sz file)
SNAPPY_E_PREAMBLE, SNAPPY_E_OFFSET, SNAPPY_E_LENGTH, SNAPPY_E_HEADER = -210, -211, -212, -213  # CHIP_SNAPPY_E_*
SNAPPY_E_CHUNK, SNAPPY_E_CHUNK_SIZE, SNAPPY_E_BLOCK, SNAPPY_E_CHECKSUM = -214, -215, -216, -217
SNAPPYPAR_SERIAL, SNAPPYPAR_PARALLEL, SNAPPYPAR_REFUSED = 0, 1, 2  # chip_snappy_parallel_summary.path
SNAPPY_IDENT = b"\xff\x06\x00\x00sNaPpY"


def snappy_chunk_dtype():
    """chip_snappy_chunk as a numpy record: offset (of the 4-byte chunk header), size (s), type (0 compressed, 1 uncompressed), crc
    (the stored, masked CRC-32C)."""
    import numpy as np

    dt = np.dtype(_SnappyChunk)
    assert dt.itemsize == 24
    return dt


class SnappyChunksSummary(api._Summary):
    """chip_snappy_chunks_summary: n_chunks (data chunks) and n_skipped the walk counted, in_used (the whole length, or the offset
    of the chunk at which the walk stopped), status."""

    __slots__ = FIELDS = api._fields(_SnappyChunksSummary)
    ENUMS = {"status": ZstdPlanStatus}


class SnappyParallelSummary(api._Summary):
    """chip_snappy_parallel_summary: n_chunks of the stream, out_len, in_used, total_out (the size to come back with on NeedOutput),
    status, path (SNAPPYPAR_*), n_skipped."""

    __slots__ = FIELDS = api._fields(_SnappyParallelSummary)


def snappy_block_decode_host(data, out_cap):
    """chip_snappy_block_decode_host: one raw block (bytes-like) decoded on the host into out_cap bytes of room: (out bytes -- the
    first out_len --, in_used, status).  The definition of the block rules."""
    import numpy as np

    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(int(out_cap), np.uint8)
    ol, iu = C.c_uint64(0), C.c_uint64(0)
    st = lib().chip_snappy_block_decode_host(api._np_ptr(buf), buf.size, api._np_ptr(out), out.size, C.byref(ol), C.byref(iu))
    if st == -101:
        raise ValueError("chip_snappy_block_decode_host refused its arguments")
    return out[:ol.value].tobytes(), int(iu.value), int(st)


def snappy_chunks_host(data, max_chunks=None):
    """chip_snappy_chunks_host over bytes / a uint8 numpy array in host memory: (chunks, summary) -- chunks a numpy record array
    (snappy_chunk_dtype) of the first min(n_chunks, max_chunks) data chunks (None = all of them: one call to count, one to fill).
    Read from the chunk headers alone; nothing is decoded."""
    return api._plan_host("chip_snappy_chunks_host", _SnappyChunksSummary, SnappyChunksSummary, "n_chunks", data, max_chunks,
                          api._record_array(snappy_chunk_dtype()))


def snappy_chunks(in_buf, length, stream=None, max_chunks=None):
    """chip_snappy_chunks over a uint8 device tensor holding `length` bytes of a framed stream (4-byte aligned, padded to a multiple
    of 4): (chunks, summary), chunks a uint8 device tensor of shape (k, 24) holding the chip_snappy_chunk records of the first
    k = min(n_chunks, max_chunks) data chunks (`.cpu().numpy().view(snappy_chunk_dtype())` reads them).  Synchronous on `stream`."""
    return api._plan_device("chip_snappy_chunks", _SnappyChunksSummary, SnappyChunksSummary, "n_chunks", in_buf, length, stream, max_chunks,
                            api._record_rows(_SnappyChunk, "zeros"))


def crc32c_batch(buf, off, length, stream=None):
    """chip_crc32c_batch on device tensors: the CRC-32C (Castagnoli), UNMASKED, of buf[off[i] : off[i] + length[i]] for every i.
    buf uint8, off int64 (read as u64), length int32 (read as u32).  Returns an int32 device tensor (read it as u32).  One wave per
    range.  Only enqueues on `stream`."""
    import torch

    dev = api._check_tensors(((buf, torch.uint8), (off, torch.int64), (length, torch.int32)))
    n = off.numel()
    if length.numel() != n:
        raise ValueError("off and length must have one length")
    crc = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return crc
    with torch.cuda.device(dev):
        rc = lib().chip_crc32c_batch(n, api._dp(buf), api._dp(off), api._dp(length), api._dp(crc), api._stream_ptr(stream))
    if rc != 0:
        raise RuntimeError(f"chip_crc32c_batch failed: {rc}")
    return crc


def snappy_parallel(in_buf, length, out_buf=None, stream=None):
    """chip_snappy_parallel over a uint8 device tensor holding `length` bytes, ONE framed stream (4-byte aligned, padded to a
    multiple of 4): (out, summary).  With `out_buf` (a uint8 device tensor) the content goes there and `out` is its first out_len
    bytes.  Without, the call is made with no room first, then with a new tensor of total_out bytes; a stream that takes the serial
    path states no size that way, so it is sized by decode_batch_sizes as one unit and decoded with that room -- a stream that is
    refused, or in error, comes back as the empty tensor and its summary.  Synchronous on `stream`."""
    import torch

    dev = api._check_tensors(((in_buf, torch.uint8),) + (((out_buf, torch.uint8),) if out_buf is not None else ()))
    length = int(length)
    if length < 0 or length > in_buf.numel():
        raise ValueError(f"length {length} outside the buffer of {in_buf.numel()} bytes")
    raw = _SnappyParallelSummary()
    base, sp = (api._dp(in_buf) if length else None), api._stream_ptr(stream)

    def call(out):
        cap = out.numel() if out is not None else 0
        rc = lib().chip_snappy_parallel(base, length, api._dp(out) if cap else None, cap, 0, C.byref(raw), sp)
        if rc != 0:
            raise RuntimeError(f"chip_snappy_parallel failed: {rc}")

    with torch.cuda.device(dev):
        if out_buf is None:
            call(None)
            need = int(raw.total_out) if raw.status == int(DecodeStatus.NeedOutput) and raw.path == SNAPPYPAR_PARALLEL else 0
            if raw.status == int(DecodeStatus.NeedOutput) and raw.path == SNAPPYPAR_SERIAL and length <= 0xFFFFFFFF:
                one = lambda v, dt: torch.tensor([v], dtype=torch.int64, device=dev).to(dt)  # noqa: E731
                size, _, st = api.decode_batch_sizes(FMT_SNAPPY, in_buf, one(0, torch.int64), one(length, torch.int32), stream=stream)
                need = int(size[0]) if int(st[0]) == int(DecodeStatus.Finished) and int(size[0]) <= 0xFFFFFFFF else 0
            out_buf = torch.empty(need, dtype=torch.uint8, device=dev)
            if need:
                call(out_buf)
        else:
            call(out_buf)
    return out_buf[:int(raw.out_len)], SnappyParallelSummary(raw)


def snappy_decode(data, device=None, stream=None):
    """The content of a whole .sz file (bytes-like), by snappy_parallel.  Returns a uint8 device tensor.  Raises ValueError where
    the stream does not finish (the message carries its status and in_used).  Waits for the result."""
    import numpy as np
    import torch

    data = bytes(data)
    dev = torch.device("cuda" if device is None else device)
    padded = np.zeros((len(data) + 3) // 4 * 4 + 4, np.uint8)
    padded[:len(data)] = np.frombuffer(data, np.uint8)
    out, s = snappy_parallel(torch.from_numpy(padded).to(dev), len(data), stream=stream)
    if s.status != int(DecodeStatus.Finished):
        raise ValueError(f"snappy_decode: the stream did not finish: status {s.status} at input byte {s.in_used}")
    return out


def _stated_length(block):
    """the preamble of a raw block, or None where it is cut or too long"""
    n = 0
    for i, b in enumerate(block[:5]):
        if i == 4 and b >= 16:
            return None
        n |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return n
    return None


def snappy_blocks_decode(blocks, device=None, stream=None):
    """A list of raw blocks (bytes-like: Parquet pages, RocksDB blocks) decoded in ONE batch, each with the room its preamble states:
    a list of uint8 device tensors, views of one output tensor.  Raises ValueError where a preamble is unreadable, RuntimeError
    naming the first block that did not decode.  Waits for the result."""
    import numpy as np
    import torch

    blocks = [bytes(b) for b in blocks]
    dev = torch.device("cuda" if device is None else device)
    caps = [_stated_length(b) for b in blocks]
    if any(c is None for c in caps):
        raise ValueError(f"snappy_blocks_decode: block {caps.index(None)} has no readable preamble")
    if not blocks:
        return []
    in_off = np.concatenate(([0], np.cumsum([(len(b) + 3) // 4 * 4 for b in blocks]))).astype(np.int64)
    blob = np.zeros(int(in_off[-1]) + 4, np.uint8)
    for o, b in zip(in_off, blocks):
        blob[o:o + len(b)] = np.frombuffer(b, np.uint8)
    out_off = np.concatenate(([0], np.cumsum(caps))).astype(np.int64)
    up = lambda a, dt: torch.from_numpy(np.asarray(a, np.int64)).to(dev).to(dt)  # noqa: E731
    out = api._decode_planned(FMT_SNAPPY_BLOCK, "block", torch.from_numpy(blob).to(dev), up(in_off[:-1], torch.int64),
                              up([len(b) for b in blocks], torch.int32), up(out_off[:-1], torch.int64), up(caps, torch.int32), int(out_off[-1]), stream)
    return [out[int(out_off[i]):int(out_off[i + 1])] for i in range(len(blocks))]
