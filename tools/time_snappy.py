"""Timing of the Snappy decoders, same process, same card:
python tools/time_snappy.py [units] [stream MiB] [repeats]
On the bench payload generator's bytes (bench_support.synth).  Compression is libsnappy's through pyarrow where that imports;
otherwise the test writer (tests/snappy_writer.py) compresses 32 distinct units and they are tiled.  The tool prints which.
  `units` (default 16 384) blocks of 64 KiB through chip_decode_batch(CHIP_FMT_SNAPPY_BLOCK) and its size pass, beside the same
  content as LZ4 blocks (liblz4 where ctypes finds it, else the library's own host encoder) through
  chip_decode_batch(CHIP_FMT_LZ4_BLOCK);
  one framed stream of `stream MiB` (default 128) of content in 64 KiB compressed chunks through chip_snappy_parallel, against its
  one-unit CHIP_FMT_SNAPPY decode (one wave, once).  The chunks' CRCs are computed by chip_crc32c_batch, which the tests hold to the
  reference CRC-32C.
Each figure is the median of `repeats` (default 5) calls after a warm-up, timed with device events, and every output is compared
with the payload."""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from compu_amd import snappy  # noqa: E402

units = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
stream_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
UNIT = synth.UNIT


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def median_of(fn):
    fn()
    torch.cuda.synchronize()
    ts = [timed(fn)[0] for _ in range(reps)]
    return float(np.median(ts)), min(ts)


def payload_and_blocks(n):
    """(payload, [a Snappy block per 64 KiB unit]) and the writer's name"""
    try:
        import pyarrow

        pay = synth.payloads(n, threads=threads)
        return pay, [pyarrow.compress(pay[i * UNIT:(i + 1) * UNIT].tobytes(), codec="snappy", asbytes=True) for i in range(n)], f"libsnappy (pyarrow {pyarrow.__version__})"
    except ImportError:
        import snappy_writer as W

        distinct = min(n, 32)
        few = synth.payloads(distinct, threads=threads)
        blocks = [W.compress_block(few[i * UNIT:(i + 1) * UNIT].tobytes()) for i in range(distinct)]
        reps_ = -(-n // distinct)
        return np.tile(few, reps_)[:n * UNIT], (blocks * reps_)[:n], f"tests/snappy_writer.py, {distinct} distinct units tiled"


def lz4_blocks(pay, n):
    path = ctypes.util.find_library("lz4")
    if path:
        lz4 = C.CDLL(path)
        lz4.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        room = C.create_string_buffer(lz4.LZ4_compressBound(UNIT))
        out = []
        for i in range(n):
            k = lz4.LZ4_compress_default(pay.ctypes.data + i * UNIT, room, UNIT, len(room))
            out.append(room.raw[:k])
        return out, "liblz4"
    cache = {}
    out = []
    for i in range(n):
        unit = pay[i * UNIT:(i + 1) * UNIT].tobytes()
        if unit not in cache:
            cache[unit] = compu_amd.lz4_block_encode_host(unit, 1)[0]
        out.append(cache[unit])
    return out, "chip_lz4_block_encode_host"


def pack(blocks):
    """the blocks 16-byte aligned in one buffer"""
    offs = np.zeros(len(blocks), np.int64)
    lens = np.asarray([len(b) for b in blocks], np.int32)
    offs[1:] = np.cumsum((lens[:-1].astype(np.int64) + 15) // 16 * 16)
    buf = np.zeros(int(offs[-1]) + (int(lens[-1]) + 15) // 16 * 16 + 16, np.uint8)
    for o, b in zip(offs, blocks):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return buf, offs, lens


def time_batch(name, fmt, pay, buf, offs, lens, sizes=False):
    n = offs.size
    d_in, d_off, d_len = torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
    d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)
    out_off = torch.arange(n, dtype=torch.int64, device=dev) * UNIT
    out_cap = torch.full((n,), UNIT, dtype=torch.int32, device=dev)
    m, lo = median_of(lambda: compu_amd.decode_batch(fmt, d_in, d_off, d_len, d_out, out_off, out_cap))
    _, _, st = compu_amd.decode_batch(fmt, d_in, d_off, d_len, d_out, out_off, out_cap)
    ok = bool((st == 2).all()) and bool(np.array_equal(d_out.cpu().numpy(), pay))
    print(f"{name}: {n} units of 64 KiB, {int(lens.sum())} compressed bytes: {m:.2f} ms (min {lo:.2f}), {pay.size / m / 1e6:.1f} GB/s of output "
          f"(all finished, decoded = payload: {ok})", flush=True)
    if sizes:
        ms, lo = median_of(lambda: compu_amd.decode_batch_sizes(fmt, d_in, d_off, d_len))
        size, _, st = compu_amd.decode_batch_sizes(fmt, d_in, d_off, d_len)
        print(f"{name}, size pass: {ms:.2f} ms (min {lo:.2f}), {pay.size / ms / 1e6:.1f} GB/s of content counted (all 64 KiB: "
              f"{bool((size == UNIT).all()) and bool((st == 2).all())})", flush=True)
    return m


pay, blocks, writer = payload_and_blocks(units)
print(f"Snappy blocks written by {writer}", flush=True)
t_snappy = time_batch("chip_decode_batch(CHIP_FMT_SNAPPY_BLOCK)", snappy.FMT_SNAPPY_BLOCK, pay, *pack(blocks), sizes=True)
lz4b, lz4_writer = lz4_blocks(pay, units)
print(f"LZ4 blocks written by {lz4_writer}", flush=True)
t_lz4 = time_batch("chip_decode_batch(CHIP_FMT_LZ4_BLOCK)", compu_amd.FMT_LZ4_BLOCK, pay, *pack(lz4b))
print(f"Snappy batch / LZ4 batch on the same content: x{t_snappy / t_lz4:.2f} of its time", flush=True)

# one framed stream: the identifier, then a compressed chunk per unit with the masked CRC-32C of its content
n = min(units, (stream_mib << 20) // UNIT)
pay, blocks = pay[:n * UNIT], blocks[:n]
d_pay = torch.from_numpy(pay).to(dev)
crc = snappy.crc32c_batch(d_pay, torch.arange(n, dtype=torch.int64, device=dev) * UNIT, torch.full((n,), UNIT, dtype=torch.int32, device=dev))
crc = crc.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
masked = (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF
parts = [snappy.SNAPPY_IDENT]
for b, c in zip(blocks, masked):
    parts.append(b"\x00" + (len(b) + 4).to_bytes(3, "little") + int(c).to_bytes(4, "little") + b)
sz = b"".join(parts)
host = np.zeros((len(sz) + 3) // 4 * 4, np.uint8)
host[:len(sz)] = np.frombuffer(sz, np.uint8)
d_in = torch.from_numpy(host).to(dev)
d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)
print(f"one .sz: {pay.size >> 20} MiB of content in {len(sz)} bytes, {n} chunks", flush=True)
i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
i32 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev).to(torch.int32)  # noqa: E731
unit, (_, _, st) = timed(lambda: compu_amd.decode_batch(snappy.FMT_SNAPPY, d_in, i64(0), i32(len(sz)), d_out, i64(0), i32(pay.size)))
print(f"  one unit of chip_decode_batch(CHIP_FMT_SNAPPY) (one wave, once): {unit:.1f} ms, {pay.size / unit / 1e6:.3f} GB/s (status {int(st[0])}, "
      f"decoded = payload: {bool(np.array_equal(d_out.cpu().numpy(), pay))})", flush=True)
d_out.zero_()
m, lo = median_of(lambda: snappy.snappy_parallel(d_in, len(sz), d_out))
_, summ = snappy.snappy_parallel(d_in, len(sz), d_out)
print(f"  chip_snappy_parallel: {m:.2f} ms (min {lo:.2f}, {reps} calls), {pay.size / m / 1e6:.2f} GB/s, x{unit / m:.1f} of the one wave; {summ!r} "
      f"(decoded = payload: {bool(np.array_equal(d_out.cpu().numpy(), pay))})", flush=True)
