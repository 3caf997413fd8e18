"""Timing of the LZ4 decoders, same process, same card:
python tools/time_lz4.py [units] [frame MiB] [repeats]
On the bench payload generator's bytes (bench_support.synth), compressed with the system's liblz4 / libzstd:
  `units` (default 16 384) blocks of 64 KiB through chip_decode_batch(CHIP_FMT_LZ4_BLOCK) and its size pass, beside the same units
  as zstd frames (level 3) through chip_decode_batch(CHIP_FMT_ZSTD);
  one frame of `frame MiB` (default 128) of independent blocks with a content checksum, at BD 4 (64 KiB blocks) and BD 7 (4 MiB
  blocks), through chip_lz4_parallel with the checksum compared and waived, against its one-unit CHIP_FMT_LZ4 decode (one wave,
  once).
Each figure is the median of `repeats` (default 5) calls after a warm-up, timed with device events, and every output is compared
with the payload."""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from tools.make_lz4_golden import Preferences  # noqa: E402

units = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
frame_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
lz4 = C.CDLL(ctypes.util.find_library("lz4"))
lz4.LZ4F_compressFrameBound.restype = lz4.LZ4F_compressFrame.restype = C.c_size_t
lz4.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
lz4.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
lz4.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
zstd = C.CDLL("libzstd.so.1")
zstd.ZSTD_compress.restype = zstd.ZSTD_compressBound.restype = C.c_size_t
zstd.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
zstd.ZSTD_compressBound.argtypes = [C.c_size_t]


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


def pack_units(pay, compress, bound):
    """every 64 KiB unit compressed on its own, the results 16-byte aligned in one buffer"""
    n = pay.size // synth.UNIT
    buf = np.zeros(n * ((bound + 15) // 16 * 16), np.uint8)
    offs, lens, at = np.zeros(n, np.int64), np.zeros(n, np.int32), 0
    for i in range(n):
        k = compress(buf.ctypes.data + at, buf.size - at, pay.ctypes.data + i * synth.UNIT)
        offs[i], lens[i] = at, k
        at += (k + 15) // 16 * 16
    return buf[:at + 16], offs, lens


def time_batch(name, fmt, pay, buf, offs, lens, sizes=False):
    n = offs.size
    d_in, d_off, d_len = torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
    d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)
    out_off = torch.arange(n, dtype=torch.int64, device=dev) * synth.UNIT
    out_cap = torch.full((n,), synth.UNIT, dtype=torch.int32, device=dev)
    m, lo = median_of(lambda: compu_amd.decode_batch(fmt, d_in, d_off, d_len, d_out, out_off, out_cap))
    _, _, st = compu_amd.decode_batch(fmt, d_in, d_off, d_len, d_out, out_off, out_cap)
    ok = bool((st == 2).all()) and bool(np.array_equal(d_out.cpu().numpy(), pay))
    print(f"{name}: {n} units of 64 KiB, {int(lens.sum())} compressed bytes: {m:.2f} ms (min {lo:.2f}), {pay.size / m / 1e6:.1f} GB/s of output "
          f"(all finished, decoded = payload: {ok})", flush=True)
    if sizes:
        m, lo = median_of(lambda: compu_amd.decode_batch_sizes(fmt, d_in, d_off, d_len))
        size, _, st = compu_amd.decode_batch_sizes(fmt, d_in, d_off, d_len)
        print(f"{name}, size pass: {m:.2f} ms (min {lo:.2f}), {pay.size / m / 1e6:.1f} GB/s of content counted (all 64 KiB: "
              f"{bool((size == synth.UNIT).all()) and bool((st == 2).all())})", flush=True)


pay = synth.payloads(units, threads=threads)
time_batch("chip_decode_batch(CHIP_FMT_LZ4_BLOCK)", compu_amd.FMT_LZ4_BLOCK, pay,
           *pack_units(pay, lambda dst, room, src: lz4.LZ4_compress_default(src, dst, synth.UNIT, min(room, 1 << 30)), lz4.LZ4_compressBound(synth.UNIT)), sizes=True)
time_batch("chip_decode_batch(CHIP_FMT_ZSTD), level 3", compu_amd.FMT_ZSTD, pay,
           *pack_units(pay, lambda dst, room, src: zstd.ZSTD_compress(dst, room, src, synth.UNIT, 3), zstd.ZSTD_compressBound(synth.UNIT)))

pay = pay[:frame_mib << 20] if pay.size >= frame_mib << 20 else synth.payloads((frame_mib << 20) // synth.UNIT, threads=threads)
for bd in (4, 7):
    prefs = Preferences()
    prefs.frameInfo.blockSizeID, prefs.frameInfo.blockMode, prefs.frameInfo.contentChecksumFlag = bd, 1, 1
    host = np.zeros((lz4.LZ4F_compressFrameBound(pay.size, C.byref(prefs)) + 3) // 4 * 4, np.uint8)
    length = lz4.LZ4F_compressFrame(host.ctypes.data, host.size, pay.ctypes.data, pay.size, C.byref(prefs))
    assert length <= host.size
    d_in = torch.from_numpy(host[:(length + 3) // 4 * 4]).to(dev)
    d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)
    print(f"one LZ4 frame at BD {bd}: {pay.size >> 20} MiB of content in {length} bytes", flush=True)
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev).to(torch.int32)  # noqa: E731
    unit, (_, _, st) = timed(lambda: compu_amd.decode_batch(compu_amd.FMT_LZ4, d_in, i64(0), i32(length), d_out, i64(0), i32(pay.size)))
    print(f"  one unit of chip_decode_batch(CHIP_FMT_LZ4) (one wave, once): {unit:.1f} ms, {pay.size / unit / 1e6:.3f} GB/s (status {int(st[0])}, "
          f"decoded = payload: {bool(np.array_equal(d_out.cpu().numpy(), pay))})", flush=True)
    for checksum in (True, False):
        d_out.zero_()
        m, lo = median_of(lambda: compu_amd.lz4_parallel(d_in, length, d_out, checksum=checksum))
        _, summ = compu_amd.lz4_parallel(d_in, length, d_out, checksum=checksum)
        print(f"  chip_lz4_parallel, content checksum {'compared' if checksum else 'waived'}: {m:.2f} ms (min {lo:.2f}, {reps} calls), "
              f"{pay.size / m / 1e6:.2f} GB/s, x{unit / m:.1f} of the one wave; {summ!r} (decoded = payload: "
              f"{bool(np.array_equal(d_out.cpu().numpy(), pay))})", flush=True)
