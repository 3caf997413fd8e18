"""Timing of the LZ4 encoders, same process, same card:
python tools/time_lz4_encode.py [units] [file MiB] [repeats]
On the bench payload generator's bytes (bench_support.synth):
  `units` (default 16 384) units of 64 KiB through chip_encode_batch(CHIP_FMT_LZ4_BLOCK) at level 1 and level 9, and beside them
  the same units through chip_encode_batch(CHIP_FMT_ZSTD, level 1), the yardstick: LZ4 has no entropy stage;
  `file MiB` (default 128) through chip_encode_file(CHIP_FMT_LZ4) at 64 KiB and 4 MiB units, with and without the content checksum,
  against the bare batch encode of the same units (the assembly's share) and against chip_lz4_parallel reading the result back.
Each figure is the median of `repeats` (default 5) calls after a warm-up, timed with device events; every result is decoded
again and compared with the payload."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402

units = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
file_mib = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")


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


def time_batch(name, fmt, level, d_in, n, unit, pay):
    """n units of `unit` bytes of d_in through chip_encode_batch; returns the median in ms"""
    slot = (compu_amd.encode_bound(fmt, unit) + 15) // 16 * 16
    in_off = torch.arange(n, dtype=torch.int64, device=dev) * unit
    in_len = torch.full((n,), unit, dtype=torch.int32, device=dev)
    d_out = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    out_off = torch.arange(n, dtype=torch.int64, device=dev) * slot
    out_cap = torch.full((n,), slot, dtype=torch.int32, device=dev)
    m, lo = median_of(lambda: compu_amd.encode_batch(fmt, level, d_in, in_off, in_len, d_out, out_off, out_cap))
    out_len, st = compu_amd.encode_batch(fmt, level, d_in, in_off, in_len, d_out, out_off, out_cap)
    back = torch.zeros(n * unit, dtype=torch.uint8, device=dev)
    _, _, ds = compu_amd.decode_batch(fmt, d_out, out_off, out_len, back, in_off, in_len)
    ok = bool((st == 2).all()) and bool((ds == 2).all()) and bool(np.array_equal(back.cpu().numpy(), pay[:n * unit]))
    total = int(out_len.sum())
    print(f"{name}, level {level}: {n} units of {unit} bytes: {m:.2f} ms (min {lo:.2f}), {n * unit / m / 1e6:.1f} GB/s of input, "
          f"{total / m / 1e6:.1f} GB/s of output, ratio {n * unit / total:.3f} (all finished, decoded = payload: {ok})", flush=True)
    return m


pay = synth.payloads(units, threads=threads)
d_pay = torch.from_numpy(pay).to(dev)
for level in (1, 9):
    time_batch("chip_encode_batch(CHIP_FMT_LZ4_BLOCK)", compu_amd.FMT_LZ4_BLOCK, level, d_pay, units, synth.UNIT, pay)
time_batch("chip_encode_batch(CHIP_FMT_LZ4)", compu_amd.FMT_LZ4, 1, d_pay, units, synth.UNIT, pay)
time_batch("chip_encode_batch(CHIP_FMT_ZSTD)", compu_amd.FMT_ZSTD, 1, d_pay, units, synth.UNIT, pay)

size = file_mib << 20
if pay.size < size:
    pay = synth.payloads(size // synth.UNIT, threads=threads)
    d_pay = torch.from_numpy(pay).to(dev)
pay = pay[:size]
for unit in (65536, 4 << 20):
    bare = time_batch(f"the bare batch of the file's {unit}-byte units", compu_amd.FMT_LZ4_BLOCK, 1, d_pay, size // unit, unit, pay)
    for cchk in (False, True):
        flags = compu_amd.W_LZ4_CONTENT_CHECKSUM if cchk else 0
        room = torch.zeros(compu_amd.encode_file_bound(compu_amd.FMT_LZ4, size, unit, flags), dtype=torch.uint8, device=dev)
        m, lo = median_of(lambda: compu_amd.encode_file(compu_amd.FMT_LZ4, 1, d_pay, size, unit_bytes=unit, flags=flags, out=room))
        out, summ = compu_amd.encode_file(compu_amd.FMT_LZ4, 1, d_pay, size, unit_bytes=unit, flags=flags, out=room)
        d_file = torch.zeros((summ.out_len + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        d_file[:summ.out_len] = out
        back = torch.zeros(size, dtype=torch.uint8, device=dev)
        dm, dlo = median_of(lambda: compu_amd.lz4_parallel(d_file, summ.out_len, back))
        _, ps = compu_amd.lz4_parallel(d_file, summ.out_len, back)
        ok = ps.status == 2 and bool(np.array_equal(back.cpu().numpy(), pay))
        print(f"chip_encode_file(CHIP_FMT_LZ4), {file_mib} MiB at {unit}-byte units, content checksum {'on' if cchk else 'off'}: {m:.2f} ms (min {lo:.2f}), "
              f"{size / m / 1e6:.2f} GB/s of input, {summ.out_len} bytes (ratio {size / summ.out_len:.3f}), the assembly's share {m - bare:.2f} ms; "
              f"chip_lz4_parallel reads it back in {dm:.2f} ms (min {dlo:.2f}), {size / dm / 1e6:.2f} GB/s, path {ps.path} (decoded = payload: {ok})",
              flush=True)
