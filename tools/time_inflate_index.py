"""Timing of the checkpoint index of ONE large gzip stream (chip_inflate_index_build, chip_inflate_index_read) against
chip_decode_batch of the same stream as a single unit, same process, same box:
python tools/time_inflate_index.py [MiB of content] [spacing in KiB, 0 = the default 1 MiB] [repeats] [ranges] [bytes per range]
Builds `MiB` (default 128) of the bench payload generator (bench_support.synth) and compresses it on the host into one gzip member
(zlib level 6, in pieces of 1 MiB joined by sync flushes, so that the host work is spread over the cores: one deflate stream, one
trailer).  After one warm-up of each, `repeats` (default 3) rounds, each call timed with device events around it (the index calls
are synchronous, so their windows are whole calls: kernels, waits and the host work between them):
  one unit     chip_decode_batch(CHIP_FMT_GZIP, 1, ..): one wave, the serial baseline (the decode kernel is the parent commit's,
               instruction for instruction)
  build        chip_inflate_index_build at `spacing`: the same decode plus recording, windows and checks
  index decode gzip_index_decode: every chunk a unit of the batch decoder, verified chunk by chunk
  ranges       `ranges` (default 1024) ranges of `bytes per range` (default 10000) at seeded random offsets through the index,
               against decode-everything-and-slice (the one-unit decode plus one gather of the same ranges)
Prints the median and the fastest of each and checks every output against the payload."""
import os
import struct
import sys
import zlib
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECE = 1 << 20


def _deflate_piece(args):
    data, last = args
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)


def one_member(pay, threads):
    mv = memoryview(pay)
    jobs = [(bytes(mv[i:i + PIECE]), i + PIECE >= len(mv)) for i in range(0, len(mv), PIECE)]
    with Pool(threads) as pool:
        body = b"".join(pool.map(_deflate_piece, jobs))
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + body + struct.pack("<II", zlib.crc32(mv), len(mv) & 0xFFFFFFFF)


def main():
    mib = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    spacing = (int(sys.argv[2]) if len(sys.argv) > 2 else 0) * 1024
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    n_ranges = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
    range_bytes = int(sys.argv[5]) if len(sys.argv) > 5 else 10000
    threads = min(16, len(os.sched_getaffinity(0)))

    from bench_support import synth

    pay = synth.payloads(mib * (1 << 20) // synth.UNIT, threads=threads)
    comp = one_member(pay, threads)

    import torch

    import compu_amd
    from compu_amd.api import _ranges_to_device

    dev = torch.device("cuda:0")
    GZIP = int(compu_amd.ZlibMode.Gzip)
    total, length = pay.size, len(comp)
    d_in = torch.zeros((length + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
    d_in[:length] = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(total, dtype=torch.uint8, device=dev)
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev).to(torch.int32)  # noqa: E731
    rng = np.random.default_rng(1)
    ranges = [(int(lo), range_bytes) for lo in rng.integers(0, total - range_bytes, n_ranges)]
    r_lo, r_len = _ranges_to_device(ranges, dev)
    gather_idx = (r_lo[:, None] + torch.arange(range_bytes, device=dev)[None, :]).reshape(-1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    def one_unit():
        return compu_amd.decode_batch(GZIP, d_in, i64(0), i32(length), d_out, i64(0), i32(total))

    def build():
        return compu_amd.inflate_index_build(GZIP, d_in, length, d_out, spacing=spacing)

    def slice_all():
        one_unit()
        return d_out[gather_idx]

    def stats(ts):
        return f"{float(np.median(ts)):.3f} ms (min {min(ts):.3f})"

    one_unit()
    index, summ = build()
    torch.cuda.synchronize()
    assert (summ.status, summ.out_len, summ.in_used, summ.check) == (2, total, length, zlib.crc32(pay))
    built_ok = np.array_equal(d_out.cpu().numpy(), pay)
    compu_amd.gzip_index_decode(index, d_in)
    compu_amd.gzip_index_read(index, d_in, (r_lo, r_len))

    t_unit, t_build, t_dec, t_rng, t_slice = [], [], [], [], []
    for _ in range(reps):
        d_out.zero_()
        t, (out_len, in_used, status) = timed(one_unit)
        t_unit.append(t)
        unit_ok = (int(status[0]), int(out_len[0]) & 0xFFFFFFFF) == (2, total) and np.array_equal(d_out.cpu().numpy(), pay)
        t_build.append(timed(build)[0])
        t, out = timed(lambda: compu_amd.gzip_index_decode(index, d_in))
        t_dec.append(t)
        dec_ok = np.array_equal(out.cpu().numpy(), pay)
        t, (got, _) = timed(lambda: compu_amd.gzip_index_read(index, d_in, (r_lo, r_len)))
        t_rng.append(t)
        t, want = timed(slice_all)
        t_slice.append(t)
        rng_ok = bool(torch.equal(got, want))
    mu, mb, md, mr, ms = (float(np.median(t)) for t in (t_unit, t_build, t_dec, t_rng, t_slice))
    print(f"one gzip member, {total} bytes of content in {length}, spacing {spacing or 1 << 20}: {index.n_points} points, {reps} rounds", flush=True)
    print(f"  one unit (chip_decode_batch)   {stats(t_unit)}   (decoded = payload: {unit_ok})", flush=True)
    print(f"  chip_inflate_index_build       {stats(t_build)}   build / one unit {mb / mu:.4f}   (decoded = payload: {built_ok})", flush=True)
    print(f"  gzip_index_decode              {stats(t_dec)}   one unit / index decode x{mu / md:.1f}   (decoded = payload: {dec_ok})", flush=True)
    print(f"  {n_ranges} ranges of {range_bytes} B         {stats(t_rng)}   decode everything and slice {stats(t_slice)}, x{ms / mr:.1f}   "
          f"(same bytes: {rng_ok})", flush=True)


if __name__ == "__main__":
    main()
