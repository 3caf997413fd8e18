"""Timing of the slabbed decode of ONE deflate stream (chip_inflate_parallel_next), both at the default chunk_bytes, in one session:
python tools/time_inflate_stream.py [MiB of content for (a)] [repeats] [GiB of content for (b), 0 = skip]
(a) tools/time_inflate_parallel.py's stream -- `MiB` (default 128) of the bench payload as one gzip member -- through slabs of 8, 32
    and 128 MiB of input, beside one chip_inflate_parallel call on the same stream.  Input and output stay on the device; after a
    warm-up, `repeats` (default 3) rounds, each timed with device events around all its calls; every output is compared with the
    payload.  Per slab size: the calls, the input bytes presented twice (the tail a call leaves to the next) and the time.
(b) a stream beyond a unit's limits: more than `GiB` (default 4) GiB of content and more than 512 MiB of input, made of one piece
    compressed once up to a full flush, its bytes repeated, and a closing piece.  Decoded device to device through 64 MiB slabs
    into one reused room; the total and the CRC-32 (zlib.crc32 over the pieces) are checked against the cursor and by the call
    itself against the trailer.
With CHIP_PAR_TIMING=1 in the environment the library prints the device time of each phase of every call."""
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FINISHED, NEED_INPUT, NEED_OUTPUT = 2, 0, 1


def decode(compu_amd, d_in, length, d_out, slab, fmt=31, keep=True):
    """the whole stream d_in[:length] through slabs of `slab` bytes; keep: the content is laid out in d_out, else every call writes
    to its beginning -> (cursor, calls, bytes presented in all, calls on the parallel path)"""
    cur = compu_amd.InflateCursor(fmt, d_in.device)
    pos = at = calls = shown = par = 0
    while True:
        n = min(slab, length - pos)
        s = compu_amd.inflate_parallel_next(cur, d_in[pos:pos + n], d_out[at:] if keep else d_out)
        calls, shown, par = calls + 1, shown + n, par + s.path
        pos += s.in_used
        at += s.out_len if keep else 0
        if s.status == FINISHED:
            return cur, calls, shown, par
        assert s.status in (NEED_INPUT, NEED_OUTPUT) and (s.in_used or s.out_len), s


def main():
    mib = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    gib = float(sys.argv[3]) if len(sys.argv) > 3 else 4
    threads = min(16, len(os.sched_getaffinity(0)))

    from bench_support import synth
    from time_inflate_index import one_member

    import torch

    import compu_amd

    dev = torch.device("cuda:0")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    def stats(ts):
        return f"{float(np.median(ts)):.3f} ms (min {min(ts):.3f})"

    def to_device(data):
        t = torch.zeros((len(data) + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        return t

    # ---- (a)
    if mib:
        pay = synth.payloads(mib * (1 << 20) // synth.UNIT, threads=threads)
        comp = one_member(pay, threads)
        total, length = pay.size, len(comp)
        d_in, d_out = to_device(comp), torch.zeros(total, dtype=torch.uint8, device=dev)
        print(f"(a) one gzip member, {total} bytes of content in {length}, {reps} rounds, chunk {compu_amd.api.PAR_DEFAULT_CHUNK >> 10} KiB", flush=True)
        compu_amd.inflate_parallel(31, d_in, length, out_buf=d_out)
        t_one, ok = [], True
        for _ in range(reps):
            d_out.zero_()
            t, (_, s) = timed(lambda: compu_amd.inflate_parallel(31, d_in, length, out_buf=d_out))
            t_one.append(t)
            ok = ok and (s.status, s.path) == (2, 1) and np.array_equal(d_out.cpu().numpy(), pay)
        print(f"  one chip_inflate_parallel call: {stats(t_one)}   (decoded = payload: {ok})", flush=True)
        for slab in (8 << 20, 32 << 20, 128 << 20):
            decode(compu_amd, d_in, length, d_out, slab)
            ts, ok = [], True
            for _ in range(reps):
                d_out.zero_()
                t, (cur, calls, shown, par) = timed(lambda: decode(compu_amd, d_in, length, d_out, slab))
                ts.append(t)
                ok = ok and (cur.out_total, cur.in_total, cur.check) == (total, length, zlib.crc32(pay)) and np.array_equal(d_out.cpu().numpy(), pay)
            print(f"  slabs of {slab >> 20:3d} MiB: {stats(ts)}   {calls} calls ({par} parallel), {shown - length} input bytes presented twice "
                  f"({100.0 * (shown - length) / length:.2f} %)   (decoded = payload: {ok})", flush=True)
        del d_in, d_out
        compu_amd.lib().chip_trim()
        torch.cuda.empty_cache()

    # ---- (b)
    if gib:
        piece = synth.payloads((32 << 20) // synth.UNIT, threads=threads).tobytes()
        last = piece[: 1 << 20]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = co.compress(piece) + co.flush(zlib.Z_FULL_FLUSH)  # ends on a byte, and nothing behind it reaches in front of it
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        tail = co.compress(last) + co.flush()
        n = max(int(gib * (1 << 30)) // len(piece) + 1, (512 << 20) // len(body) + 1)
        total = n * len(piece) + len(last)
        crc = 0
        for _ in range(n):
            crc = zlib.crc32(piece, crc)
        crc = zlib.crc32(last, crc)
        head = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"
        length = len(head) + n * len(body) + len(tail) + 8
        d_in = torch.zeros(length + 8, dtype=torch.uint8, device=dev)
        d_in[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
        d_body = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
        for k in range(n):
            d_in[len(head) + k * len(body):len(head) + (k + 1) * len(body)] = d_body
        end = tail + struct.pack("<II", crc, total & 0xFFFFFFFF)
        d_in[length - len(end):length] = torch.frombuffer(bytearray(end), dtype=torch.uint8).to(dev)
        assert total > 1 << 32 and length > 512 << 20
        d_out = torch.zeros(768 << 20, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cur, calls, shown, par = decode(compu_amd, d_in, length, d_out, 64 << 20, keep=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = (cur.out_total, cur.in_total, cur.check, cur.phase) == (total, length, crc, compu_amd.api.CUR_DONE)
        print(f"(b) one gzip member, {total} bytes of content in {length} ({n} pieces of {len(piece)} in {len(body)}): {dt:.3f} s, "
              f"{total / dt / 1e9:.2f} GB/s of content, {calls} calls ({par} parallel) through 64 MiB slabs   (total and CRC-32 as computed: {ok})",
              flush=True)
        assert ok


if __name__ == "__main__":
    main()
