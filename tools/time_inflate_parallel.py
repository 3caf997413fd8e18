"""Timing of the parallel decode of ONE large gzip stream (chip_inflate_parallel) and of its first pass (chip_inflate_find_starts):
python tools/time_inflate_parallel.py [MiB of content] [chunk KiB, 0 = the default, or a comma list to sweep] [repeats]
The stream is tools/time_inflate_index.py's: `MiB` (default 128) of the bench payload as one gzip member, zlib level 6.  Run that
tool in the same session for the figures to compare with: the one-unit decode, the index build, gzip_index_decode.  After one
warm-up per chunk size, `repeats` (default 3) rounds; every call is synchronous and is timed with device events around it (kernels,
waits and the host work between them).  Every output is compared with the payload, and the index the call leaves is read back once
through gzip_index_decode.  With CHIP_PAR_TIMING=1 in the environment the library prints the device time of each phase of every call."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    mib = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    chunks = [int(x) * 1024 for x in (sys.argv[2] if len(sys.argv) > 2 else "0").split(",")]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    threads = min(16, len(os.sched_getaffinity(0)))

    from bench_support import synth
    from time_inflate_index import one_member

    pay = synth.payloads(mib * (1 << 20) // synth.UNIT, threads=threads)
    comp = one_member(pay, threads)

    import torch

    import compu_amd

    dev = torch.device("cuda:0")
    GZIP = int(compu_amd.ZlibMode.Gzip)
    total, length = pay.size, len(comp)
    d_in = torch.zeros((length + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
    d_in[:length] = torch.frombuffer(bytearray(comp), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(total, dtype=torch.uint8, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    def stats(ts):
        return f"{float(np.median(ts)):.3f} ms (min {min(ts):.3f})"

    print(f"one gzip member, {total} bytes of content in {length}, {reps} rounds", flush=True)
    for chunk in chunks:
        eff = chunk or compu_amd.api.PAR_DEFAULT_CHUNK
        _, index, summ = compu_amd.inflate_parallel(GZIP, d_in, length, out_buf=d_out, chunk_bytes=chunk, index=True)
        assert (summ.status, summ.out_len, summ.in_used, summ.check) == (2, total, length, zlib.crc32(pay)), summ
        index_ok = np.array_equal(compu_amd.gzip_index_decode(index, d_in).cpu().numpy(), pay)
        compu_amd.inflate_find_starts(d_in, length, 80, eff)
        t_par, t_find, ok = [], [], True
        for _ in range(reps):
            d_out.zero_()
            t, (_, s) = timed(lambda: compu_amd.inflate_parallel(GZIP, d_in, length, out_buf=d_out, chunk_bytes=chunk))
            t_par.append(t)
            ok = ok and (s.status, s.path) == (2, 1) and np.array_equal(d_out.cpu().numpy(), pay)
            t_find.append(timed(lambda: compu_amd.inflate_find_starts(d_in, length, 80, eff, max_starts=0))[0])
        print(f"  chunk {eff >> 10:4d} KiB: chip_inflate_parallel {stats(t_par)}   chip_inflate_find_starts {stats(t_find)}   "
              f"starts {summ.n_starts}, false {summ.n_false}, chain {summ.n_points} of {-(-length // eff)} chunks   "
              f"(decoded = payload: {ok}; index reads back: {index_ok})", flush=True)


if __name__ == "__main__":
    main()
