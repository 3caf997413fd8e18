"""Timing of the brotli decode kernel on synthetic 64 KiB units, against libbrotlidec on 16 threads over the same streams:
python tools/time_brotli.py [quality units] ...   (default: 5 65536, 9 65536, 11 8192)"""
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import brotli_ref as B  # noqa: E402
import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402

UNIT = 65536


def cpu_rate(parts, threads=16):
    _, dec = B.libs()
    dec.BrotliDecoderDecompress.argtypes = [C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    outs = [C.create_string_buffer(UNIT) for _ in range(threads)]

    def work(k):
        dst = outs[k]
        for i in range(k, len(parts), threads):
            n = C.c_size_t(UNIT)
            if dec.BrotliDecoderDecompress(len(parts[i]), parts[i], C.byref(n), dst) != 1 or n.value != UNIT:
                raise RuntimeError(f"libbrotlidec failed on unit {i}")

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return time.perf_counter() - t0


def run(quality, n):
    dev = torch.device("cuda:0")
    pay = synth.payloads(n)
    mv = memoryview(pay)
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(lambda i: B.compress(bytes(mv[i * UNIT:(i + 1) * UNIT]), quality, 22), range(n)))
    lens = np.array([len(p) for p in parts], np.int32)
    padded = [p + b"\0" * (-len(p) % 4) for p in parts]
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(np.array([len(p) for p in padded[:-1]], np.int64))
    buf = np.frombuffer(b"".join(padded) + b"\0" * 4, np.uint8).copy()
    d_out = torch.zeros(n * UNIT, dtype=torch.uint8, device=dev)
    args = (compu_amd.FMT_BROTLI, torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev), d_out,
            torch.arange(n, dtype=torch.int64, device=dev) * UNIT, torch.full((n,), UNIT, dtype=torch.int32, device=dev))
    compu_amd.decode_batch(*args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ol, iu, st = compu_amd.decode_batch(*args)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ok = bool((st == 2).all()) and torch.equal(d_out, torch.from_numpy(pay).to(dev))
    ms = min(ts)
    cpu_s = cpu_rate(parts)
    gb = n * UNIT / 1e9
    print(f"brotli q{quality}: {n} units x 64 KiB, ratio {lens.sum() / (n * UNIT):.3f}: kernel {ms:.2f} ms = {gb / (ms / 1e3):.2f} GB/s "
          f"(correct={ok}); libbrotlidec 16 threads {cpu_s * 1e3:.1f} ms = {gb / cpu_s:.2f} GB/s", flush=True)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    jobs = list(zip(a[::2], a[1::2])) if a else [(5, 65536), (9, 65536), (11, 8192)]
    for q, n in jobs:
        run(q, n)
