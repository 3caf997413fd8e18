"""Timing of the batch brotli encoder: python tools/time_brotli_encode.py [units] [qualities]   (default 65536 units x 64 KiB,
qualities 1,5,11).  Prints, per quality, the best of three launches (kernel time, GB/s of input), the ratio, whether the GPU brotli
decoder returns the input, and the same units through the system libbrotlienc on 16 CPU threads (quality 11 on 1 024 units only)."""
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import brotli_ref  # noqa: E402
import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402

FMT_BROTLI, UNIT = 101, 65536
n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
qualities = [int(q) for q in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 5, 11]
dev = torch.device("cuda:0")
pay = synth.payloads(n, threads=16)
cap = (compu_amd.encode_bound(FMT_BROTLI, UNIT) + 15) & ~15
d_in = torch.from_numpy(pay).to(dev)
d_out = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
ar = torch.arange(n, dtype=torch.int64, device=dev)
units = torch.full((n,), UNIT, dtype=torch.int32, device=dev)
back = torch.zeros(n * UNIT, dtype=torch.uint8, device=dev)
for quality in qualities:
    args = (FMT_BROTLI, quality, d_in, ar * UNIT, units, d_out, ar * cap, torch.full((n,), cap, dtype=torch.int32, device=dev))
    compu_amd.encode_batch(*args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ol, st = compu_amd.encode_batch(*args)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    back.zero_()
    dl, iu, ds = compu_amd.decode_batch(FMT_BROTLI, d_out, ar * cap, ol.to(torch.int32), back, ar * UNIT, units)
    torch.cuda.synchronize()
    ok = bool((st == 2).all()) and bool((ds == 2).all()) and torch.equal(back, d_in)
    comp = int(ol.to(torch.int64).sum())
    ms = min(ts)
    print(f"brotli encode quality {quality}, {n} units x 64 KiB: {ms:.2f} ms ({n * UNIT / ms / 1e6:.2f} GB/s of input), "
          f"ratio {comp / (n * UNIT):.4f} (round trip={ok})", flush=True)

enc, _ = brotli_ref.libs()
enc.BrotliEncoderMaxCompressedSize.restype = C.c_size_t
enc.BrotliEncoderMaxCompressedSize.argtypes = [C.c_size_t]
enc.BrotliEncoderCompress.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
bound = enc.BrotliEncoderMaxCompressedSize(UNIT)
for quality in qualities:
    m = min(n, 1024) if quality >= 10 else n
    dst = C.create_string_buffer(m * bound)
    sizes = [0] * m

    def one(i):
        sz = C.c_size_t(bound)
        assert enc.BrotliEncoderCompress(quality, 22, 0, UNIT, C.c_void_p(pay.ctypes.data + i * UNIT), C.byref(sz),
                                         C.c_void_p(C.addressof(dst) + i * bound))
        sizes[i] = sz.value

    with ThreadPoolExecutor(16) as ex:
        t = time.perf_counter()
        list(ex.map(one, range(m)))
        dt = time.perf_counter() - t
    print(f"system libbrotlienc quality {quality}, 16 CPU threads, {m} units: {dt * 1e3:.1f} ms ({m * UNIT / dt / 1e9:.3f} GB/s), "
          f"ratio {sum(sizes) / (m * UNIT):.4f}", flush=True)
