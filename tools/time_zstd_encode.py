"""Timing of the batch zstd encoder: python tools/time_zstd_encode.py [units] [level]   (default 65536 units x 64 KiB, level 3)
Prints the best of three launches (kernel time, GB/s of input), the ratio, whether the GPU zstd decoder returns the input, and the
same units through the system libzstd at level 1 on 16 CPU threads.  ESTATS=1 with a -DCHIP_STATS build
(COMPU_HIP_LIB=compu_amd/libcompu_hip_stats.so) prints the kernel's own cycle counters per phase."""
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

import compu_amd  # noqa: E402
import zstd_ref  # noqa: E402
from bench_support import synth  # noqa: E402

FMT_ZSTD, UNIT = 100, 65536
n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
level = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")
pay = synth.payloads(n, threads=16)
cap = (compu_amd.encode_bound(FMT_ZSTD, UNIT) + 15) & ~15
d_in = torch.from_numpy(pay).to(dev)
d_out = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
ar = torch.arange(n, dtype=torch.int64, device=dev)
units = torch.full((n,), UNIT, dtype=torch.int32, device=dev)
args = (FMT_ZSTD, level, d_in, ar * UNIT, units, d_out, ar * cap, torch.full((n,), cap, dtype=torch.int32, device=dev))
estats = None
if os.environ.get("ESTATS") == "1":
    estats = torch.zeros(n * 16, dtype=torch.int64, device=dev)
    os.environ["CHIP_STATS_PTR"] = str(estats.data_ptr())
compu_amd.encode_batch(*args)
torch.cuda.synchronize()
if estats is not None:
    estats_host = estats.cpu().numpy().copy()
    os.environ.pop("CHIP_STATS_PTR")
ts = []
for _ in range(3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ol, st = compu_amd.encode_batch(*args)
    b.record()
    torch.cuda.synchronize()
    ts.append(a.elapsed_time(b))
back = torch.zeros(n * UNIT, dtype=torch.uint8, device=dev)
dl, iu, ds = compu_amd.decode_batch(FMT_ZSTD, d_out, ar * cap, ol.to(torch.int32), back, ar * UNIT, units)
torch.cuda.synchronize()
ok = bool((st == 2).all()) and bool((ds == 2).all()) and torch.equal(back, d_in)
comp = int(ol.to(torch.int64).sum())
ms = min(ts)
print(f"{os.path.basename(os.environ.get('COMPU_HIP_LIB', 'prod'))}: zstd encode level {level}, {n} units x 64 KiB: {ms:.2f} ms "
      f"({n * UNIT / ms / 1e6:.2f} GB/s of input), ratio {comp / (n * UNIT):.4f} (round trip={ok})")
if estats is not None:
    z = estats_host.reshape(n, 16).astype(np.float64).mean(axis=0)
    tot = z[0] + z[1] + z[2] + z[3]
    for i, name in enumerate(("match finding", "literals (Huffman)", "sequences (FSE)", "frame, blocks, checksum")):
        print(f"  cycles per unit, {name:26s} {z[i]:14.0f}  ({100 * z[i] / tot:5.1f} %)")

zl = zstd_ref.load()
if zl is not None:
    zb = zl.ZSTD_compressBound(UNIT)
    dst = np.zeros(n * zb, np.uint8)
    sizes = np.zeros(n, np.int64)

    def one(i):
        sizes[i] = zl.ZSTD_compress(C.c_void_p(dst.ctypes.data + i * zb), zb, C.c_void_p(pay.ctypes.data + i * UNIT), UNIT, 1)

    with ThreadPoolExecutor(16) as ex:
        t = time.perf_counter()
        list(ex.map(one, range(n)))
        dt = time.perf_counter() - t
    print(f"system libzstd level 1, 16 CPU threads: {dt * 1e3:.1f} ms ({n * UNIT / dt / 1e9:.2f} GB/s), ratio {sizes.sum() / (n * UNIT):.4f}")
