"""Timing of the tar plan (chip_tar_plan), same process, same box:
python tools/time_tar.py [--n MEMBERS] [--size BYTES] [--reps R] [--level L]
A synthetic ustar archive of --n members (default 16 384) of --size bytes each (default 16 384) of the bench payload generator
(bench_support.synth), every eighth name long enough for a GNU L header, two zero blocks at the end.  Reported:
  chip_tar_plan       the whole synchronous call with the records written (candidates, describe, chain, output; two waits), timed
                      with device events around it: the median and the minimum of --reps (default 20) calls after three warm-up calls
  chip_tar_plan_host  the serial walk over the same image in host memory, host clock, median of five
  inflate_parallel    chip_inflate_parallel over the same archive gzipped (zlib level --level, default 1) into a buffer that is there,
                      device events, median of five after two warm-up calls: what producing the image costs, to set the plan beside
The device plan's records and summary are compared with the host plan's before anything is timed.  Needs the GPU: there is no
CPU timing to fall back to."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16384)
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--level", type=int, default=1)
args = ap.parse_args()
assert torch.cuda.is_available(), "time_tar.py measures on the GPU"
dev = torch.device("cuda:0")


def header(name, size, typeflag=b"0"):
    h = bytearray(512)
    h[0:len(name)] = name
    h[100:108], h[108:116], h[116:124] = b"0000644\0", b"0001750\0", b"0001750\0"
    h[124:136], h[136:148] = b"%011o\0" % size, b"%011o\0" % 1700000000
    h[148:156], h[156:157], h[257:265] = b" " * 8, typeflag, b"ustar\x0000"
    h[148:156] = b"%06o\0 " % sum(h)
    return bytes(h)


def archive(n, size):
    pad = bytes(-size % 512)
    units = -(-max(n * size, 1) // synth.UNIT)
    content = np.asarray(synth.payloads(units, threads=min(16, len(os.sched_getaffinity(0))))).tobytes()
    parts = []
    for k in range(n):
        name = b"shard/%08d.bin" % k
        if k % 8 == 7:
            name = b"shard/" + b"deep/" * 24 + b"%08d.bin" % k  # above 100 bytes: a GNU long name
            parts += [header(b"././@LongLink", len(name) + 1, b"L"), name + bytes(-(len(name) + 1) % 512 + 1)]
        parts += [header(name[:100], size), content[k * size:(k + 1) * size], pad]
    return b"".join(parts) + bytes(1024)


image = archive(args.n, args.size)
co = zlib.compressobj(args.level, zlib.DEFLATED, 31)
gz = co.compress(image) + co.flush()


def to_device(data):
    t = torch.zeros((len(data) + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    t[:len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    return t


d_image, d_gz = to_device(image), to_device(gz)
host_entries, host_summ = compu_amd.tar_plan_host(image)
entries, summ = compu_amd.tar_plan(d_image, len(image))
assert summ.as_tuple() == host_summ.as_tuple() and summ.status == compu_amd.TarStatus.Ok and summ.n_entries == args.n, (summ, host_summ)
assert entries.cpu().numpy().tobytes() == host_entries.tobytes()

lib = compu_amd.lib()
raw = compu_amd.api._TarPlanSummary()
rows = torch.empty((args.n, 72), dtype=torch.uint8, device=dev)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def plan():
    assert lib.chip_tar_plan(C.c_void_p(d_image.data_ptr()), len(image), args.n, C.c_void_p(rows.data_ptr()), C.byref(raw), stream) == 0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def series(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = [timed(fn) for _ in range(reps)]
    return float(np.median(t)), min(t)


plan_med, plan_min = series(plan, 3, args.reps)

host = []
buf = np.frombuffer(image, np.uint8)
h_rows = np.zeros(args.n, compu_amd.tar_entry_dtype())
for _ in range(5):
    t0 = time.perf_counter()
    assert lib.chip_tar_plan_host(buf.ctypes.data_as(C.c_void_p), len(image), args.n, h_rows.ctypes.data_as(C.c_void_p), C.byref(raw)) == 0
    host.append(1e3 * (time.perf_counter() - t0))
host_med = float(np.median(host))

out = torch.empty(len(image), dtype=torch.uint8, device=dev)
res = {}


def inflate():
    res["r"] = compu_amd.inflate_parallel(compu_amd.ZlibMode.Gzip, d_gz, len(gz), out_buf=out)


inf_med, inf_min = series(inflate, 2, 5)
decoded, isumm = res["r"]
assert isumm.status == int(compu_amd.DecodeStatus.Finished) and isumm.out_len == len(image) and bool(torch.equal(decoded, d_image[:len(image)]))

headers = int(np.count_nonzero(host_entries["group_off"] != host_entries["header_off"])) + args.n
print(f"archive: {args.n} members of {args.size} B, {headers} headers, {len(image)} bytes; gzip level {args.level}: {len(gz)} bytes")
print(f"chip_tar_plan      {plan_med:.3f} ms (min {plan_min:.3f}, {args.reps} calls) = {len(image) / plan_med / 1e6:.1f} GB/s of image, "
      f"{1e3 * plan_med / args.n:.3f} us per member")
print(f"chip_tar_plan_host {host_med:.3f} ms (median of 5, host clock)")
print(f"inflate_parallel   {inf_med:.3f} ms (min {inf_min:.3f}, path {isumm.path}) of the same archive gzipped; plan / decode = {plan_med / inf_med:.3f}")
print(json.dumps({"n": args.n, "size": args.size, "image_bytes": len(image), "gzip_bytes": len(gz), "tar_plan_ms": round(plan_med, 4),
                  "tar_plan_min_ms": round(plan_min, 4), "tar_plan_host_ms": round(host_med, 4), "inflate_parallel_ms": round(inf_med, 4),
                  "inflate_path": isumm.path}))
