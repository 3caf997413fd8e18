"""Timing of the tar writer (chip_tar_write), same process, same box:
python tools/time_tar_write.py [members] [content KiB per member] [repeats] [flags]
The shape tools/time_tar.py reads: `members` (default 16 384) members of `content KiB` (default 16) of the bench payload generator
(bench_support.synth) each, every eighth with a name above 100 bytes that has no place for a prefix split (a pax path record, or a GNU
L header with flags 1).  After two warm-up rounds, `repeats` (default 10) rounds of every measurement, alternating, each timed with
device events (the writer's calls are synchronous, so their window is the whole call: kernels, the waits and the host work between
them):
  tar_write            the whole call into a buffer that is there
  sizing call          the same call without room and without an entries array: check, scan and the first wait, nothing else
  entries call         without room, with the entries array: the sizing call and the headers kernel writing entries[] only
  pack_units           chip_pack_units over the same content ranges: the floor, one read and one write of the content bytes
  tar_write_host       chip_tar_write_host over the same arrays in host memory (host clock, median of three)
and derived from them: headers + copy + second wait = tar_write - sizing call.  The kernels one by one are a profiler's to give
(rocprofv3 --kernel-trace --stats -- python tools/time_tar_write.py): tw_check_kernel, the two scan kernels, tw_headers_kernel,
tw_copy_kernel.  The device image is compared with the host image, read by tarfile (a sample of members) and planned by chip_tar_plan
before anything is reported.  Needs the GPU."""
import ctypes as C
import io
import json
import os
import sys
import tarfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
SIZE = (int(sys.argv[2]) if len(sys.argv) > 2 else 16) * 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
flags = int(sys.argv[4]) if len(sys.argv) > 4 else 0
assert torch.cuda.is_available(), "time_tar_write.py measures on the GPU"
dev = torch.device("cuda:0")
threads = min(16, len(os.sched_getaffinity(0)))

pay = np.asarray(synth.payloads(-(-max(n * SIZE, 1) // synth.UNIT), threads=threads)).reshape(-1)[:n * SIZE]
src = np.zeros(n, compu_amd.tar_source_dtype())
names = bytearray()
for k in range(n):
    name = b"shard/%08d.bin" % k if k % 8 != 7 else b"shard/" + b"deep_" * 24 + b"%08d.bin" % k
    src[k] = (k * SIZE, SIZE, len(names), 0, 1700000000, len(name), 0, 0o644, 1000, 1000, ord("0"), (0, 0, 0))
    names += name
names = bytes(names)
d_src = torch.from_numpy(src.view(np.uint8).reshape(-1, 64).copy()).to(dev)
d_names = torch.from_numpy(np.frombuffer(names, np.uint8).copy()).to(dev)
d_content = torch.from_numpy(np.ascontiguousarray(pay)).to(dev)
room = compu_amd.tar_write_bound(n, len(names), n * SIZE)
d_out = torch.zeros(room, dtype=torch.uint8, device=dev)
d_packed = torch.zeros(n * SIZE, dtype=torch.uint8, device=dev)
in_off = torch.arange(n, dtype=torch.int64, device=dev) * SIZE
in_len = torch.full((n,), SIZE, dtype=torch.int32, device=dev)
state = {}

lib = compu_amd.lib()
raw = compu_amd.api._TarWriteSummary()
rows = torch.empty((n, 72), dtype=torch.uint8, device=dev)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def write():
    state["write"] = compu_amd.tar_write(d_src, d_names, d_content, flags=flags, out=d_out)


def sizing(entries):
    def run():
        assert lib.chip_tar_write(n, P(d_src), P(d_names), len(names), P(d_content), n * SIZE, flags, 0, None, 0, P(rows) if entries else None, C.byref(raw),
                                  stream) == 0 and raw.status == compu_amd.TarWriteStatus.NeedOutput

    return run


def pack():
    state["pack"] = compu_amd.pack_units(d_content, in_off, in_len, d_packed)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


steps = [("tar_write", write), ("sizing call", sizing(False)), ("entries call", sizing(True)), ("pack_units", pack)]
for _ in range(2):
    for _, fn in steps:
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in steps}
for _ in range(reps):
    for name, fn in steps:
        times[name].append(timed(fn))

host = []
for _ in range(3):
    t0 = time.perf_counter()
    h_image, h_entries, h_summ = compu_amd.tar_write_host(src, names, pay, flags=flags, out_cap=room)
    host.append(1e3 * (time.perf_counter() - t0))
image, entries, summ = state["write"]
same = summ.as_tuple() == h_summ.as_tuple() and image.cpu().numpy().tobytes() == h_image and entries.cpu().numpy().tobytes() == h_entries.tobytes()
with tarfile.open(fileobj=io.BytesIO(h_image), mode="r:") as tf:
    infos = tf.getmembers()
    sample = sorted({0, 7, n // 2, n - 1})
    readable = len(infos) == n and all(np.array_equal(np.frombuffer(tf.extractfile(infos[k]).read(), np.uint8), pay[k * SIZE:(k + 1) * SIZE]) for k in sample)
planned, psumm = compu_amd.tar_plan(image, summ.out_len)
plan_same = psumm.status == compu_amd.TarStatus.Ok and planned.cpu().numpy().tobytes() == h_entries.tobytes()
med = {k: float(np.median(v)) for k, v in times.items()}
mn = {k: min(v) for k, v in times.items()}
host_med = float(np.median(host))
rest = med["tar_write"] - med["sizing call"]
print(f"tar write {n} members x {SIZE} B, flags {flags} -> {summ.out_len} bytes, {summ.n_ext} extension headers, {reps} rounds: "
      + ", ".join(f"{k} {med[k]:.3f} ms (min {mn[k]:.3f})" for k, _ in steps)
      + f"; headers + copy + second wait {rest:.3f} ms; tar_write_host {host_med:.1f} ms (host clock, includes the face's copies); "
      f"tar_write {summ.out_len / med['tar_write'] / 1e6:.1f} GB/s of image, pack_units {n * SIZE / med['pack_units'] / 1e6:.1f} GB/s of content; "
      f"tar_write / pack_units {med['tar_write'] / med['pack_units']:.2f} (device image equals the host image: {same}, tarfile reads {len(sample)} "
      f"sampled members: {readable}, chip_tar_plan gives the answered entries: {plan_same})", flush=True)
print(json.dumps({"n": n, "size": SIZE, "flags": flags, "image_bytes": summ.out_len, "n_ext": summ.n_ext, "tar_write_ms": round(med["tar_write"], 4),
                  "tar_write_min_ms": round(mn["tar_write"], 4), "sizing_ms": round(med["sizing call"], 4), "entries_ms": round(med["entries call"], 4),
                  "pack_units_ms": round(med["pack_units"], 4), "pack_units_min_ms": round(mn["pack_units"], 4), "tar_write_host_ms": round(host_med, 2),
                  "same": bool(same and readable and plan_same)}))
