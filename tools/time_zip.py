"""Timing of the ZIP path: the directory plan (chip_zip_plan), chip_zip_decode over all entries, chip_crc32_batch alone over the
decoded entries, and -- the yardstick -- chip_decode_batch(CHIP_FMT_DEFLATE) over the same units alone, same process, same box:
python tools/time_zip.py [entries] [content KiB per entry] [repeats]
Builds an archive of `entries` (default 16384) deflated entries of `content KiB` (default 64) of the bench payload generator
(bench_support.synth) each, compressed by zlib at level 6 on the host, with local headers, a directory and an end record (ZIP64
records above 65 535 entries).  After two warm-up rounds, `repeats` (default 10) rounds of plan, zip decode, CRC pass, plain batch
decode, alternating, each timed with device events (the plan and the zip decode are synchronous calls, so their window is the
whole call: kernels, the waits and the host work between them).  Prints the median and the fastest of each and what the plan and
the CRC pass add to the plain decode, and checks the plan against the known offsets, the CRCs against zlib and the output against
the payload."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from compu_amd.api import _ZipDecodeSummary, _ZipPlanSummary  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
ENTRY = (int(sys.argv[2]) if len(sys.argv) > 2 else 64) * 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
lib = compu_amd.lib()

pay = synth.payloads(n * ENTRY // synth.UNIT, threads=threads) if ENTRY >= synth.UNIT else synth.payloads(n, unit_size=ENTRY, threads=threads)
packed, offs, lens = synth.deflate_units(pay, n, unit_size=ENTRY, kind="dynamic", threads=threads)
crcs = [zlib.crc32(pay[k * ENTRY:(k + 1) * ENTRY]) for k in range(n)]
parts, directory, data_off, at = [], [], [], 0
for k in range(n):
    name = b"e%07d" % k
    comp = packed[int(offs[k]):int(offs[k]) + int(lens[k])].tobytes()
    fields = struct.pack("<HHHHHIII", 20, 0, 8, 0, 0x21, crcs[k], len(comp), ENTRY)
    directory.append(b"PK\x01\x02" + struct.pack("<H", 20) + fields + struct.pack("<HHHHHII", len(name), 0, 0, 0, 0, 0, at) + name)
    parts.append(b"PK\x03\x04" + fields + struct.pack("<HH", len(name), 0) + name + comp)
    data_off.append(at + 30 + len(name))
    at += len(parts[-1])
cd = b"".join(directory)
tail = b""
if n > 0xFFFF or at > 0xFFFFFFFF:
    tail = b"PK\x06\x06" + struct.pack("<QHHIIQQQQ", 44, 45, 45, 0, 0, n, n, len(cd), at) + b"PK\x06\x07" + struct.pack("<IQI", 0, at + len(cd), 1)
tail += b"PK\x05\x06" + struct.pack("<HHHHIIH", 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), min(len(cd), 0xFFFFFFFF), min(at, 0xFFFFFFFF), 0)
archive = b"".join(parts) + cd + tail
length = len(archive)
d_in = torch.from_numpy(np.frombuffer(archive + bytes(-length % 4 + 4), np.uint8).copy()).to(dev)
d_units = torch.from_numpy(packed).to(dev)  # the yardstick's input: the units alone, as the bench lays them out
k_off, k_len = torch.from_numpy(offs.view(np.int64)).to(dev), torch.from_numpy(lens.view(np.int32)).to(dev)
lay_off = torch.arange(n, dtype=torch.int64, device=dev) * ENTRY
lay_cap = torch.full((n,), ENTRY, dtype=torch.int32, device=dev)
lay_len = torch.full((n,), ENTRY, dtype=torch.int64, device=dev)
rows = torch.zeros((n, 56), dtype=torch.uint8, device=dev)
out_off, status = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
d_out = torch.zeros(n * ENTRY, dtype=torch.uint8, device=dev)
d_ref = torch.zeros(n * ENTRY, dtype=torch.uint8, device=dev)
ps, ds = _ZipPlanSummary(), _ZipDecodeSummary()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def plan():
    rc = lib.chip_zip_plan(p(d_in), length, n, p(rows), C.byref(ps), stream)
    assert rc == 0, rc


def zip_decode():
    rc = lib.chip_zip_decode(p(d_in), length, p(rows), n, n, None, p(d_out), d_out.numel(), p(out_off), p(status), C.byref(ds), stream)
    assert rc == 0, rc


def crc_pass():
    return compu_amd.crc32_batch(d_out, lay_off, lay_len)


def plain():
    return compu_amd.decode_batch(-15, d_units, k_off, k_len, d_ref, lay_off, lay_cap)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


for _ in range(2):
    plan()
    zip_decode()
    crc_pass()
    plain()
torch.cuda.synchronize()
t_plan, t_zip, t_crc, t_plain = [], [], [], []
for _ in range(reps):
    t_plan.append(timed(plan)[0])
    t_zip.append(timed(zip_decode)[0])
    t, got_crc = timed(crc_pass)
    t_crc.append(t)
    t, (out_len, in_used, st) = timed(plain)
    t_plain.append(t)
ent = rows.cpu().numpy().reshape(-1).view(compu_amd.zip_entry_dtype())
same_plan = (ps.n_entries, ps.n_ok, ps.total_size, ps.status) == (n, n, n * ENTRY, 0) and ent["data_off"].tolist() == data_off and bool(
    (ent["status"] == 0).all())
same_zip = (ds.n_ok, ds.n_bad, ds.total_out, ds.status) == (n, 0, n * ENTRY, 0) and bool((status == 2).all()) and np.array_equal(d_out.cpu().numpy(), pay)
same_crc = got_crc.cpu().numpy().view(np.uint32).tolist() == crcs
same_plain = bool((st == 2).all()) and np.array_equal(d_ref.cpu().numpy(), pay)
med = lambda t: float(np.median(t))  # noqa: E731
pm, zm, cm, dm = med(t_plan), med(t_zip), med(t_crc), med(t_plain)
gib = n * ENTRY / 2**30
print(f"zip {n} entries x {ENTRY} B ({length} bytes of archive, {len(cd)} of directory), {reps} rounds: plan {pm:.3f} ms (min {min(t_plan):.3f}), "
      f"zip decode {zm:.3f} ms (min {min(t_zip):.3f}, {gib / zm * 1e3:.1f} GiB/s out), crc pass alone {cm:.3f} ms (min {min(t_crc):.3f}, "
      f"{gib / cm * 1e3:.1f} GiB/s), plain deflate batch {dm:.3f} ms (min {min(t_plain):.3f}, {gib / dm * 1e3:.1f} GiB/s out); plan / plain {pm / dm:.3f}, "
      f"crc / plain {cm / dm:.3f}, zip decode / plain {zm / dm:.3f}, (plan + zip decode) / plain {(pm + zm) / dm:.3f} (plan = known offsets: {same_plan}, "
      f"zip decode = payload: {same_zip}, crc = zlib: {same_crc}, plain = payload: {same_plain})", flush=True)
