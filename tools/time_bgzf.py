"""Timing of the BGZF plan (chip_bgzf_plan) against the chip_decode_batch(CHIP_FMT_GZIP) of the same blocks, same process, same box:
python tools/time_bgzf.py [blocks] [repeats]
Builds a BGZF file of `blocks` (default 65536) blocks of 65 280 payload bytes from the bench payload generator (bench_support.synth),
compressed with the system zlib at level 6 on the host, plus the EOF marker.  After two warm-up rounds, `repeats` (default 10) rounds of
plan, then decode, alternating, each timed with device events (the plan call is synchronous, so its window is the whole call: kernels,
the two waits and the host work between them).  Prints the median and the fastest of each, the ratio plan / decode, the number of
header candidates in the file, and checks the plan against chip_bgzf_plan_host and the decoded bytes against the payload."""
import ctypes as C
import os
import struct
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from compu_amd.api import _BgzfSummary  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
PAYLOAD = 65280
HEAD, FIXED = b"\x1f\x8b\x08\x04", b"\x06\x00BC\x02\x00"
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
lib = compu_amd.lib()

pay = synth.payloads(n, unit_size=PAYLOAD, threads=threads)
mv = memoryview(pay)


def one_block(i):
    data = mv[i * PAYLOAD:(i + 1) * PAYLOAD]
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    size = 18 + len(body) + 8
    assert size <= 65536
    return HEAD + b"\x00\x00\x00\x00\x00\xff" + FIXED + struct.pack("<H", size - 1) + body + struct.pack("<II", zlib.crc32(data), PAYLOAD)


with ThreadPoolExecutor(threads) as ex:
    parts = list(ex.map(one_block, range(n), chunksize=64))
data = b"".join(parts) + compu_amd.bgzf_eof_block()
del parts
length = len(data)
candidates, at = 0, data.find(HEAD)
while at >= 0:
    candidates += at + 18 <= length and data[at + 10:at + 16] == FIXED
    at = data.find(HEAD, at + 1)
h_off, h_len, h_ooff, h_cap, h_sum = compu_amd.bgzf_plan_host(data)
host = np.zeros((length + 3) // 4 * 4, np.uint8)
host[:length] = np.frombuffer(data, np.uint8)
d_in = torch.from_numpy(host).to(dev)
del data, host
m = n + 1
in_off, out_off = torch.zeros(m, dtype=torch.int64, device=dev), torch.zeros(m, dtype=torch.int64, device=dev)
in_len, out_cap = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
d_out = torch.zeros(n * PAYLOAD, dtype=torch.uint8, device=dev)
summ = _BgzfSummary()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def plan():
    rc = lib.chip_bgzf_plan(p(d_in), length, m, p(in_off), p(in_len), p(out_off), p(out_cap), C.byref(summ), stream)
    assert rc == 0, rc


def decode():
    return compu_amd.decode_batch(31, d_in, in_off, in_len, d_out, out_off, out_cap)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


for _ in range(2):
    plan()
    decode()
torch.cuda.synchronize()
t_plan, t_dec = [], []
for _ in range(reps):
    t_plan.append(timed(plan)[0])
    t, (out_len, in_used, status) = timed(decode)
    t_dec.append(t)
same_plan = (summ.n_blocks, summ.total_out, summ.in_used, summ.status, summ.eof) == h_sum.as_tuple() and all(
    np.array_equal(g.cpu().numpy().view(w.dtype), w) for g, w in ((in_off, h_off), (in_len, h_len), (out_off, h_ooff), (out_cap, h_cap)))
same_bytes = bool((status == 2).all()) and np.array_equal(d_out.cpu().numpy(), pay)
pm, dm = float(np.median(t_plan)), float(np.median(t_dec))
print(f"bgzf {n} blocks x {PAYLOAD} B ({length} bytes of BGZF, {candidates} header candidates), {reps} rounds: plan {pm:.3f} ms (min {min(t_plan):.3f}), "
      f"decode {dm:.3f} ms (min {min(t_dec):.3f}), ratio {pm / dm:.3f} (plan = host plan: {same_plan}, decoded = payload: {same_bytes})", flush=True)
