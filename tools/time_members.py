"""The price of serialising k members on one wave (CHIP_F_MEMBERS) against the same members as units of their own, same process, same box:
python tools/time_members.py [members] [launches]
`members` (default 16384) gzip members, and as many zstd frames, of 16 KiB of decoded text each are decoded three ways: as that many
single-member units without the flag, and as members / k units of k members each with the flag, k = 4 and k = 64.  hipEvent timing of
`launches` (default 20) launches of each after two warm-up launches; prints the median and the fastest, and the ratio to the unflagged
time of the same run.  The outputs of the three ways are compared byte for byte."""
import os, sys, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import compu_amd
from bench_support import synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
MEMBER = 16384
assert n % 64 == 0
dev = torch.device("cuda:0")
threads = min(16, len(os.sched_getaffinity(0)))
pay = memoryview(synth.payloads(n * MEMBER // synth.UNIT, threads=threads))


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), min(ts), r


def gzip_member(i):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(pay[i * MEMBER:(i + 1) * MEMBER]) + c.flush()


def zstd_frame(i):
    return synth._mixed_one((pay[i * MEMBER:(i + 1) * MEMBER], zstd_frame.idx[i]))


def zstd_indices():
    idx, i = [], 0
    while len(idx) < n:
        if not (synth._splitmix64(i) & 1):
            idx.append(i)
        i += 1
    return idx


from concurrent.futures import ThreadPoolExecutor
for kind, fmt, make in (("gzip", 31, gzip_member), ("zstd", 100, zstd_frame)):
    if kind == "zstd":
        zstd_frame.idx = zstd_indices()
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(make, range(n)))
    lens1 = np.array([len(p) for p in parts], np.int64)
    total = int(lens1.sum())
    buf = np.zeros((total + 7) & ~3, np.uint8); buf[:total] = np.frombuffer(b"".join(parts), np.uint8)
    d_in = torch.from_numpy(buf).to(dev)
    starts = np.zeros(n + 1, np.int64); starts[1:] = np.cumsum(lens1)
    d_out = torch.zeros(n * MEMBER, dtype=torch.uint8, device=dev)
    base = None
    for k in (1, 4, 64):
        m = n // k
        offs = torch.from_numpy(starts[:-1:k].copy()).to(dev)
        lens = torch.from_numpy((starts[k::k] - starts[:-1:k]).astype(np.int32)).to(dev)
        ooff = torch.arange(m, dtype=torch.int64, device=dev) * (k * MEMBER)
        caps = torch.full((m,), k * MEMBER, dtype=torch.int32, device=dev)
        flags = compu_amd.F_MEMBERS if k > 1 else 0
        d_out.zero_()
        med, fastest, (ol, iu, st) = timed(lambda: compu_amd.decode_batch(fmt, d_in, offs, lens, d_out, ooff, caps, flags=flags))
        ok = bool((st == 2).all()) and bool((ol == k * MEMBER).all()) and torch.equal(iu, lens)
        if base is None:
            base, ref = med, d_out.clone()
        ok = ok and torch.equal(ref, d_out)
        print(f"{kind:5s} {n} members of {MEMBER} B as {m} units of {k}{' (no flag)' if k == 1 else ''}, {reps} launches: {med:.3f} ms (min {fastest:.3f}), "
              f"x{med / base:.2f} of the unflagged time (right answers={ok})", flush=True)
    del d_in, buf
