"""Timing of the size pass (chip_decode_batch_sizes) against chip_decode_batch of the same batch, same process, same box:
python tools/time_sizes.py [units] [launches]
hipEvent timing of `launches` (default 20) launches of each after two warm-up launches; prints the median and the fastest per kind
(dynamic, fixed, stored, zstd, mixed = gzip + zstd through CHIP_FMT_DETECT: synthetic 64 KiB units as bench.py builds them) and the ratio size pass / decode.
With SSTATS=1 and a -DCHIP_STATS build (COMPU_HIP_LIB=compu_amd/libcompu_hip_stats.so) it also prints the kernels' own cycle counters per
unit, decode beside size pass (inflate_unit.h's stat slots; zstd_unit.h's ZT_* / ZC); the timings of that build are not the product's."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import compu_amd
from bench_support import synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda:0")
threads = min(16, len(os.sched_getaffinity(0)))
pay = synth.payloads(n, threads=threads)
d_out = torch.zeros(n * synth.UNIT, dtype=torch.uint8, device=dev)
ooff = torch.arange(n, dtype=torch.int64, device=dev) * synth.UNIT
caps = torch.full((n,), synth.UNIT, dtype=torch.int32, device=dev)


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


def zstd_units():
    """every unit as a zstd frame: the mixed layout's own frames (the indices its generator turns into zstd)"""
    from concurrent.futures import ThreadPoolExecutor
    mv = memoryview(pay)
    idx, i = [], 0
    while len(idx) < n:
        if not (synth._splitmix64(i) & 1):
            idx.append(i)
        i += 1
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(synth._mixed_one, [(mv[k * synth.UNIT:(k + 1) * synth.UNIT], idx[k]) for k in range(n)]))
    lens = np.array([len(p) for p in parts], np.int32)
    offs = np.zeros(n, np.int64); offs[1:] = np.cumsum(lens[:-1].astype(np.int64))
    total = int(lens.astype(np.int64).sum())
    buf = np.zeros((total + 7) & ~3, np.uint8); buf[:total] = np.frombuffer(b"".join(parts), np.uint8)
    return buf, offs, lens


for kind in ("dynamic", "fixed", "stored", "zstd", "mixed"):
    fmt = {"zstd": 100, "mixed": 0}.get(kind, -15)
    if kind == "zstd":
        packed, offs, lens = zstd_units()
    elif kind == "mixed":
        packed, offs, lens = synth.mixed_units(pay, n, threads=threads)
    else:
        packed, offs, lens = synth.deflate_units(pay, n, kind=kind, threads=threads)
    d_in, d_off, d_len = torch.from_numpy(packed).to(dev), torch.from_numpy(offs.astype(np.int64)).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
    d_med, d_min, (ol, iu, st) = timed(lambda: compu_amd.decode_batch(fmt, d_in, d_off, d_len, d_out, ooff, caps))
    s_med, s_min, (size, used, sst) = timed(lambda: compu_amd.decode_batch_sizes(fmt, d_in, d_off, d_len))
    ok = bool((st == 2).all()) and bool((sst == 2).all()) and torch.equal(size, ol.to(torch.int64)) and torch.equal(used, iu)
    if os.environ.get("SSTATS") == "1" and kind != "mixed":
        stats = torch.zeros(n * 24, dtype=torch.int64, device=dev)
        os.environ["CHIP_STATS_PTR"] = str(stats.data_ptr())
        rows = []
        for fn in (lambda: compu_amd.decode_batch(fmt, d_in, d_off, d_len, d_out, ooff, caps), lambda: compu_amd.decode_batch_sizes(fmt, d_in, d_off, d_len)):
            stats.zero_(); fn(); torch.cuda.synchronize()
            rows.append(stats.cpu().numpy().reshape(n, 24).astype(np.float64).mean(axis=0))
        del os.environ["CHIP_STATS_PTR"]
        if kind == "zstd":
            names = {0: "whole frame", 1: "Huffman literals", 3: "FSE state chain", 4: "sequence chunks altogether", 5: "phase A", 6: "phase B", 7: "XXH64",
                     13: "Huffman table", 14: "sequence tables"}
        else:
            names = {0: "header other", 1: "window load", 2: "walk", 3: "path resolve", 4: "code lengths", 5: "table build", 6: "trailer / checksum",
                     16: "flush: token groups", 17: "flush: match rounds", 18: "flush: chunk store", 20: "flush rest (size pass: count_tokens)"}
        for i in sorted(names):
            print(f"    cycles per unit, {names[i]:40s} decode {rows[0][i]:11.0f}   size pass {rows[1][i]:11.0f}", flush=True)
    print(f"{kind:8s} {n} units x {synth.UNIT} B, {reps} launches: decode {d_med:.3f} ms (min {d_min:.3f}), size pass {s_med:.3f} ms (min {s_min:.3f}), "
          f"ratio {s_med / d_med:.3f} (same answers={ok})", flush=True)
    del d_in, packed
