"""Timing of the seekable-zstd path (chip_zstd_seek_plan, chip_zstd_seek_read, chip_xxh64_batch, chip_zstd_seek_table_write), same
process, same box:
python tools/time_zstd_seek.py [frames] [repeats] [unit bytes] [range bytes]
Builds a seekable file of `frames` (default 8192) frames of `unit bytes` (default 65 536) from the bench payload generator
(bench_support.synth) with seekable_write at level 1, checksums in the table.  After two warm-up rounds, `repeats` (default 20) rounds,
alternating, each call timed with device events around the whole call (the window holds kernels, waits and host work):
  the index     chip_zstd_seek_plan over the table alone   against   chip_zstd_plan over the whole file
  the write     chip_xxh64_batch over every chunk, and chip_zstd_seek_table_write, next to chip_encode_file of the same input
  the read      for seeded ranges of `range bytes` (default 10 000), one in each frame of a random 1/64, 1/8 and all of the frames:
                chip_zstd_seek_read with the checksums, the same with checksum NULL (chip_read_ranges), and chip_xxh64_batch alone
                over exactly the frames the read selects -- the wave-per-range hash next to the read it is part of
Prints the median and the fastest of each, and checks the verified read's bytes against the unverified one's."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from compu_amd.api import _FileSummary, _ReadSummary, _ZstdPlanSummary, _ZstdSeekSummary  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
unit = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
span = int(sys.argv[4]) if len(sys.argv) > 4 else 10000
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
lib = compu_amd.lib()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
content = n * unit


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def rounds(calls):
    """two warm-up rounds, then `reps` rounds of the calls in turn: name -> (median, fastest) in ms"""
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t[k].append(timed(fn))
    return {k: (float(np.median(v)), min(v)) for k, v in t.items()}


def show(r, k):
    return f"{r[k][0]:.3f} ms (min {r[k][1]:.3f})"


print(f"building {n} frames of {unit} B ...", flush=True)
d_pay = torch.from_numpy(synth.payloads(n, unit_size=unit, threads=threads)).to(dev)
out, fs = compu_amd.seekable_write(d_pay, content, level=1, unit_bytes=unit)
length, table_off = fs.out_len, fs.table_off
d_file = torch.zeros((length + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
d_file[:length] = out
del out
compu_amd.trim()
in_off, in_len, out_off, out_cap, cs, ps = compu_amd.zstd_seek_plan(d_file[table_off:length], length)
assert int(ps.status) == 0 and ps.n_frames == n and ps.total_out == content and ps.checksums == 1, ps
print(f"seekable zstd, {n} frames x {unit} B: {length} bytes of file, {length - table_off} of them the table, {content} bytes of content, "
      f"{reps} rounds", flush=True)

# ---- the index ------------------------------------------------------------------------------------------------------------------
arrays = [torch.zeros(n, dtype=dt, device=dev) for dt in (torch.int64, torch.int32, torch.int64, torch.int32, torch.int32)]
zs, zp = _ZstdSeekSummary(), _ZstdPlanSummary()
tail = d_file[table_off:length]


def seek_plan():
    rc = lib.chip_zstd_seek_plan(p(tail), tail.numel(), length, n, *[p(t) for t in arrays], C.byref(zs), stream)
    assert rc == 0 and zs.status == 0 and zs.n_frames == n, (rc, zs.status)


def frame_plan():
    rc = lib.chip_zstd_plan(p(d_file), length, n, *[p(t) for t in arrays[:4]], C.byref(zp), stream)
    assert rc == 0 and zp.status == 0 and zp.n_frames == n, (rc, zp.status)


r = rounds({"seek": seek_plan, "frames": frame_plan})
print(f"index: chip_zstd_seek_plan over the {tail.numel()} bytes of table {show(r, 'seek')}; chip_zstd_plan over the file {show(r, 'frames')}, "
      f"x{r['frames'][0] / r['seek'][0]:.1f}", flush=True)

# ---- the write ------------------------------------------------------------------------------------------------------------------
chunk_off = torch.arange(n, dtype=torch.int64, device=dev) * unit
chunk_len = torch.full((n,), unit, dtype=torch.int32, device=dev)
digest = torch.zeros(n, dtype=torch.int64, device=dev)
table = torch.zeros(17 + 12 * n, dtype=torch.uint8, device=dev)
enc_out = torch.zeros(compu_amd.encode_file_bound(compu_amd.FMT_ZSTD, content, unit, 0), dtype=torch.uint8, device=dev)
size, es = C.c_uint64(0), _FileSummary()


def hash_all():
    assert lib.chip_xxh64_batch(n, p(d_pay), p(chunk_off), p(chunk_len), p(digest), stream) == 0


def write_table():
    assert lib.chip_zstd_seek_table_write(n, p(in_len), p(out_cap), p(cs), p(table), table.numel(), C.byref(size), stream) == 0


def encode():
    rc = lib.chip_encode_file(compu_amd.FMT_ZSTD, 1, unit, 0, p(d_pay), content, p(enc_out), enc_out.numel(), C.byref(es), stream)
    assert rc == 0 and es.status == 0, (rc, es.status)


r = rounds({"hash": hash_all, "table": write_table, "encode": encode})
low = digest.view(torch.int32)[::2]
assert torch.equal(low, cs), "chip_xxh64_batch over the chunks differs from the table's checksums"
print(f"write: chip_xxh64_batch over {n} chunks {show(r, 'hash')} = {content / r['hash'][0] / 1e6:.1f} GB/s; chip_zstd_seek_table_write "
      f"{show(r, 'table')}; chip_encode_file of the same input {show(r, 'encode')} (the hash is {100 * r['hash'][0] / r['encode'][0]:.1f} % of it)",
      flush=True)
del enc_out

# ---- the read -------------------------------------------------------------------------------------------------------------------
for name, share in (("1/64 of the frames", 64), ("1/8 of the frames", 8), ("all frames", 1)):
    rng = np.random.default_rng(share)
    m = max(1, n // share)
    frames = rng.permutation(n)[:m].astype(np.int64)
    lo = np.minimum(frames * unit + rng.integers(0, unit, m), content - span)
    r_lo = torch.from_numpy(lo).to(dev)
    r_len = torch.full((m,), span, dtype=torch.int32, device=dev)
    total = m * span
    dst_v, dst_u = torch.zeros(total + 16, dtype=torch.uint8, device=dev), torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    dst_off, status = torch.zeros(m, dtype=torch.int64, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
    rs = _ReadSummary()
    sel = compu_amd.select_units(in_off, in_len, out_off, out_cap, r_lo, r_len)
    k = int(sel[8].n_sel)
    sel_off, sel_cap = out_off[sel[0].long()].contiguous(), sel[4]  # the selected frames' content, where it lies in the payload
    sel_digest = torch.zeros(k, dtype=torch.int64, device=dev)

    def read(checksum, dst):
        rc = lib.chip_zstd_seek_read(n, p(d_file), p(in_off), p(in_len), p(out_off), p(out_cap), checksum, m, p(r_lo), p(r_len), p(dst), total,
                                     p(dst_off), p(status), C.byref(rs), stream)
        assert rc == 0 and rs.status == 0 and rs.n_bad == 0 and rs.out_len == total and rs.n_units == k, (rc, rs.status, rs.n_bad, rs.out_len)

    def hash_selected():
        assert lib.chip_xxh64_batch(k, p(d_pay), p(sel_off), p(sel_cap), p(sel_digest), stream) == 0

    r = rounds({"verified": lambda: read(p(cs), dst_v), "plain": lambda: read(None, dst_u), "hash": hash_selected})
    same = bool(torch.equal(dst_v[:total], dst_u[:total]))
    extra = r["verified"][0] - r["plain"][0]
    print(f"{name}: {m} ranges of {span} B, {k} of {n} frames decoded: chip_zstd_seek_read verified {show(r, 'verified')}, checksum NULL "
          f"{show(r, 'plain')}: the check costs {extra:.3f} ms = {100 * extra / r['verified'][0]:.1f} % of the verified read; chip_xxh64_batch alone "
          f"over the {k} frames' content {show(r, 'hash')} = {k * unit / r['hash'][0] / 1e6:.1f} GB/s (same bytes: {same})", flush=True)
