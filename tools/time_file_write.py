"""Timing of the file writer (chip_pack_units, chip_encode_file), same process, same box:
python tools/time_file_write.py [input MiB] [repeats] [bgzf level] [zstd level]
Pack: three shapes -- 16 384 units of about 64 KiB, 64 units of 16 MiB, 262 144 units of 100 bytes -- and 1 KiB in 64 units (what
a call costs whatever it moves: five launches and two waits), of random bytes in slots, the source ranges at every alignment;
chip_pack_units into a buffer of exactly the total against a plain device-to-device copy
(Tensor.copy_) of the same number of bytes, `repeats` (default 10) rounds each after two warm-up rounds, alternating, timed with
device events.  chip_pack_units is synchronous, so its window is the whole call: the scan, the wait for the total, the copy and
the wait behind it; the copy kernel alone is not timed separately.  Prints GB/s of bytes moved (read + written = 2 x total) for
both and the ratio of the times; the packed bytes are checked against a masked select of the slots.
Writer: `input MiB` (default 512) of the bench payload generator (bench_support.synth) through chip_encode_file against
chip_encode_batch alone on the same cuts -- BGZF with 65 280-byte units (level default 6), zstd with 64 KiB, 256 KiB and 1 MiB
units (level default 3), with the seek table.  The batch call only enqueues: its window ends at the kernel's end.  The
difference is what the arrays, the packing, the trailer and the two waits cost.  The file is checked against gzip / the plan.
Last, once: the path this replaces at 4 096 BGZF blocks -- out_len to the host, torch.cat of one slice per block and the EOF
block -- against chip_encode_file's packing of the same blocks, wall clock."""
import ctypes as C
import gzip
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402

in_mib = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
bgzf_level = int(sys.argv[3]) if len(sys.argv) > 3 else 6
zstd_level = int(sys.argv[4]) if len(sys.argv) > 4 else 3
dev = torch.device("cuda:0")
lib = compu_amd.lib()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def median_of(fn_a, fn_b):
    for _ in range(2):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fn_a)[0])
        tb.append(timed(fn_b)[0])
    return float(np.median(ta)), min(ta), float(np.median(tb)), min(tb)


# ---- pack ----------------------------------------------------------------------------------------------------------------------
def pack_shape(name, n, slot, lens):
    gen = torch.Generator(device=dev).manual_seed(n)
    src = torch.randint(0, 256, (n * slot + 64,), dtype=torch.uint8, device=dev, generator=gen)
    shift = torch.arange(n, dtype=torch.int64, device=dev) % 16  # every source alignment
    src_off = torch.arange(n, dtype=torch.int64, device=dev) * slot + shift
    src_len = lens.to(torch.int32)
    total = int(lens.sum())
    dst = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    dst_off = torch.zeros(n, dtype=torch.int64, device=dev)
    plain_src = src[:total]
    plain_dst = torch.zeros(total, dtype=torch.uint8, device=dev)
    got = C.c_uint64(0)

    def pack():
        rc = lib.chip_pack_units(n, p(src), p(src_off), p(src_len), p(dst), total, p(dst_off), C.byref(got), stream)
        assert rc == 0 and got.value == total, (rc, got.value)

    pm, pmin, cm, cmin = median_of(pack, lambda: plain_dst.copy_(plain_src))
    # the expected bytes: unit i is slot i from its shift on
    ok = True
    rows = max(1, (256 << 20) // slot)
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        view = src[r0 * slot:r1 * slot].view(r1 - r0, slot)
        col = torch.arange(slot, device=dev)[None, :] - shift[r0:r1, None]
        want = view[(col >= 0) & (col < lens[r0:r1, None])]
        a = int(dst_off[r0])
        ok = ok and bool(torch.equal(dst[a:a + want.numel()], want))
        del view, col, want
    print(f"pack {name}: {n} units, {total} bytes: chip_pack_units {pm:.3f} ms (min {pmin:.3f}) = {2 * total / pm / 1e6:.0f} GB/s, "
          f"device-to-device copy {cm:.3f} ms (min {cmin:.3f}) = {2 * total / cm / 1e6:.0f} GB/s, pack / copy {pm / cm:.2f} "
          f"(packed = the slots' bytes: {ok})", flush=True)


g = torch.Generator(device=dev).manual_seed(1)
pack_shape("64 KiB units", 16384, 65536 + 64, torch.randint(63000, 65537, (16384,), device=dev, generator=g))
pack_shape("16 MiB units", 64, (16 << 20) + 64, torch.full((64,), 16 << 20, dtype=torch.int64, device=dev))
pack_shape("100-byte units", 262144, 128, torch.full((262144,), 100, dtype=torch.int64, device=dev))
pack_shape("the call's floor, 64 units of 16 bytes", 64, 32, torch.full((64,), 16, dtype=torch.int64, device=dev))

# ---- writer --------------------------------------------------------------------------------------------------------------------
length = in_mib << 20
threads = min(16, len(os.sched_getaffinity(0)))
pay = np.asarray(synth.payloads(length // synth.UNIT, threads=threads))
d_in = torch.from_numpy(pay).to(dev)


def writer(name, fmt, level, unit, flags):
    n = (length + unit - 1) // unit
    slot = (compu_amd.encode_bound(fmt, unit) + 15) // 16 * 16
    in_off = torch.arange(n, dtype=torch.int64, device=dev) * unit
    in_len = torch.clamp(length - in_off, max=unit).to(torch.int32)
    out_off = torch.arange(n, dtype=torch.int64, device=dev) * slot
    out_cap = torch.full((n,), slot, dtype=torch.int32, device=dev)
    slots = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    out_len, status = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    bound = compu_amd.encode_file_bound(fmt, length, unit, flags)
    d_file = torch.zeros(bound + 16, dtype=torch.uint8, device=dev)
    res = {}

    def batch():
        compu_amd.encode_batch(fmt, level, d_in, in_off, in_len, slots, out_off, out_cap, out_len, status)

    def file():
        res["file"] = compu_amd.encode_file(fmt, level, d_in, length, unit, flags, out=d_file[:bound])

    fm, fmin, bm, bmin = median_of(file, batch)
    out, summ = res["file"]
    same = summ.n_units == n and bool((status == 2).all()) and summ.table_off == int(out_len.sum()) + (28 if fmt == compu_amd.FMT_BGZF else 0)
    if fmt == compu_amd.FMT_BGZF:
        head = out[:int(out_len[:4].sum())].cpu().numpy().tobytes()
        same = same and gzip.decompress(head) == bytes(memoryview(pay)[:4 * unit])
        same = same and compu_amd.bgzf_plan(d_file, summ.out_len)[4].as_tuple() == (n + 1, length, summ.out_len, 0, 1)
    else:
        plan = compu_amd.zstd_plan(d_file, summ.out_len)[4]
        same = same and (plan.n_frames, plan.n_skippable, plan.total_out, plan.in_used, int(plan.status)) == (n, 1 if flags else 0, length, summ.out_len, 0)
    print(f"writer {name}: {n} units of {unit} B, {length} -> {summ.out_len} bytes: chip_encode_file {fm:.3f} ms (min {fmin:.3f}), "
          f"chip_encode_batch alone {bm:.3f} ms (min {bmin:.3f}), difference {fm - bm:.3f} ms = {100 * (fm - bm) / bm:.1f} % (checked: {same})", flush=True)


writer(f"bgzf level {bgzf_level}", compu_amd.FMT_BGZF, bgzf_level, 65280, 0)
for kib in (64, 256, 1024):
    writer(f"zstd level {zstd_level}, {kib} KiB", compu_amd.FMT_ZSTD, zstd_level, kib << 10, compu_amd.W_SEEK_TABLE)

# ---- the path this replaces: one slice per block through torch.cat -----------------------------------------------------------
n = 4096
part = n * 65280
assert part <= length
in_off = torch.arange(n, dtype=torch.int64, device=dev) * 65280
in_len = torch.full((n,), 65280, dtype=torch.int32, device=dev)
slot = (compu_amd.encode_bound(compu_amd.FMT_BGZF, 65280) + 15) // 16 * 16
out_off = torch.arange(n, dtype=torch.int64, device=dev) * slot
out_cap = torch.full((n,), slot, dtype=torch.int32, device=dev)
slots = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
eof = torch.frombuffer(bytearray(compu_amd.bgzf_eof_block()), dtype=torch.uint8).to(dev)
out_len, status = compu_amd.encode_batch(compu_amd.FMT_BGZF, bgzf_level, d_in, in_off, in_len, slots, out_off, out_cap)
torch.cuda.synchronize()


def cat_path():
    lens = out_len.tolist()
    offs = out_off.tolist()
    return torch.cat([slots[o:o + ln] for o, ln in zip(offs, lens)] + [eof])


def pack_path():
    dst, _, total = compu_amd.pack_units(slots, out_off, out_len)
    return dst


for fn in (cat_path, pack_path):
    fn()
torch.cuda.synchronize()
t0 = time.perf_counter()
a = cat_path()
torch.cuda.synchronize()
t1 = time.perf_counter()
b = pack_path()
torch.cuda.synchronize()
t2 = time.perf_counter()
print(f"{n} BGZF blocks laid end to end: torch.cat of one slice per block {1e3 * (t1 - t0):.3f} ms, pack_units (two calls: size, fill) "
      f"{1e3 * (t2 - t1):.3f} ms, x{(t1 - t0) / (t2 - t1):.1f} (same bytes: {bool(torch.equal(a[:-28], b))})", flush=True)
