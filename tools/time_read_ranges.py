"""Timing of the range reader (chip_read_ranges, chip_select_units), same process, same box:
python tools/time_read_ranges.py [blocks] [repeats] [range bytes]
Builds a BGZF file of `blocks` (default 65536) blocks of 65 280 payload bytes from the bench payload generator (bench_support.synth)
with chip_encode_file at level 6, plans it, and draws seeded ranges of `range bytes` (default 10 000) bytes, one in each block of
a random subset of the blocks (a range may run on into the next block), in random order.  Three subsets: about 1/64, 1/8 and all of
the blocks.  Per subset, after two warm-up rounds, `repeats` (default 20) rounds of three calls, alternating, each timed with
device events around the whole call (all three are synchronous, so the window holds kernels, waits and host work):
  chip_read_ranges                       select, decode the touched blocks, gather
  the path at hand without it            chip_decode_batch over the whole plan, then chip_pack_units with the ranges as sources
  chip_select_units                      the selection alone, sub-batch arrays included
Prints the median and the fastest of each and the units decoded, and checks the reader's bytes against the baseline's."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from compu_amd.api import _ReadSummary, _SelectSummary  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
span = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
PAYLOAD = 65280
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
lib = compu_amd.lib()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

content = n * PAYLOAD
print(f"building {n} blocks ...", flush=True)
d_pay = torch.from_numpy(synth.payloads(n, unit_size=PAYLOAD, threads=threads)).to(dev)
out, fs = compu_amd.encode_file(compu_amd.FMT_BGZF, 6, d_pay, content)
length = fs.out_len
d_file = torch.zeros((length + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)  # (4-byte aligned and padded, the bound's slack given back)
d_file[:length] = out
del out, d_pay
compu_amd.trim()  # the writer's slot area is not needed any more
in_off, in_len, out_off, out_cap, ps = compu_amd.bgzf_plan(d_file, length)
assert ps.n_blocks == n + 1 and ps.total_out == content and int(ps.status) == 0, ps
units = n + 1
d_out = torch.zeros(content, dtype=torch.uint8, device=dev)
o_len, o_used, o_status = (torch.zeros(units, dtype=torch.int32, device=dev) for _ in range(3))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def sweep(name, share):
    rng = np.random.default_rng(share)
    m = max(1, n // share)
    blocks = rng.permutation(n)[:m].astype(np.int64)
    lo = blocks * PAYLOAD + rng.integers(0, PAYLOAD, m)
    lo = np.minimum(lo, content - span)
    r_lo = torch.from_numpy(lo).to(dev)
    r_len = torch.full((m,), span, dtype=torch.int32, device=dev)
    total = m * span
    dst_read, dst_base = torch.zeros(total + 16, dtype=torch.uint8, device=dev), torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    dst_off, status = torch.zeros(m, dtype=torch.int64, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
    base_off = torch.zeros(m, dtype=torch.int64, device=dev)
    sel = [torch.zeros(units, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int32, torch.int64, torch.int32)]
    src_off = torch.zeros(m, dtype=torch.int64, device=dev)
    rs, ss, got = _ReadSummary(), _SelectSummary(), C.c_uint64(0)

    def read():
        rc = lib.chip_read_ranges(31, units, p(d_file), p(in_off), p(in_len), p(out_off), p(out_cap), m, p(r_lo), p(r_len), p(dst_read), total,
                                  p(dst_off), p(status), C.byref(rs), stream)
        assert rc == 0 and rs.status == 0 and rs.n_bad == 0 and rs.out_len == total, (rc, rs.status, rs.n_bad, rs.out_len)

    def baseline():
        rc = lib.chip_decode_batch(31, units, p(d_file), p(in_off), p(in_len), p(d_out), p(out_off), p(out_cap), p(o_len), p(o_used), p(o_status), stream)
        assert rc == 0, rc
        rc = lib.chip_pack_units(m, p(d_out), p(r_lo), p(r_len), p(dst_base), total, p(base_off), C.byref(got), stream)
        assert rc == 0 and got.value == total, (rc, got.value)

    def select():
        rc = lib.chip_select_units(units, p(in_off), p(in_len), p(out_off), p(out_cap), m, p(r_lo), p(r_len), units, *[p(t) for t in sel], p(src_off),
                                   p(dst_off), p(status), C.byref(ss), stream)
        assert rc == 0 and ss.status == 0, (rc, ss.status)

    for _ in range(2):
        read(), baseline(), select()
    torch.cuda.synchronize()
    t = {"read": [], "base": [], "sel": []}
    for _ in range(reps):
        t["read"].append(timed(read))
        t["base"].append(timed(baseline))
        t["sel"].append(timed(select))
    same = bool(torch.equal(dst_read[:total], dst_base[:total])) and bool((o_status == 2).all()) and ss.n_sel == rs.n_units
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"{name}: {m} ranges of {span} B = {total} bytes, {rs.n_units} of {n} blocks decoded: chip_read_ranges {med['read']:.3f} ms "
          f"(min {min(t['read']):.3f}), decode all + chip_pack_units {med['base']:.3f} ms (min {min(t['base']):.3f}), x{med['base'] / med['read']:.2f}; "
          f"chip_select_units alone {med['sel']:.3f} ms (min {min(t['sel']):.3f}) = {100 * med['sel'] / med['read']:.1f} % of the read "
          f"(same bytes: {same})", flush=True)


print(f"bgzf {n} blocks x {PAYLOAD} B: {length} bytes of BGZF, {content} bytes of content, {reps} rounds", flush=True)
for name, share in (("1/64 of the blocks", 64), ("1/8 of the blocks", 8), ("all blocks", 1)):
    sweep(name, share)
