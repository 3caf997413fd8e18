"""Timing of the gzip member index (chip_gzip_plan), of the plain size pass (chip_decode_batch_sizes) over the same members with
known arrays, of the chip_decode_batch(CHIP_FMT_GZIP) of the plan's arrays, and of the same bytes as ONE CHIP_FMT_GZIP unit with
CHIP_F_MEMBERS, same process, same box:
python tools/time_gzip_plan.py [members] [content KiB per member] [repeats] [MiB of members in the single unit]
Builds a buffer of `members` (default 16384) gzip members of `content KiB` (default 64) of the bench payload generator
(bench_support.synth) each, compressed by zlib at level 6 on the host.  After two warm-up rounds, `repeats` (default 10) rounds of
plan, size pass, batch decode, alternating, each timed with device events (the plan call is synchronous, so its window is the whole
call: kernels, the two waits and the host work between them).  The single unit is one wave walking every member: it is timed once,
after a warm-up on the first member alone, over the longest run of whole members from position 0 that fits `MiB` (default 64, at
most 511) of compressed bytes and 4 GiB - 1 of output.  Prints the median and the fastest of each, the number of candidates, and
checks the plan against the known arrays and both outputs against the payload."""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from compu_amd.api import _GzipPlanSummary  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
MEMBER = (int(sys.argv[2]) if len(sys.argv) > 2 else 64) * 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
unit_mib = min(int(sys.argv[4]) if len(sys.argv) > 4 else 64, 511)
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
lib = compu_amd.lib()
GZIP = int(compu_amd.ZlibMode.Gzip)

pay = synth.payloads(n * MEMBER // synth.UNIT, threads=threads) if MEMBER >= synth.UNIT else synth.payloads(n, unit_size=MEMBER, threads=threads)
packed, offs, lens = synth.deflate_units(pay, n, unit_size=MEMBER, kind="dynamic", wbits=31, threads=threads)
length = int(lens.sum(dtype=np.uint64))
candidates = len(re.findall(rb"(?=\x1f\x8b\x08[\x00-\x1f])", packed[:length].tobytes()))
d_in = torch.from_numpy(packed).to(dev)
k_off = torch.from_numpy(offs.view(np.int64)).to(dev)  # the known arrays: what a caller who wrote the members holds
k_len = torch.from_numpy(lens.view(np.int32)).to(dev)
in_off, out_off = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
in_len, out_cap = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
s_size, s_used, s_status = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
d_out = torch.zeros(n * MEMBER, dtype=torch.uint8, device=dev)
summ = _GzipPlanSummary()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def plan():
    rc = lib.chip_gzip_plan(p(d_in), length, n, p(in_off), p(in_len), p(out_off), p(out_cap), C.byref(summ), stream)
    assert rc == 0, rc


def sizes():
    return compu_amd.decode_batch_sizes(GZIP, d_in, k_off, k_len, s_size, s_used, s_status)


def decode():
    return compu_amd.decode_batch(GZIP, d_in, in_off, in_len, d_out, out_off, out_cap)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


for _ in range(2):
    plan()
    sizes()
    decode()
torch.cuda.synchronize()
t_plan, t_size, t_dec = [], [], []
for _ in range(reps):
    t_plan.append(timed(plan)[0])
    t_size.append(timed(sizes)[0])
    t, (out_len, in_used, status) = timed(decode)
    t_dec.append(t)
got = (summ.n_members, summ.total_out, summ.in_used, summ.status, summ.member_status)
same_plan = got == (n, n * MEMBER, length, 0, 0) and np.array_equal(in_off.cpu().numpy().view(np.uint64), offs) and np.array_equal(
    in_len.cpu().numpy().view(np.uint32), lens) and bool((out_cap == MEMBER).all())
same_sizes = bool((s_status == 2).all()) and bool((s_size == MEMBER).all()) and np.array_equal(s_used.cpu().numpy().view(np.uint32), lens)
same_bytes = bool((status == 2).all()) and np.array_equal(d_out.cpu().numpy(), pay)
pm, sm, dm = float(np.median(t_plan)), float(np.median(t_size)), float(np.median(t_dec))
print(f"gzip {n} members x {MEMBER} B ({length} bytes of members, {candidates} candidates), {reps} rounds: plan {pm:.3f} ms (min {min(t_plan):.3f}), "
      f"plain size pass {sm:.3f} ms (min {min(t_size):.3f}), batch decode {dm:.3f} ms (min {min(t_dec):.3f}); plan / size pass {pm / sm:.3f}, "
      f"size pass / decode {sm / dm:.3f}, (plan + decode) / decode {(pm + dm) / dm:.3f} (plan = known arrays: {same_plan}, sizes: {same_sizes}, "
      f"decoded = payload: {same_bytes})", flush=True)

# the same bytes as one unit: a unit's input is limited to 512 MiB and its output to 4 GiB - 1
ends = np.cumsum(lens, dtype=np.uint64)
k = int(min(np.searchsorted(ends, unit_mib << 20, side="right"), 0xFFFFFFFF // MEMBER, n))
if k == 0:
    print(f"one CHIP_F_MEMBERS unit: not measured, the first member does not fit {unit_mib} MiB", flush=True)
    sys.exit(0)
unit_in, unit_out = int(ends[k - 1]), k * MEMBER
i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
i32 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev).to(torch.int32)  # noqa: E731
d_out.zero_()


def unit(in_bytes, cap):
    return compu_amd.decode_batch(GZIP, d_in, i64(0), i32(in_bytes), d_out, i64(0), i32(cap), flags=compu_amd.F_MEMBERS)


unit(int(lens[0]), MEMBER)
torch.cuda.synchronize()
tu, (out_len, in_used, status) = timed(lambda: unit(unit_in, unit_out))
answer = (int(status[0]), int(out_len[0]) & 0xFFFFFFFF, int(in_used[0]) & 0xFFFFFFFF)
ok = answer == (2, unit_out, unit_in) and np.array_equal(d_out[:unit_out].cpu().numpy(), pay[:unit_out])
share = unit_in / length
print(f"one CHIP_F_MEMBERS unit over the first {k} members ({unit_in} bytes, {share:.3f} of the buffer): {tu:.3f} ms, x{tu / (share * (pm + dm)):.1f} of "
      f"that share of plan + batch decode, x{tu / (share * dm):.1f} of that share of the batch decode (decoded = payload: {ok})", flush=True)
