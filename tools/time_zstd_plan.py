"""Timing of the zstd frame index (chip_zstd_plan), of the chip_decode_batch(CHIP_FMT_ZSTD) of its arrays, and of the same buffer as ONE
CHIP_FMT_ZSTD unit with CHIP_F_MEMBERS, same process, same box:
python tools/time_zstd_plan.py [frames] [content KiB per frame] [repeats] [repeats of the single unit]
Builds a buffer of `frames` (default 4096) zstd frames of `content KiB` (default 256) of the bench payload generator
(bench_support.synth) each, compressed with the system libzstd at level 3 with checksum and content size on the host.  After two
warm-up rounds, `repeats` (default 10) rounds of plan, then batch decode, alternating, each timed with device events (the plan call is
synchronous, so its window is the whole call: kernels, the two waits and the host work between them).  The single unit is one wave
walking every frame: it is timed `repeats of the single unit` (default 1) times after a warm-up on the first frame alone, and not at all
when the buffer exceeds the 512 MiB a unit's input may have (halve `frames` then).  Prints the
median and the fastest of each, the number of magic-number candidates, and checks the plan against chip_zstd_plan_host and both
outputs against the payload."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from compu_amd.api import _ZstdPlanSummary  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
FRAME = (int(sys.argv[2]) if len(sys.argv) > 2 else 256) * 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
unit_reps = int(sys.argv[4]) if len(sys.argv) > 4 else 1
assert FRAME % synth.UNIT == 0
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
lib = compu_amd.lib()

pay = synth.payloads(n * FRAME // synth.UNIT, threads=threads)
mv = memoryview(pay)
zstd_index = next(i for i in range(64) if not (synth._splitmix64(i) & 1))  # an index that synth._mixed_one compresses with libzstd
with ThreadPoolExecutor(threads) as ex:
    parts = list(ex.map(lambda i: synth._mixed_one((mv[i * FRAME:(i + 1) * FRAME], zstd_index)), range(n)))
data = b"".join(parts)
first_len = len(parts[0])
del parts
length = len(data)
candidates = sum(data.count((0x184D2A50 | k).to_bytes(4, "little")) for k in range(16)) + data.count(b"\x28\xb5\x2f\xfd")
h_off, h_len, h_ooff, h_cap, h_sum = compu_amd.zstd_plan_host(data)
assert h_sum.n_frames == n and h_sum.n_unsized == 0 and h_sum.total_out == n * FRAME, h_sum
host = np.zeros((length + 3) // 4 * 4, np.uint8)
host[:length] = np.frombuffer(data, np.uint8)
d_in = torch.from_numpy(host).to(dev)
del data, host
in_off, out_off = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
in_len, out_cap = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
d_out = torch.zeros(n * FRAME, dtype=torch.uint8, device=dev)
summ = _ZstdPlanSummary()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def plan():
    rc = lib.chip_zstd_plan(p(d_in), length, n, p(in_off), p(in_len), p(out_off), p(out_cap), C.byref(summ), stream)
    assert rc == 0, rc


def decode():
    return compu_amd.decode_batch(compu_amd.FMT_ZSTD, d_in, in_off, in_len, d_out, out_off, out_cap)


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
got = (summ.n_frames, summ.n_skippable, summ.n_unsized, summ.total_out, summ.in_used, summ.status)
same_plan = got == h_sum.as_tuple() and all(
    np.array_equal(g.cpu().numpy().view(w.dtype), w) for g, w in ((in_off, h_off), (in_len, h_len), (out_off, h_ooff), (out_cap, h_cap)))
same_bytes = bool((status == 2).all()) and np.array_equal(d_out.cpu().numpy(), pay)
pm, dm = float(np.median(t_plan)), float(np.median(t_dec))
print(f"zstd {n} frames x {FRAME} B ({length} bytes of frames, {candidates} magic candidates), {reps} rounds: plan {pm:.3f} ms (min {min(t_plan):.3f}), "
      f"batch decode {dm:.3f} ms (min {min(t_dec):.3f}), ratio {pm / dm:.4f} (plan = host plan: {same_plan}, decoded = payload: {same_bytes})", flush=True)

# the same buffer as one unit: a unit's input is limited to 512 MiB and its output to 4 GiB - 1
if length > (512 << 20) - 64 or n * FRAME > 0xFFFFFFFF:
    print(f"one CHIP_F_MEMBERS unit: not measured, {length} bytes in / {n * FRAME} bytes out do not fit a unit", flush=True)
    sys.exit(0)
i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
i32 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev).to(torch.int32)  # noqa: E731
d_out.zero_()


def unit(in_bytes, cap):
    return compu_amd.decode_batch(compu_amd.FMT_ZSTD, d_in, i64(0), i32(in_bytes), d_out, i64(0), i32(cap), flags=compu_amd.F_MEMBERS)


unit(first_len, FRAME)
torch.cuda.synchronize()
t_unit = []
for _ in range(unit_reps):
    t, (out_len, in_used, status) = timed(lambda: unit(length, n * FRAME))
    t_unit.append(t)
answer = (int(status[0]), int(out_len[0]) & 0xFFFFFFFF, int(in_used[0]) & 0xFFFFFFFF)
ok = answer == (2, n * FRAME, length) and np.array_equal(d_out.cpu().numpy(), pay)
if not ok:
    diff = np.flatnonzero(d_out.cpu().numpy() != pay)
    print(f"one CHIP_F_MEMBERS unit answered (status, out_len, in_used) = {answer}, expected {(2, n * FRAME, length)}; "
          f"{diff.size} bytes differ, the first at {int(diff[0]) if diff.size else None}", flush=True)
um = float(np.median(t_unit))
print(f"one CHIP_F_MEMBERS unit, {unit_reps} launches: {um:.3f} ms (min {min(t_unit):.3f}), x{um / dm:.1f} of the batch decode (decoded = payload: {ok})",
      flush=True)
