"""Timing of chip_zstd_parallel against the one wave a frame is without it, same process, same card:
python tools/time_zstd_parallel.py [content MiB] [repeats]
Builds ONE frame of `content MiB` (default 512) of the bench payload generator (bench_support.synth), compressed with the system
libzstd at level 3 with checksum and content size -- what `zstd file` writes.  Decodes it by
  the one-unit chip_decode_batch(CHIP_FMT_ZSTD), once (the yardstick; not possible when the frame exceeds the 2^28 bytes of a unit's input),
  chip_zstd_parallel with the checksum, `repeats` (default 5) times after a warm-up,
  chip_zstd_parallel with CHIP_ZPAR_NO_CHECKSUM, likewise,
each timed with device events around the synchronous call and compared with the payload.  Then one call of each kind with
CHIP_ZPAR_TIMING=1, in which the library waits behind every phase and prints it on stderr: describe, tokens, place, each jump round
with the words left after it, deliver, checksum."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402

mib = float(sys.argv[1]) if len(sys.argv) > 1 else 512  # (a multiple of 1/16: the generator makes units of 64 KiB)
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")

pay = synth.payloads(int(mib * (1 << 20)) // synth.UNIT, threads=threads)
z = C.CDLL("libzstd.so.1")
z.ZSTD_compressBound.restype = z.ZSTD_compress2.restype = C.c_size_t
z.ZSTD_compressBound.argtypes = [C.c_size_t]
z.ZSTD_createCCtx.restype = C.c_void_p
z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
z.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
cctx = z.ZSTD_createCCtx()
for param, value in ((100, 3), (201, 1), (200, 1)):  # level, checksum, content size
    z.ZSTD_CCtx_setParameter(cctx, param, value)
host = np.zeros((z.ZSTD_compressBound(pay.size) + 3) // 4 * 4, np.uint8)
length = z.ZSTD_compress2(cctx, host.ctypes.data, host.size, pay.ctypes.data, pay.size)
z.ZSTD_freeCCtx(cctx)
assert not z.ZSTD_isError(C.c_size_t(length))
host = host[:(length + 3) // 4 * 4]
host[length:] = 0
d_in = torch.from_numpy(host).to(dev)
d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def same():
    return bool(np.array_equal(d_out.cpu().numpy(), pay))


print(f"one zstd frame: {mib:g} MiB of content in {length} bytes", flush=True)
unit = None
if length <= (1 << 28) and pay.size <= 0xFFFFFFFF:
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev).to(torch.int32)  # noqa: E731
    compu_amd.decode_batch(compu_amd.FMT_ZSTD, d_in, i64(0), i32(length), d_out, i64(0), i32(0))  # warm-up: no room
    torch.cuda.synchronize()
    unit, (out_len, in_used, status) = timed(lambda: compu_amd.decode_batch(compu_amd.FMT_ZSTD, d_in, i64(0), i32(length), d_out, i64(0), i32(pay.size)))
    print(f"one unit of chip_decode_batch (one wave): {unit:.1f} ms, {pay.size / unit / 1e6:.3f} GB/s (status {int(status[0])}, decoded = payload: {same()})",
          flush=True)
else:
    print(f"one unit of chip_decode_batch: not possible, {length} bytes exceed the 2^28 of a zstd unit's input", flush=True)

for checksum in (True, False):
    d_out.zero_()
    compu_amd.zstd_parallel(d_in, length, d_out, checksum=checksum)
    ts = []
    for _ in range(reps):
        t, (out, summ) = timed(lambda: compu_amd.zstd_parallel(d_in, length, d_out, checksum=checksum))
        ts.append(t)
    m = float(np.median(ts))
    print(f"chip_zstd_parallel, checksum {'compared' if checksum else 'waived'}: {m:.2f} ms (min {min(ts):.2f}, {reps} calls), {pay.size / m / 1e6:.2f} GB/s"
          + (f", x{unit / m:.1f} of the one wave" if unit else "") + f"; {summ!r} (decoded = payload: {same()})", flush=True)
    print("  phases of one more call, each waited for:", flush=True)
    os.environ["CHIP_ZPAR_TIMING"] = "1"
    compu_amd.zstd_parallel(d_in, length, d_out, checksum=checksum)
    del os.environ["CHIP_ZPAR_TIMING"]
    sys.stderr.flush()
