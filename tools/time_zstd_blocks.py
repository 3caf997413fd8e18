"""Timing of the block description of ONE large zstd frame (chip_zstd_blocks), and what it finds:
python tools/time_zstd_blocks.py [content MiB] [repeats] [yardstick]
Builds one frame of `content MiB` (default 512) of the bench payload generator (bench_support.synth), compressed with the system
libzstd at level 3 with checksum and content size on the host -- what `zstd file` writes.  After two warm-up calls, `repeats`
(default 10) calls of chip_zstd_blocks timed with device events (the call is synchronous, so its window is the whole call: three
kernels, the two waits and the host work between them); chip_zstd_blocks_host on the same bytes by the wall clock; the records of
both compared.  Prints what the blocks say about decoding them apart: how many reuse a table, and how far back its source lies.
With `yardstick` = 1 the frame is also decoded once as ONE unit of chip_decode_batch(CHIP_FMT_ZSTD) -- the one wave a frame is
today -- when it fits a unit (2^28 bytes of input).
With `yardstick` = xxh, instead of all that: the rate of XXH64 over the content on ONE wave, which a parallel decode of one frame
cannot split.  A frame of raw blocks of `content MiB` (at most 255) is decoded as one unit with and without Content_Checksum,
`repeats` times each; a raw block is a copy, so the difference of the two is the checksum."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import compu_amd  # noqa: E402
from bench_support import synth  # noqa: E402
from compu_amd.api import _ZstdBlocksSummary  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
yardstick = len(sys.argv) > 3 and sys.argv[3] == "1"
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
lib = compu_amd.lib()

pay = synth.payloads(mib * (1 << 20) // synth.UNIT, threads=threads)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


if len(sys.argv) > 3 and sys.argv[3] == "xxh":
    from oracle import oracle as O

    assert mib <= 255
    nb = pay.size // (128 << 10)
    body = np.empty((nb, 3 + (128 << 10)), np.uint8)
    body[:, :3] = np.frombuffer(((128 << 10) << 3).to_bytes(3, "little"), np.uint8)  # raw, not last
    body[:, 3:] = pay.reshape(nb, 128 << 10)
    body[-1, 0] |= 1
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev).to(torch.int32)  # noqa: E731
    d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)
    med = {}
    for checksum in (False, True):
        # window descriptor 0x50: 1 MiB; an 8-byte Frame_Content_Size
        head = b"\x28\xb5\x2f\xfd" + bytes([0xC0 | (4 if checksum else 0), 0x50]) + pay.size.to_bytes(8, "little")
        tail = (O.xxh64(pay.tobytes()) & 0xFFFFFFFF).to_bytes(4, "little") if checksum else b""
        frame = np.concatenate([np.frombuffer(head, np.uint8), body.reshape(-1), np.frombuffer(tail + bytes(8), np.uint8)])
        length = len(head) + body.size + len(tail)
        d_in = torch.from_numpy(frame[:(length + 3) // 4 * 4]).to(dev)
        run = lambda: compu_amd.decode_batch(compu_amd.FMT_ZSTD, d_in, i64(0), i32(length), d_out, i64(0), i32(pay.size))  # noqa: E731
        run()
        ts = []
        for _ in range(reps):
            t, (out_len, in_used, status) = timed(run)
            ts.append(t)
        ok = (int(status[0]), int(out_len[0]) & 0xFFFFFFFF, int(in_used[0]) & 0xFFFFFFFF) == (2, pay.size, length) and np.array_equal(d_out.cpu().numpy(), pay)
        med[checksum] = float(np.median(ts))
        print(f"{mib} MiB in {nb} raw blocks, one wave, checksum {'on' if checksum else 'off'}: {med[checksum]:.2f} ms (min {min(ts):.2f}, {reps} launches; "
              f"decoded = payload: {ok})", flush=True)
    d = med[True] - med[False]
    print(f"XXH64 on one wave: {d:.2f} ms, {pay.size / d / 1e6:.2f} GB/s; the copy of the raw blocks alone: {pay.size / med[False] / 1e6:.2f} GB/s", flush=True)
    sys.exit(0)

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

t0 = time.perf_counter()
h_blocks, h_sum = compu_amd.zstd_blocks_host(host[:length])
t_host = (time.perf_counter() - t0) * 1e3  # (count and fill: two walks)
n = h_sum.n_blocks
assert h_sum.status == 0 and h_sum.in_used == length and h_sum.content_size == pay.size, h_sum

d_in = torch.from_numpy(host).to(dev)
d_blocks = torch.zeros((n, 48), dtype=torch.uint8, device=dev)
summ = _ZstdBlocksSummary()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def describe():
    rc = lib.chip_zstd_blocks(C.c_void_p(d_in.data_ptr()), length, n, C.c_void_p(d_blocks.data_ptr()), C.byref(summ), stream)
    assert rc == 0, rc


for _ in range(2):
    describe()
ts = [timed(describe)[0] for _ in range(reps)]
same = d_blocks.cpu().numpy().tobytes() == h_blocks.tobytes() and compu_amd.ZstdBlocksSummary(summ).as_tuple() == h_sum.as_tuple()
print(f"one zstd frame, {mib} MiB of content in {length} bytes, {n} blocks, window {h_sum.window_size}: chip_zstd_blocks {np.median(ts):.3f} ms "
      f"(min {min(ts):.3f}, {reps} calls), host form {t_host:.3f} ms for count and fill (device records = host records: {same})", flush=True)

comp = h_blocks["type"] == 2
idx = np.arange(n)
print(f"blocks: {int((h_blocks['type'] == 0).sum())} raw, {int((h_blocks['type'] == 1).sum())} RLE, {int(comp.sum())} compressed; "
      f"{int(h_blocks['n_seq'].sum())} sequences, {int(h_blocks['lit_regen'].sum())} literal bytes "
      f"({int(h_blocks['lit_comp'][comp & (h_blocks['lit_type'] >= 2)].sum())} bytes of Huffman streams)")
needs = [comp & (h_blocks["lit_type"] == 3)] + [comp & (h_blocks["n_seq"] > 0) & (h_blocks["mode"][:, k] == 3) for k in range(3)]
for k, name in enumerate(("Huffman (treeless)", "LL repeat", "OF repeat", "ML repeat")):
    m = needs[k]
    back = (idx - h_blocks["src"][:, k])[m]
    missing = int((h_blocks["src"][:, k][m] < 0).sum())
    print(f"  {name}: {int(m.sum())} blocks reuse it" + (f", source {int(np.median(back))} blocks back in the median, {int(back.max())} at most" if m.any() else "")
          + (f", {missing} WITHOUT a source" if missing else ""))
alone = comp & ~(needs[0] | needs[1] | needs[2] | needs[3])
print(f"  {int(alone.sum())} compressed blocks reuse no table")

if yardstick:
    if length > (1 << 28) or pay.size > 0xFFFFFFFF:
        print(f"one unit: not measured, {length} bytes in / {pay.size} bytes out do not fit a zstd unit", flush=True)
        sys.exit(0)
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int64, device=dev).to(torch.int32)  # noqa: E731
    d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)
    first = int(h_blocks["offset"][1]) if n > 1 else length
    compu_amd.decode_batch(compu_amd.FMT_ZSTD, d_in, i64(0), i32(first), d_out, i64(0), i32(0))  # warm-up: the first block, no room
    torch.cuda.synchronize()
    t, (out_len, in_used, status) = timed(lambda: compu_amd.decode_batch(compu_amd.FMT_ZSTD, d_in, i64(0), i32(length), d_out, i64(0), i32(pay.size)))
    ok = (int(status[0]), int(out_len[0]) & 0xFFFFFFFF, int(in_used[0]) & 0xFFFFFFFF) == (2, pay.size, length) and np.array_equal(d_out.cpu().numpy(), pay)
    print(f"one unit of chip_decode_batch (one wave): {t:.1f} ms, {pay.size / t / 1e6:.3f} GB/s of content (decoded = payload: {ok})", flush=True)
