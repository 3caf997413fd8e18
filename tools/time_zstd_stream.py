"""Timing of the slabbed decode of ONE zstd frame (chip_zstd_parallel_next), in one session on one card:
python tools/time_zstd_stream.py [frame MiB, comma separated] [large frame GiB] [repeats] [prefix MiB]
1. Slabs against one-shot.  For each frame size (default 128,512: MiB of the bench payload generator's content, compressed by the
   system libzstd at level 3 with checksum and content size -- what `zstd file` writes) the frame lies in device memory and is
   decoded by chip_zstd_parallel (the yardstick) and by chip_zstd_parallel_next in slabs of 16, 64 and 256 MiB of input, each with
   the checksum compared and waived: medians of `repeats` (default 5) whole decodes by the wall clock (every call is synchronous),
   every output compared with the payload.  The room of a call is what is left of the output buffer, at most 2^31 - 1 bytes.
2. Beyond the old limit.  One frame of `large frame GiB` (default 3; 0 skips the part) of content, which neither chip_zstd_parallel
   nor a unit of the batch decode takes, in slabs of 256 MiB, once with the checksum and once without.  Its yardstick is the
   streaming decoder (one wave) over the first `prefix MiB` (default 256) of content of the same frame, EXTRAPOLATED to the frame.
Then one slabbed decode of the first frame with CHIP_ZPAR_TIMING=1, in which the library waits behind every phase and prints it on
stderr: walk, tokens, place, each jump round with the words left after it, deliver, checksum, window."""
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

sizes = [float(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "128,512").split(",") if v]
big_gib = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
prefix_mib = int(sys.argv[4]) if len(sys.argv) > 4 else 256
threads = min(16, len(os.sched_getaffinity(0)))
dev = torch.device("cuda:0")
FINISHED, NEED_OUTPUT, NEED_INPUT = 2, 1, 0
ROOM_MAX = (1 << 31) - 1

z = C.CDLL("libzstd.so.1")
z.ZSTD_compressBound.restype = z.ZSTD_compress2.restype = C.c_size_t
z.ZSTD_compressBound.argtypes = [C.c_size_t]
z.ZSTD_createCCtx.restype = C.c_void_p
z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
z.ZSTD_CCtx_setParameter.restype = C.c_size_t
z.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]


def one_frame(pay):
    """the payload as one frame of the system libzstd: level 3, checksum, content size (worker threads where the library has them:
    still one frame, the same blocks)"""
    cctx = z.ZSTD_createCCtx()
    for param, value in ((100, 3), (201, 1), (200, 1)):
        z.ZSTD_CCtx_setParameter(cctx, param, value)
    z.ZSTD_CCtx_setParameter(cctx, 400, max(1, threads // 2))  # ZSTD_c_nbWorkers; an error (a library without them) changes nothing
    host = np.zeros(z.ZSTD_compressBound(pay.size), np.uint8)
    n = z.ZSTD_compress2(cctx, host.ctypes.data, host.size, pay.ctypes.data, pay.size)
    z.ZSTD_freeCCtx(cctx)
    assert not z.ZSTD_isError(C.c_size_t(n))
    return host[:n]


def payload(n_bytes):
    return synth.payloads(int(n_bytes) // synth.UNIT, threads=threads)


def slabbed(d_in, length, d_out, slab, checksum):
    """one whole decode: (calls, blocks)"""
    cur, pos, out_pos, calls, blocks = compu_amd.ZstdCursor(dev), 0, 0, 0, 0
    while True:
        room = d_out[out_pos:out_pos + ROOM_MAX]
        s = compu_amd.zstd_parallel_next(cur, d_in[pos:min(length, pos + slab)], room, checksum=checksum)
        calls, blocks, pos, out_pos = calls + 1, blocks + s.n_blocks, pos + s.in_used, out_pos + s.out_len
        if s.status == FINISHED:
            assert pos == length
            return calls, blocks, out_pos
        assert s.status in (NEED_INPUT, NEED_OUTPUT) and (s.in_used or s.out_len), s


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def same(d_out, pay):
    """the output against the payload, piece by piece on the host"""
    step = 256 << 20
    return all(np.array_equal(d_out[k:k + step].cpu().numpy(), pay[k:k + step]) for k in range(0, pay.size, step))


first = None
for mib in sizes:
    pay = payload(mib * (1 << 20))
    frame = one_frame(pay)
    length = frame.size
    d_in = torch.from_numpy(np.concatenate([frame, np.zeros((-length) % 4 + 4, np.uint8)])).to(dev)
    d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)
    if first is None:
        first = (d_in, length, d_out)
    print(f"one zstd frame: {mib:g} MiB of content in {length} bytes", flush=True)
    for checksum in (True, False):
        word = "compared" if checksum else "waived"
        compu_amd.zstd_parallel(d_in, length, d_out, checksum=checksum)
        ts = [wall(lambda: compu_amd.zstd_parallel(d_in, length, d_out, checksum=checksum))[0] for _ in range(reps)]
        one = float(np.median(ts))
        print(f"  chip_zstd_parallel, checksum {word}: {one:.2f} ms (min {min(ts):.2f}), {pay.size / one / 1e6:.2f} GB/s (decoded = payload: {same(d_out, pay)})",
              flush=True)
        for slab_mib in (16, 64, 256):
            d_out.zero_()
            slabbed(d_in, length, d_out, slab_mib << 20, checksum)
            runs = [wall(lambda: slabbed(d_in, length, d_out, slab_mib << 20, checksum)) for _ in range(reps)]
            ts = [r[0] for r in runs]
            m, (calls, blocks, out_len) = float(np.median(ts)), runs[-1][1]
            print(f"  chip_zstd_parallel_next, slabs of {slab_mib} MiB, checksum {word}: {m:.2f} ms (min {min(ts):.2f}) in {calls} calls, {blocks} blocks, "
                  f"{pay.size / m / 1e6:.2f} GB/s, {m - one:+.2f} ms = {(m - one) / calls:+.2f} ms per call against one-shot "
                  f"(decoded = payload: {out_len == pay.size and same(d_out, pay)})", flush=True)

if first is not None:
    d_in, length, d_out = first
    print("phases of one more slabbed decode of the first frame (64 MiB slabs, checksum compared), each waited for:", flush=True)
    os.environ["CHIP_ZPAR_TIMING"] = "1"
    slabbed(d_in, length, d_out, 64 << 20, True)
    del os.environ["CHIP_ZPAR_TIMING"]
    sys.stderr.flush()
    del d_in, d_out, first
    torch.cuda.empty_cache()

if big_gib > 0:
    pay = payload(big_gib * (1 << 30))
    t0 = time.perf_counter()
    frame = one_frame(pay)
    length = frame.size
    print(f"one zstd frame beyond the old limit: {pay.size} bytes ({pay.size / (1 << 30):.2f} GiB) of content in {length} bytes "
          f"(compressed on the host in {time.perf_counter() - t0:.1f} s)", flush=True)
    d_in = torch.from_numpy(frame).to(dev)
    d_out = torch.zeros(pay.size, dtype=torch.uint8, device=dev)
    raw = compu_amd.api._ZstdParallelSummary()
    if length <= 0xFFFFFFFF:
        rc = compu_amd.lib().chip_zstd_parallel(C.c_void_p(d_in.data_ptr()), length, C.c_void_p(d_out.data_ptr()), pay.size, 0, 0, C.byref(raw), None)
        print(f"  chip_zstd_parallel on it: rc {rc}, path {raw.path} (2 = refused), out_len {raw.out_len}", flush=True)
    for checksum in (True, False):
        d_out.zero_()
        ms, (calls, blocks, out_len) = wall(lambda: slabbed(d_in, length, d_out, 256 << 20, checksum))
        print(f"  chip_zstd_parallel_next, slabs of 256 MiB, checksum {'compared' if checksum else 'waived'}: {ms:.1f} ms in {calls} calls, {blocks} blocks, "
              f"{pay.size / ms / 1e6:.2f} GB/s (decoded = payload: {out_len == pay.size and same(d_out, pay)})", flush=True)
    # the yardstick: the streaming decoder, one wave, over a prefix of the same frame
    dec = compu_amd.decoder_interface.zstd_hip()
    want, got, pos = prefix_mib << 20, 0, 0
    out = np.zeros(8 << 20, np.uint8)
    data = frame.tobytes() if length < (1 << 30) else bytes(frame[:1 << 30])
    t0 = time.perf_counter()
    while got < want:
        r = dec.decode(data[pos:pos + (4 << 20)], out)
        assert r.is_ok(), r
        used = min(4 << 20, len(data) - pos) - r.input_remain
        made = out.size - r.output_remain
        assert np.array_equal(out[:made], pay[got:got + made])
        pos, got = pos + used, got + made
        assert used or made
    sec = time.perf_counter() - t0
    print(f"  streaming decoder (one wave) over the first {got / (1 << 20):.0f} MiB of content: {sec:.2f} s, {got / sec / 1e9:.3f} GB/s; "
          f"EXTRAPOLATED to the frame's {pay.size / (1 << 30):.2f} GiB: {sec * pay.size / got:.1f} s", flush=True)
