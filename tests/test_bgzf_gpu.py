"""BGZF on the GPU: chip_bgzf_plan against chip_bgzf_plan_host (itself pinned to the walk of bgzf_cases.py) on faulty files,
decoys, deep chains and large blocks; bgzf_decode; the CHIP_FMT_BGZF encoder; the round trip on the device; two host threads on
one stream."""
import ctypes as C
import gzip
import os
import struct
import threading

import numpy as np
import pytest

import bgzf_cases as B
from bgzf_cases import POISON32, POISON64, check_arrays, host_plan

pytestmark = pytest.mark.gpu

FMT_BGZF, FINISHED, ENC_FINISHED, ENC_ERROR = 131, 2, 2, 3


def upload(torch, data, shift=0):
    """`data` in a device tensor at a 4-byte aligned start `shift` bytes behind a 16-byte aligned one, padded to a multiple of 4."""
    room = shift + (len(data) + 3) // 4 * 4 + 4
    t = torch.full((room,), 0xA5, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t[shift:]


def gpu_plan(torch, lib, d_buf, length, max_blocks, room):
    """chip_bgzf_plan into poisoned device arrays of `room` entries: (rows written, summary tuple, the four tensors)."""
    from compu_amd.api import _BgzfSummary

    arrs = [torch.full((room,), POISON64, dtype=torch.int64, device="cuda"), torch.full((room,), POISON32, dtype=torch.int32, device="cuda"),
            torch.full((room,), POISON64, dtype=torch.int64, device="cuda"), torch.full((room,), POISON32, dtype=torch.int32, device="cuda")]
    s = _BgzfSummary(7, 7, 7, 7, 7)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.chip_bgzf_plan(C.c_void_p(d_buf.data_ptr()) if length else None, length, max_blocks,
                            *[C.c_void_p(a.data_ptr()) if max_blocks else None for a in arrs], C.byref(s), stream)
    assert rc == 0
    host = [a.cpu().numpy().view(dt) for a, dt in zip(arrs, (np.uint64, np.uint32, np.uint64, np.uint32))]
    rows, summ = check_arrays(host, s, max_blocks)
    return rows, summ, arrs


def assert_same_plan(torch, lib, data, shift=0, max_blocks=None):
    n = B.walk(data)[1][0]
    m = n + 2 if max_blocks is None else max_blocks
    want = host_plan(lib, data, m, max(n, m) + 3)
    got = gpu_plan(torch, lib, upload(torch, data, shift), len(data), m, max(n, m) + 3)
    assert got[1] == want[1] and got[0] == want[0]
    return got


@pytest.mark.parametrize("name,data", B.plan_files(), ids=[n for n, _ in B.plan_files()])
def test_plan_equals_host_plan_on_every_cpu_file(gpu, name, data):
    import compu_amd

    rows, summ, _ = assert_same_plan(gpu, compu_amd.lib(), data, shift=4 * (len(data) % 4))
    assert (rows, summ) == B.walk(data)


def test_plan_counts_and_fills_part_of_a_file(gpu):
    import compu_amd

    data = dict(B.fault_files())["five_eof"]
    for m in (0, 2, 6, 9):
        assert_same_plan(gpu, compu_amd.lib(), data, max_blocks=m)
    in_off, in_len, out_off, out_cap, summ = compu_amd.bgzf_plan(upload(gpu, data), len(data))
    rows, want = B.walk(data)
    assert list(zip(in_off.tolist(), in_len.tolist(), out_off.tolist(), out_cap.tolist())) == rows and summ.as_tuple() == want


@pytest.mark.parametrize("name", sorted(B.decoy_files()))
def test_plan_drops_decoys(gpu, name):
    import compu_amd

    data = B.decoy_files()[name]
    for shift in (0, 12):
        rows, summ, _ = assert_same_plan(gpu, compu_amd.lib(), data, shift=shift)
        assert (rows, summ) == B.walk(data)


def test_plan_and_decode_of_a_deep_chain_at_every_alignment(gpu):
    import compu_amd

    data, payload = B.deep_file()
    want = B.walk(data)
    assert want[1][0] == 5001 and len(data) % 4 != 0  # >= 13 doubling levels
    for shift in (0, 4, 8, 12):
        rows, summ, _ = assert_same_plan(gpu, compu_amd.lib(), data, shift=shift)
        assert (rows, summ) == want
    out = compu_amd.bgzf_decode(upload(gpu, data, 8), len(data))
    assert out.cpu().numpy().tobytes() == payload


def test_plan_and_decode_of_large_stored_blocks(gpu):
    import compu_amd

    data, payload = B.large_file()
    d_buf = upload(gpu, data)
    rows, summ, arrs = assert_same_plan(gpu, compu_amd.lib(), data)
    assert (rows, summ) == B.walk(data) and summ[0] == 41
    n = summ[0]
    out = gpu.zeros(summ[1], dtype=gpu.uint8, device="cuda")
    out_len, in_used, status = compu_amd.decode_batch(compu_amd.ZlibMode.Gzip, d_buf, arrs[0][:n], arrs[1][:n], out, arrs[2][:n], arrs[3][:n])
    gpu.cuda.synchronize()
    assert (status.cpu().numpy() == FINISHED).all() and out_len.tolist() == [r[3] for r in rows] and in_used.tolist() == [r[1] for r in rows]
    assert out.cpu().numpy().tobytes() == payload


def test_decode_of_alice_written_by_zlib(gpu, alice):
    import compu_amd

    data = B.bgzf(B.cut(alice), level=6)
    out = compu_amd.bgzf_decode(upload(gpu, data), len(data))
    assert out.cpu().numpy().tobytes() == alice
    with pytest.raises(ValueError):  # a file that stops inside a block is refused with its summary
        compu_amd.bgzf_decode(upload(gpu, data[:-40]), len(data) - 40)
    broken = bytearray(data)
    broken[len(B.block(alice[:65280])) + 40] ^= 0x10  # damage inside the second block's body
    with pytest.raises(RuntimeError, match="block 1 "):
        compu_amd.bgzf_decode(upload(gpu, bytes(broken)), len(broken))


def encode_units(torch, units, level):
    """encode_batch(CHIP_FMT_BGZF) of `units`: (device input, output tensor, out_off, out_len, status as lists)."""
    import compu_amd

    in_off, at = [], 0
    for u in units:
        in_off.append(at)
        at += (len(u) + 15) // 16 * 16
    src = bytearray(at + 16)
    for o, u in zip(in_off, units):
        src[o:o + len(u)] = u
    cap = (compu_amd.encode_bound(FMT_BGZF, 65281) + 15) // 16 * 16
    d_in = torch.frombuffer(src, dtype=torch.uint8).cuda()
    d_out = torch.zeros(cap * len(units), dtype=torch.uint8, device="cuda")
    out_off = [cap * i for i in range(len(units))]
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    out_len, status = compu_amd.encode_batch(FMT_BGZF, level, d_in, i64(in_off), i32([len(u) for u in units]), d_out, i64(out_off),
                                             i32([cap] * len(units)))
    torch.cuda.synchronize()
    return d_in, d_out, out_off, out_len.tolist(), status.tolist()


def encoder_units(alice):
    rnd = np.random.default_rng(11).integers(0, 256, 65281, dtype=np.uint8).tobytes()
    return [b"", alice[:1], alice[:100], alice[:65280], rnd[:65280], rnd]


@pytest.mark.parametrize("level", [1, 6])
def test_encoder_writes_bgzf_blocks(gpu, alice, level):
    import compu_amd

    units = encoder_units(alice)
    _, d_out, out_off, out_len, status = encode_units(gpu, units, level)
    assert status[-1] == ENC_ERROR and out_len[-1] == 0  # 65 281 bytes: more than a block's payload
    out = d_out.cpu().numpy().tobytes()
    blocks = []
    for u, o, n, st in zip(units[:-1], out_off, out_len, status):
        blk = out[o:o + n]
        assert st == ENC_FINISHED and 28 <= n <= 65536
        xfl = 4 if level == 1 else 0
        assert blk[:16] == B.MAGIC + bytes([0, 0, 0, 0, xfl, 0xFF]) + B.BC
        assert struct.unpack("<H", blk[16:18])[0] + 1 == n and struct.unpack("<I", blk[-4:])[0] == len(u)
        assert gzip.decompress(blk) == u
        blocks.append(blk)
    data = b"".join(blocks) + compu_amd.bgzf_eof_block()
    *_, summ = compu_amd.bgzf_plan_host(data)
    assert summ.as_tuple() == (len(blocks) + 1, sum(len(u) for u in units[:-1]), len(data), B.OK, 1)
    assert B.walk(data)[1] == summ.as_tuple()


@pytest.mark.parametrize("level", [1, 6])
def test_round_trip_on_the_device(gpu, alice, level):
    import compu_amd

    units = encoder_units(alice)[:-1]
    _, d_out, out_off, out_len, status = encode_units(gpu, units, level)
    assert status == [ENC_FINISHED] * len(units)
    eof = gpu.frombuffer(bytearray(compu_amd.bgzf_eof_block()), dtype=gpu.uint8).cuda()
    d_file = gpu.cat([d_out[o:o + n] for o, n in zip(out_off, out_len)] + [eof, gpu.zeros(4, dtype=gpu.uint8, device="cuda")])
    length = sum(out_len) + 28
    in_off, in_len, out_off2, out_cap, summ = compu_amd.bgzf_plan(d_file, length)
    assert summ.as_tuple() == (len(units) + 1, sum(len(u) for u in units), length, B.OK, 1)
    assert in_len.tolist() == out_len + [28] and out_cap.tolist() == [len(u) for u in units] + [0]
    back = gpu.zeros(summ.total_out, dtype=gpu.uint8, device="cuda")
    got_len, _, st = compu_amd.decode_batch(compu_amd.ZlibMode.Gzip, d_file, in_off, in_len, back, out_off2, out_cap)
    gpu.cuda.synchronize()
    assert st.tolist() == [FINISHED] * (len(units) + 1) and got_len.tolist() == out_cap.tolist()
    assert back.cpu().numpy().tobytes() == b"".join(units)


def test_two_host_threads_plan_on_one_stream(gpu):
    """The slot is locked from its lookup to the last launch: two threads with files of different sizes (the scratch of one
    would not do for the other) on the same stream get their own answers every time."""
    import compu_amd

    lib = compu_amd.lib()
    files = [B.deep_file()[0], B.decoy_files()["a_chain_to_end"]]
    bufs = [upload(gpu, f) for f in files]
    wants = [host_plan(lib, f, B.walk(f)[1][0], B.walk(f)[1][0] + 3) for f in files]
    gpu.cuda.synchronize()
    stream = gpu.cuda.current_stream()
    errors = []

    def work(k):
        try:
            with gpu.cuda.stream(stream):
                for _ in range(20):
                    n = wants[k][1][0]
                    got = gpu_plan(gpu, lib, bufs[k], len(files[k]), n, n + 3)
                    assert got[:2] == wants[k]
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    compu_amd.trim()  # the plan's slots are released with the others
