"""The zstd frame index on the GPU: chip_zstd_plan against chip_zstd_plan_host (itself pinned to the walk of zstd_plan_cases.py by
tests/test_zstd_plan_cpu.py) on every case; the plan's arrays through chip_decode_batch(CHIP_FMT_ZSTD) against the content and
against the same buffer as one CHIP_F_MEMBERS unit; zstd_frames_decode with its size pass; chip_layout_units against
numpy.cumsum; two host threads on one stream; chip_trim.  Without the feature every test here fails at the missing symbols."""
import ctypes as C
import threading

import numpy as np
import pytest

import zstd_plan_cases as Z
from zstd_plan_cases import POISON32, POISON64, check_arrays, host_plan

pytestmark = pytest.mark.gpu

FMT_ZSTD, F_MEMBERS, FINISHED = 100, 2, 2


def upload(torch, data, shift=0, fill=0xA5):
    """`data` in a device tensor at a 4-byte aligned start `shift` bytes behind a 16-byte aligned one, padded to a multiple of 4;
    the bytes around it hold `fill`."""
    room = shift + (len(data) + 3) // 4 * 4 + 4
    t = torch.full((room,), fill, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t[shift:]


def gpu_plan(torch, lib, d_buf, length, max_frames, room):
    """chip_zstd_plan into poisoned device arrays of `room` entries: (rows written, summary tuple, the four tensors)."""
    arrs = [torch.full((room,), POISON64, dtype=torch.int64, device="cuda"), torch.full((room,), POISON32, dtype=torch.int32, device="cuda"),
            torch.full((room,), POISON64, dtype=torch.int64, device="cuda"), torch.full((room,), POISON32, dtype=torch.int32, device="cuda")]
    s = Z.new_summary()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.chip_zstd_plan(C.c_void_p(d_buf.data_ptr()) if length else None, length, max_frames,
                            *[C.c_void_p(a.data_ptr()) if max_frames else None for a in arrs], C.byref(s), stream)
    assert rc == 0
    host = [a.cpu().numpy().view(dt) for a, dt in zip(arrs, (np.uint64, np.uint32, np.uint64, np.uint32))]
    rows, summ = check_arrays(host, s, max_frames)
    return rows, summ, arrs


def assert_same_plan(torch, lib, data, shift=0, max_frames=None, fill=0xA5):
    n = host_plan(lib, data, 0, 1)[1][0]
    m = n + 2 if max_frames is None else max_frames
    want = host_plan(lib, data, m, max(n, m) + 3)
    got = gpu_plan(torch, lib, upload(torch, data, shift, fill), len(data), m, max(n, m) + 3)
    assert got[1] == want[1] and got[0] == want[0]
    return got


@pytest.mark.parametrize("name,data", Z.all_files(), ids=[n for n, _ in Z.all_files()])
def test_plan_equals_host_plan(gpu, name, data):
    import compu_amd

    lib = compu_amd.lib()
    assert_same_plan(gpu, lib, data, shift=4 * (len(data) % 4))
    assert_same_plan(gpu, lib, data, shift=(8, 12, 0, 4)[len(data) % 4], fill=0xFD)  # the padding behind len completes no magic


@pytest.mark.parametrize("name,data", Z.block_cap_files(), ids=[n for n, _ in Z.block_cap_files()])
def test_plan_follows_2_pow_20_blocks_and_no_more(gpu, name, data):
    import compu_amd

    rows, summ, _ = assert_same_plan(gpu, compu_amd.lib(), data)
    assert summ[5] == (Z.TOO_LARGE if name.endswith("plus_1") else Z.OK)


def test_plan_counts_and_fills_part_of_a_buffer(gpu):
    import compu_amd

    data = dict(Z.all_files())["mixed_sized_unsized"]
    for m in (0, 2, 6, 9):
        assert_same_plan(gpu, compu_amd.lib(), data, max_frames=m)
    data = dict(Z.all_files())["nine_x_3000_mixed"]
    for m in (0, 1, 1024, 1025, 2000, 2001):
        assert_same_plan(gpu, compu_amd.lib(), data, max_frames=m)
    in_off, in_len, out_off, out_cap, summ = compu_amd.zstd_plan(upload(gpu, data), len(data))
    rows, want = Z.walk(data)
    got = list(zip(in_off.tolist(), in_len.tolist(), out_off.tolist(), (out_cap.cpu().numpy().view(np.uint32)).tolist()))
    assert got == rows and summ.as_tuple() == want
    assert compu_amd.zstd_plan(upload(gpu, b""), 0)[4].as_tuple() == (0, 0, 0, 0, 0, 0)


def test_plan_at_every_alignment(gpu):
    import compu_amd

    files = dict(Z.all_files())
    for name in ("nine_x_300", "chunk_boundary_shift_3", "tile_boundary_shift_2", "frame_at_end_of_last_block", "len_mod_4_is_3_frame_last"):
        for shift in (0, 4, 8, 12):
            rows, summ, _ = assert_same_plan(gpu, compu_amd.lib(), files[name], shift=shift)
            assert (rows, summ) == Z.walk(files[name])


def members_decode(torch, d_buf, length, cap):
    """the whole buffer as ONE CHIP_FMT_ZSTD unit with CHIP_F_MEMBERS: (output bytes, out_len, in_used, status)"""
    import compu_amd

    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")  # noqa: E731
    out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    ol, iu, st = compu_amd.decode_batch(FMT_ZSTD, d_buf, i64(0), i32(length), out, i64(0), i32(cap), flags=F_MEMBERS)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()[:int(ol[0])], int(ol[0]), int(iu[0]), int(st[0])


@pytest.mark.parametrize("name", ["sized_only", "eleven_hundred_sized"])
def test_the_plans_arrays_decode_every_frame(gpu, name):
    """no unsized frame: the four arrays go unchanged to chip_decode_batch(CHIP_FMT_ZSTD)"""
    import compu_amd

    buf, content = {n: (b, c) for n, b, c in Z.decodable()}[name]
    d_buf = upload(gpu, buf)
    rows, summ, arrs = assert_same_plan(gpu, compu_amd.lib(), buf)
    n = summ[0]
    assert summ[2] == 0 and summ[3] == len(content) and summ[5] == Z.OK
    out = gpu.zeros(max(summ[3], 4), dtype=gpu.uint8, device="cuda")
    out_len, in_used, status = compu_amd.decode_batch(FMT_ZSTD, d_buf, arrs[0][:n], arrs[1][:n], out, arrs[2][:n], arrs[3][:n])
    gpu.cuda.synchronize()
    assert (status.cpu().numpy() == FINISHED).all() and out_len.tolist() == [r[3] for r in rows] and in_used.tolist() == [r[1] for r in rows]
    assert out.cpu().numpy().tobytes()[:summ[3]] == content
    got, ol, iu, st = members_decode(gpu, d_buf, len(buf), len(content))
    assert (got, ol, iu, st) == (content, len(content), len(buf), FINISHED)


@pytest.mark.parametrize("name", [n for n, _, _ in Z.decodable()])
def test_frames_decode_equals_the_content_and_the_members_unit(gpu, name):
    """zstd_frames_decode: with unsized frames through the size pass and chip_layout_units"""
    import compu_amd

    buf, content = {n: (b, c) for n, b, c in Z.decodable()}[name]
    d_buf = upload(gpu, buf, 4)
    out, (in_off, in_len, out_off, out_cap), summ = compu_amd.zstd_frames_decode(d_buf, len(buf))
    rows, want = Z.walk(buf)
    assert summ.as_tuple() == want and out.cpu().numpy().tobytes() == content
    assert in_off.tolist() == [r[0] for r in rows] and in_len.tolist() == [r[1] for r in rows]
    assert (name in ("sized_only", "eleven_hundred_sized")) == (summ.n_unsized == 0)
    sizes = out_cap.tolist()
    assert out_off.tolist() == [sum(sizes[:i]) for i in range(len(sizes))] and sum(sizes) == len(content)
    assert all(r[3] in (Z.UNSIZED, s) for r, s in zip(rows, sizes))  # a stated size is the decoded size
    got, ol, iu, st = members_decode(gpu, d_buf, len(buf), len(content))
    assert (got, ol, iu, st) == (content, len(content), len(buf), FINISHED)


def test_a_damaged_third_frame(gpu):
    """per-frame statuses FINISHED, FINISHED, the error; the CHIP_F_MEMBERS unit reports the same error with out_len = the sum in
    front of it; zstd_frames_decode names the frame"""
    import compu_amd

    import zstd_writer as W

    good = [Z.part("fcs2"), Z.part("rle_raw_rle"), Z.part("fcs8")]
    bad = W.Frame(checksum=True).raw(Z.text(400, 3), last=True).finish(checksum_value=0x12345678)[0]  # a wrong XXH64: -22
    buf = good[0] + good[1] + bad + good[2]
    d_buf = upload(gpu, buf)
    rows, summ, arrs = assert_same_plan(gpu, compu_amd.lib(), buf)
    assert summ[0] == 4 and summ[5] == Z.OK
    out = gpu.zeros(summ[3], dtype=gpu.uint8, device="cuda")
    out_len, in_used, status = compu_amd.decode_batch(FMT_ZSTD, d_buf, arrs[0][:4], arrs[1][:4], out, arrs[2][:4], arrs[3][:4])
    gpu.cuda.synchronize()
    assert status.tolist() == [FINISHED, FINISHED, -22, FINISHED]
    got, ol, iu, st = members_decode(gpu, d_buf, len(buf), summ[3])
    assert st == -22 and ol == rows[0][3] + rows[1][3] + int(out_len[2])
    with pytest.raises(RuntimeError, match="frame 2 "):
        compu_amd.zstd_frames_decode(d_buf, len(buf))
    with pytest.raises(ValueError):  # a buffer that stops inside a frame is refused with its summary
        compu_amd.zstd_frames_decode(upload(gpu, buf[:-3]), len(buf) - 3)


@pytest.mark.parametrize("n", [0, 1, 1024, 1025, 3000])
def test_layout_units_equals_cumsum(gpu, n):
    import compu_amd

    rng = np.random.default_rng(n)
    sizes = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    if n:
        sizes[rng.integers(0, n, max(1, n // 7))] = 0
    if n >= 1024:
        sizes[[5, 1000, n - 1]] = [(1 << 32) + 5, 1 << 32, (1 << 40) + 1]  # clipped and counted
        sizes[[6, 1022]] = [(1 << 32) - 1, (1 << 32) - 2]  # the largest sizes a unit can hold
    d_size = gpu.from_numpy(sizes.view(np.int64)).cuda()
    out_off, out_cap, total, n_over = compu_amd.layout_units(d_size)
    want_off = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64) if n else sizes
    assert (out_off.cpu().numpy().view(np.uint64) == want_off).all()
    assert (out_cap.cpu().numpy().view(np.uint32) == np.minimum(sizes, 0xFFFFFFFF).astype(np.uint32)).all()
    assert total == int(sizes.sum()) and n_over == (3 if n >= 1024 else 0)
    assert (d_size.cpu().numpy().view(np.uint64) == sizes).all()  # the sizes are left as they were


def test_two_host_threads_plan_on_one_stream(gpu):
    """The slot is locked from its lookup to the last launch: two threads with buffers of different sizes (the scratch of one
    would not do for the other) on the same stream get their own answers every time; chip_trim() releases the slot and the next
    plan allocates again."""
    import compu_amd

    lib = compu_amd.lib()
    named = dict(Z.all_files())
    files = [named["nine_x_3000_mixed"], named["frame_in_raw_block"]]
    bufs = [upload(gpu, f) for f in files]
    wants = [host_plan(lib, f, Z.walk(f)[1][0], Z.walk(f)[1][0] + 3) for f in files]
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
    compu_amd.trim()  # the plan's slot is released with the others
    for k in range(2):
        n = wants[k][1][0]
        assert gpu_plan(gpu, lib, bufs[k], len(files[k]), n, n + 3)[:2] == wants[k]
    assert compu_amd.layout_units(gpu.tensor([3, 0, 4], dtype=gpu.int64, device="cuda"))[2:] == (7, 0)
