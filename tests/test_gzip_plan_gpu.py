"""The gzip member index on the GPU: chip_gzip_plan against the reference plan of every case (gzip_plan_ref.py: the walk of
include/compu_hip.h over the CPU oracle and the case's twin, pinned to zlib by tests/test_gzip_plan_cpu.py) and against the same
walk over the size pass itself (the contract to the letter); the plan's arrays through chip_decode_batch(CHIP_FMT_GZIP) against the
content and against the same bytes as one CHIP_F_MEMBERS unit; a file chip_encode_file(CHIP_FMT_GZIP) wrote; gzip_members_read;
two host threads on one stream; chip_trim; a decode on the inflate slot right behind a plan; member sizes at the 2^32 edge.
Without the feature every test here fails at the missing symbol."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import gzip_plan_cases as G
import gzip_plan_ref as R
from gzip_plan_cases import POISON32, POISON64, check_arrays

pytestmark = pytest.mark.gpu

GZIP, F_MEMBERS, NEED_INPUT, FINISHED = 31, 2, 0, 2
CASES = G.all_cases()
IDS = [c.name for c in CASES]


def upload(torch, data, shift=0, fill=0xA5):
    """`data` in a device tensor at a 4-byte aligned start `shift` bytes behind a 16-byte aligned one, padded to a multiple of 4;
    the bytes around it hold `fill`."""
    room = shift + (len(data) + 3) // 4 * 4 + 4
    t = torch.full((room,), fill, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t[shift:]


def gpu_plan(torch, lib, d_buf, length, max_members, room):
    """chip_gzip_plan into poisoned device arrays of `room` entries: (rows written, summary tuple, the four tensors)."""
    arrs = [torch.full((room,), POISON64, dtype=torch.int64, device="cuda"), torch.full((room,), POISON32, dtype=torch.int32, device="cuda"),
            torch.full((room,), POISON64, dtype=torch.int64, device="cuda"), torch.full((room,), POISON32, dtype=torch.int32, device="cuda")]
    s = G.new_summary()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.chip_gzip_plan(C.c_void_p(d_buf.data_ptr()) if length else None, length, max_members,
                            *[C.c_void_p(a.data_ptr()) if max_members else None for a in arrs], C.byref(s), stream)
    assert rc == 0
    host = [a.cpu().numpy().view(dt) for a, dt in zip(arrs, (np.uint64, np.uint32, np.uint64, np.uint32))]
    rows, summ = check_arrays(host, s, max_members)
    return rows, summ, arrs


def assert_plan(torch, lib, data, want, shift=0, max_members=None, fill=0xA5):
    """the plan of `data` equals want = (rows, summary), cut to max_members rows"""
    n = want[1][0]
    m = n + 2 if max_members is None else max_members
    got = gpu_plan(torch, lib, upload(torch, data, shift, fill), len(data), m, max(n, m) + 3)
    assert got[1] == want[1] and got[0] == want[0][:m]
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_equals_the_reference(gpu, case):
    import compu_amd

    lib, want = compu_amd.lib(), R.reference(case.name)
    n = len(case.data)
    assert_plan(gpu, lib, case.data, want, shift=4 * (n % 4))
    # what lies behind len completes no header: the padding holds the bytes that would (`1f 8b 08` + 00 is one)
    assert_plan(gpu, lib, case.data, want, shift=(8, 12, 0, 4)[n % 4], fill=0x00)
    assert_plan(gpu, lib, case.data, want, shift=0, fill=0x08)


def test_plan_is_the_walk_over_the_size_pass(gpu):
    """the contract to the letter: size1 is the unflagged chip_decode_batch_sizes over the device buffer"""
    import compu_amd

    lib = compu_amd.lib()
    i64 = lambda v: gpu.tensor([v], dtype=gpu.int64, device="cuda")  # noqa: E731
    i32 = lambda v: gpu.tensor([v], dtype=gpu.int32, device="cuda")  # noqa: E731
    for case in CASES:
        d_buf = upload(gpu, case.data)

        def size1(p, room):
            size, iu, st = compu_amd.decode_batch_sizes(GZIP, d_buf, i64(p), i32(room))
            return int(st[0]), int(size[0]), int(iu[0])

        want = R.walk(case.data, size1)
        assert want == R.reference(case.name), case.name  # (the size pass agrees with the oracle over the twin)
        n = want[1][0]
        got = gpu_plan(gpu, lib, d_buf, len(case.data), n + 1, n + 4)
        assert got[:2] == want, case.name


def test_plan_counts_then_fills_then_fills_a_part(gpu):
    import compu_amd

    lib = compu_amd.lib()
    for name, ms in (("header_fields", (0, 6, 2, 1, 9)), ("three_thousand_tiny", (0, 3000, 1, 1024, 1025, 2999, 3001)),
                     ("third_block_type_3", (0, 2, 1)), ("first_wrong_isize", (0, 1))):
        case, want = G.by_name(name), R.reference(name)
        for m in ms:
            assert_plan(gpu, lib, case.data, want, max_members=m)
    case, want = G.by_name("three_thousand_tiny"), R.reference("three_thousand_tiny")
    in_off, in_len, out_off, out_cap, summ = compu_amd.gzip_plan(upload(gpu, case.data), len(case.data))
    got = list(zip(in_off.tolist(), in_len.tolist(), out_off.tolist(), (out_cap.cpu().numpy().view(np.uint32)).tolist()))
    assert got == want[0] and summ.as_tuple() == want[1]
    assert compu_amd.gzip_plan(upload(gpu, case.data), len(case.data), max_members=7)[0].tolist() == [r[0] for r in want[0][:7]]
    assert compu_amd.gzip_plan(upload(gpu, b""), 0)[4].as_tuple() == (0, 0, 0, 0, 0)
    summ = compu_amd.gzip_plan(upload(gpu, G.by_name("third_wrong_fhcrc").data), len(G.by_name("third_wrong_fhcrc").data))[4]
    assert (summ.status, summ.member_status, summ.n_members) == (compu_amd.GzipPlanStatus.BadMember, -3, 2)


def test_plan_at_every_alignment(gpu):
    import compu_amd

    for name in ("starts_at_every_residue_mod_16", "chunk_boundary_straddled_by_3", "tile_boundary_straddled_by_2", "len_mod_4_is_3",
                 "third_trailing_3"):
        for shift in (0, 4, 8, 12):
            assert_plan(gpu, compu_amd.lib(), G.by_name(name).data, R.reference(name), shift=shift)


def members_decode(torch, d_buf, length, cap):
    """the first `length` bytes as ONE CHIP_FMT_GZIP unit with CHIP_F_MEMBERS: (output bytes, out_len, in_used, status)"""
    import compu_amd

    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")  # noqa: E731
    out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    ol, iu, st = compu_amd.decode_batch(GZIP, d_buf, i64(0), i32(length), out, i64(0), i32(cap), flags=F_MEMBERS)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()[:int(ol[0])], int(ol[0]), int(iu[0]), int(st[0])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_plans_arrays_decode_every_member(gpu, case):
    """the four arrays go unchanged to chip_decode_batch(CHIP_FMT_GZIP): every unit finishes with its content (a wrong CRC-32 is
    -3 there and its neighbours are fine), and the planned bytes as one CHIP_F_MEMBERS unit say the same"""
    import compu_amd

    d_buf = upload(gpu, case.data)
    rows, summ, arrs = assert_plan(gpu, compu_amd.lib(), case.data, R.reference(case.name))
    n, total, used = summ[0], summ[1], summ[2]
    content = b"".join(case.contents)
    assert n == len(case.contents) and total == len(content)
    if n == 0:
        return
    out = gpu.zeros(max(total, 4), dtype=gpu.uint8, device="cuda")
    out_len, in_used, status = compu_amd.decode_batch(GZIP, d_buf, arrs[0][:n], arrs[1][:n], out, arrs[2][:n], arrs[3][:n])
    gpu.cuda.synchronize()
    assert status.tolist() == [-3 if k in case.bad_crc else FINISHED for k in range(n)]
    assert out_len.tolist() == [r[3] for r in rows] and in_used.tolist() == [r[1] for r in rows]
    assert out.cpu().numpy().tobytes()[:total] == content  # (a member with a wrong CRC-32 still decodes to its bytes)
    got, ol, iu, st = members_decode(gpu, d_buf, used, total)
    if case.bad_crc:
        bad = min(case.bad_crc)
        upto = sum(r[3] for r in rows[:bad + 1])
        assert (got, ol, st) == (content[:upto], upto, -3)
    else:
        assert (got, ol, iu, st) == (content, total, used, FINISHED)


def test_a_file_the_writer_wrote_is_planned_and_decoded(gpu):
    """chip_encode_file(CHIP_FMT_GZIP) writes one member per unit: 1 MiB in units of 4 096 bytes is 256 members"""
    import compu_amd

    data = (G.text(700_000, 200) + G.noise(100_000, 201) + bytes(1 << 20))[: 1 << 20]
    d_in = upload(gpu, data)
    d_file, fs = compu_amd.encode_file(compu_amd.ZlibMode.Gzip, 6, d_in, len(data), unit_bytes=4096)
    assert fs.status == compu_amd.FileStatus.Ok and fs.n_units == 256
    out, (in_off, in_len, out_off, out_cap), summ = compu_amd.gzip_members_decode(d_file, fs.out_len)
    assert summ.as_tuple() == (256, 1 << 20, fs.out_len, G.OK, 0)
    assert out_cap.tolist() == [4096] * 256 and out_off.tolist() == [4096 * k for k in range(256)]
    assert int(in_off[0]) == 0 and (in_off[1:] == (in_off[:-1] + in_len[:-1])).all() and int(in_off[-1] + in_len[-1]) == fs.out_len
    assert out.cpu().numpy().tobytes() == data


def test_members_read_against_slicing(gpu):
    import compu_amd

    case = G.by_name("stored_fixed_dynamic_levels")
    content = b"".join(case.contents)
    sizes = [len(c) for c in case.contents]
    d_buf = upload(gpu, case.data, 8)
    a = sum(sizes[:4])  # the start of member 4
    ranges = [(a + 10, 500), (sizes[0] - 5, sizes[1] + 20), (0, 1), (len(content) - 3, 3), (a - 1, 2), (sum(sizes[:6]) + 7, 0), (0, sizes[0])]
    out, dst_off = compu_amd.gzip_members_read(d_buf, len(case.data), ranges)
    assert out.cpu().numpy().tobytes() == b"".join(content[lo:lo + ln] for lo, ln in ranges)
    assert dst_off.tolist() == [sum(r[1] for r in ranges[:i]) for i in range(len(ranges))]
    with pytest.raises(ValueError, match="outside the content"):
        compu_amd.gzip_members_read(d_buf, len(case.data), [(0, 4), (len(content) - 1, 2)])
    stop = G.by_name("third_trailing_zeros")
    with pytest.raises(ValueError, match="BadHeader"):
        compu_amd.gzip_members_read(upload(gpu, stop.data), len(stop.data), [(0, 4)])
    with pytest.raises(ValueError, match="BadHeader"):
        compu_amd.gzip_members_decode(upload(gpu, stop.data), len(stop.data))
    bad = G.by_name("third_wrong_crc")
    with pytest.raises(RuntimeError, match="member 2 "):
        compu_amd.gzip_members_decode(upload(gpu, bad.data), len(bad.data))
    got = compu_amd.gzip_members_read(upload(gpu, bad.data), len(bad.data), [(3, 50)])[0]  # member 0 alone is touched
    assert got.cpu().numpy().tobytes() == bad.contents[0][3:53]


def test_two_host_threads_plan_on_one_stream_and_trim(gpu):
    """The plan's slot is locked from its lookup to the last launch, and the size pass takes the inflate slot inside it: two
    threads with buffers of different sizes on the same stream get their own answers every time; chip_trim() releases both slots
    and the next plan allocates again."""
    import compu_amd

    lib = compu_amd.lib()
    names = ["three_thousand_tiny", "members_in_stored_payload"]
    files = [G.by_name(k).data for k in names]
    wants = [R.reference(k) for k in names]
    bufs = [upload(gpu, f) for f in files]
    gpu.cuda.synchronize()
    stream = gpu.cuda.current_stream()
    errors = []

    def work(k):
        try:
            with gpu.cuda.stream(stream):
                for _ in range(10):
                    n = wants[k][1][0]
                    assert gpu_plan(gpu, lib, bufs[k], len(files[k]), n, n + 3)[:2] == wants[k]
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    compu_amd.trim()
    for k in (1, 0):
        n = wants[k][1][0]
        assert gpu_plan(gpu, lib, bufs[k], len(files[k]), n, n + 3)[:2] == wants[k]


def test_a_decode_right_behind_a_plan_on_the_same_stream(gpu):
    """the size pass shares the inflate slot of the stream with chip_decode_batch: a small plan, a decode of more units than the
    plan had candidates (the slot grows), a larger plan, the decode again -- on a stream of their own"""
    import compu_amd

    lib = compu_amd.lib()
    big, small = G.by_name("three_thousand_tiny"), G.by_name("header_fields")
    stream = gpu.cuda.Stream()
    with gpu.cuda.stream(stream):
        d_big, d_small = upload(gpu, big.data), upload(gpu, small.data)
        rows, summ, arrs = assert_plan(gpu, lib, big.data, R.reference(big.name))
        content = b"".join(big.contents)
        for case, d_buf in ((small, d_small), (big, d_big), (small, d_small)):
            want = R.reference(case.name)
            n = want[1][0]
            assert gpu_plan(gpu, lib, d_buf, len(case.data), n, n + 3)[:2] == want
            out = gpu.zeros(len(content), dtype=gpu.uint8, device="cuda")
            out_len, in_used, status = compu_amd.decode_batch(GZIP, d_big, arrs[0][:3000], arrs[1][:3000], out, arrs[2][:3000], arrs[3][:3000],
                                                              stream=stream)
            stream.synchronize()
            assert (status == FINISHED).all() and out.cpu().numpy().tobytes() == content


@pytest.mark.parametrize("name", [e[0] for e in G.edge_cases()])
def test_member_sizes_at_the_2_pow_32_edge(gpu, name):
    """a member of 2^32 bytes is TOO_LARGE, one of 2^32 - 2 is a member with out_cap 0xFFFFFFFE, two of them put out_off[1] and
    total_out beyond 32 bits; the reference is arithmetic, and nothing is decoded"""
    import compu_amd

    data, rows, summ = {e[0]: e[1:] for e in G.edge_cases()}[name]
    t0 = time.perf_counter()
    got = assert_plan(gpu, compu_amd.lib(), data, (rows, summ))
    print(f"{name}: planned in {time.perf_counter() - t0:.2f} s")
    if name == "two_of_2_pow_32_minus_2":
        assert got[0][1][2] == 0xFFFFFFFE and got[1][1] == 2 * 0xFFFFFFFE > 1 << 32
